"""Command-line entry points (reference: code/main/train.py, train_alter.py, test.py)."""
