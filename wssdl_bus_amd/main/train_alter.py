"""python -m wssdl_bus_amd.main.train_alter: alternating training (reference code/main/train_alter.py) -- an argument
parser over fast_rcnn.train_bus.train_net_alter."""
from ..fast_rcnn.train_bus import train_net_alter
from ._common import run_training, train_parser


def parser():
    return train_parser('Train a Faster R-CNN network on alternating mini-batches', 'Resnet_train_alter')


def main(argv=None):
    args = parser().parse_args(argv)
    return run_training(args, train_net_alter)


if __name__ == '__main__':
    main()
