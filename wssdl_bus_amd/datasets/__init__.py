"""Evaluation of detections (reference code/lib/datasets): AP, CorLoc and FROC counts on the device."""
from .voc_eval_bus import (DetectionAccumulator, FROC_THRESHOLDS, eval_detections, evaluate_detections, flatten_batched,  # noqa: F401
                           pack_gt, voc_ap)
