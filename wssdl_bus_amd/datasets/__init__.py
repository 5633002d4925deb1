"""Evaluation (reference code/lib/datasets): AP, CorLoc and FROC counts of detections, and the recall of RPN proposals,
on the device."""
from .recall import (AREAS, AREA_RANGES, evaluate_recall_host, evaluate_recall_table, pack_recall_gt)  # noqa: F401
from .voc_eval_bus import (DetectionAccumulator, FROC_THRESHOLDS, eval_detections, evaluate_detections, flatten_batched,  # noqa: F401
                           pack_gt, voc_ap)
