"""prepare_roidb: the keys a roidb entry gains before training (the reference's roi_data_layer/roidb.py; its
add_bbox_regression_targets belongs to the non-RPN path and is not part of this package)."""
import numpy as np
from PIL import Image


def prepare_roidb(imdb):
    """Every entry of imdb.roidb gets 'image' (its file), 'width', 'height', and per box the class of largest overlap
    ('max_classes') with that overlap ('max_overlaps')."""
    for i, entry in enumerate(imdb.roidb):
        path = imdb.image_path_at(i)
        with Image.open(path) as im:
            width, height = im.size
        overlaps = entry['gt_overlaps']
        overlaps = overlaps.toarray() if hasattr(overlaps, 'toarray') else np.asarray(overlaps)
        entry.update(image=path, width=width, height=height, max_classes=overlaps.argmax(axis=1),
                     max_overlaps=overlaps.max(axis=1))
