"""The BUS image database: what the reference's datasets/bus.py and datasets/imdb.py give the data layers, restated.

Layout under `data_path`: ImageSets/Main/<set>.txt lists the image names, TIFFImages/<name>.tif holds the 8-bit grey
images, Annotations/<name>.xml the VOC-style boxes plus one <BIRADS><diag> element per image.  An annotation becomes
one [k, 5] integer table (x1, y1, x2, y2, class) parsed object by object; every array of the roidb entry is cut from
that table.  Behaviour pinned by tests/test_data_layer_cpu.py: 0-based coordinates stored as uint16, objects marked
difficult dropped, class names matched lower-cased and stripped, birads_diag = diag + 1, dense gt_overlaps, no cache."""
import os
import xml.etree.ElementTree as ET

import numpy as np
from PIL import Image

from ..fast_rcnn.config import cfg

CLASSES = ('__background__', 'benign', 'malignant')
_SUBDIR = {'image': ('TIFFImages', '.tif'), 'annotation': ('Annotations', '.xml'), 'set': (os.path.join('ImageSets', 'Main'), '.txt')}


def object_row(obj, class_index):
    """One <object> -> (x1, y1, x2, y2, class) with 0-based corners, or None for an object marked difficult."""
    if int(obj.findtext('difficult')) != 0:
        return None
    box = obj.find('bndbox')
    corners = [float(box.findtext(tag)) - 1 for tag in ('xmin', 'ymin', 'xmax', 'ymax')]
    return corners + [class_index[obj.findtext('name').lower().strip()]]


def read_annotation(path, classes=CLASSES):
    """An annotation file -> the roidb entry of an unflipped image."""
    class_index = {name: k for k, name in enumerate(classes)}
    root = ET.parse(path).getroot()
    rows = [r for r in (object_row(o, class_index) for o in root.iter('object')) if r is not None]
    table = np.asarray(rows, dtype=np.float64).reshape(len(rows), 5)
    labels = table[:, 4].astype(np.int32)
    spans = table[:, 2:4] - table[:, 0:2] + 1
    return dict(boxes=table[:, :4].astype(np.uint16), gt_classes=labels,
                gt_overlaps=np.eye(len(classes), dtype=np.float32)[labels],
                seg_areas=(spans[:, 0] * spans[:, 1]).astype(np.float32), flipped=False,
                birads_diag=int(root.find('BIRADS').findtext('diag')) + 1)


def mirror_boxes(boxes, width):
    """Boxes of the horizontally mirrored image of `width` columns: (x1, x2) -> (width - 1 - x2, width - 1 - x1)."""
    out = np.asarray(boxes).astype(np.int64)
    out[:, [0, 2]] = int(width) - 1 - out[:, [2, 0]]
    if (out[:, [0, 2]] < 0).any():
        raise ValueError("a box lies outside an image %d columns wide" % width)
    return out.astype(np.asarray(boxes).dtype)


class bus(object):
    """bus(image_set, data_path): classes, num_classes, image_index, image_path_at, gt_roidb(), roidb,
    append_flipped_images()."""

    def __init__(self, image_set, data_path=None):
        self.name = 'bus_' + image_set
        self.classes = CLASSES
        self._root = cfg.DATA_DIR if data_path is None else data_path
        with open(self._file('set', image_set)) as f:
            self._names = [line.strip() for line in f.read().splitlines()]
        self._roidb = None

    def _file(self, kind, name):
        sub, ext = _SUBDIR[kind]
        path = os.path.join(self._root, sub, name + ext)
        if not os.path.exists(path):
            raise IOError("%s: no such %s file" % (path, kind))
        return path

    num_classes = property(lambda self: len(self.classes))
    image_index = property(lambda self: self._names)
    num_images = property(lambda self: len(self._names))

    def image_path_at(self, i):
        return self._file('image', self._names[i])

    def gt_roidb(self):
        """One entry per listed image, read from the annotations on every call."""
        return [read_annotation(self._file('annotation', name), self.classes) for name in self._names]

    @property
    def roidb(self):
        if self._roidb is None:
            self._roidb = self.gt_roidb()
        return self._roidb

    def _width(self, i):
        with Image.open(self.image_path_at(i)) as im:
            return im.size[0]

    def append_flipped_images(self):
        """Doubles the database: image i gets a twin at num_images + i with 'flipped' set and mirrored boxes; the
        twin shares the labels, overlaps and birads_diag of its original."""
        twins = [dict({k: e[k] for k in ('gt_overlaps', 'gt_classes', 'birads_diag')}, flipped=True,
                      boxes=mirror_boxes(e['boxes'], self._width(i))) for i, e in enumerate(self.roidb)]
        self.roidb.extend(twins)
        self._names = self._names + self._names

    def evaluate_recall(self, candidate_boxes=None, thresholds=None, area='all', limit=None):
        """imdb.py:125-213 with the reference's signature and return dict ('ar', 'recalls', 'thresholds',
        'gt_overlaps'): one cell of recall.evaluate_recall_table -- the device op where a GPU is present, otherwise
        recall.evaluate_recall_host, the same arithmetic in NumPy.  candidate_boxes=None evaluates the roidb's
        gt_classes == 0 rows.  A flipped roidb raises KeyError ('seg_areas'), as in the reference."""
        import torch
        from . import recall
        assert area in recall.AREAS, 'unknown area range: {}'.format(area)
        roidb = self.roidb[:self.num_images]
        gt = recall.pack_recall_gt(roidb)
        boxes = recall.non_gt_boxes(roidb) if candidate_boxes is None else [candidate_boxes[i] for i in range(self.num_images)]
        table = recall.evaluate_recall_table if torch.cuda.is_available() else recall.evaluate_recall_host
        cell = table(boxes, gt, areas=(area,), limits=(limit,), thresholds=thresholds)[(area, limit)]
        return {k: cell[k] for k in ('ar', 'recalls', 'thresholds', 'gt_overlaps')}
