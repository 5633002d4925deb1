#!/usr/bin/env python3
"""Golden vectors for the data layers: tests/golden/data_layer.npz.

Runs ONLY where the reference tree is present.  Stages the reference's own roi_data_layer/layer_bus.py,
layer_bus_joint.py, minibatch_bus.py and utils/blob.py in a scratch copy (lib2to3; fast_rcnn/config.py beside them, as
make_golden_image.py does for the last two) and runs them with the same `skimage` stand-in, rotation off:
skimage.io.imread hands back the synthetic plane registered under the entry's "file name", skimage.transform.resize
is the nearest-neighbour stand-in.  Stored per forward: the db indices, im_scales, the shapes handed to and asked of
the resize, gt_boxes, num_gt_boxes, im_info; per run one np.random.random_sample() taken after the last forward,
which pins the number and order of the draws.  Results only: the roidbs are regenerated from data_layer_inputs.py."""
import importlib
import os
import shutil
import subprocess
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ref_python_stage as stage  # noqa: E402

from data_layer_inputs import FORWARDS, IMS_PER_BATCH, SEED, WS_IMS_PER_BATCH, make_roidbs  # noqa: E402
from image_inputs import nearest  # noqa: E402


def main():
    root = stage.stage()
    os.makedirs(os.path.join(root, "roi_data_layer"), exist_ok=True)
    open(os.path.join(root, "roi_data_layer", "__init__.py"), "w").close()
    for rel in ("utils/blob.py", "roi_data_layer/minibatch_bus.py", "roi_data_layer/layer_bus.py",
                "roi_data_layer/layer_bus_joint.py"):
        dst = os.path.join(root, rel)
        shutil.copy(os.path.join(stage.LIB, rel), dst)
        subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n", dst],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    roidb_s, roidb_ws, planes = make_roidbs()
    calls = []
    sk = types.ModuleType("skimage")
    sk.transform = types.ModuleType("skimage.transform")
    sk.io = types.ModuleType("skimage.io")

    def resize(im, shape, *a, **k):
        shape = tuple(int(s) for s in shape)
        calls.append((tuple(im.shape[:2]), shape))
        return nearest(im, shape)
    sk.transform.resize = resize
    sk.io.imread = lambda path: planes[path]
    sys.modules["skimage"] = sk
    sys.modules["skimage.transform"] = sk.transform
    sys.modules["skimage.io"] = sk.io
    cfg = importlib.import_module("fast_rcnn.config").cfg
    mb = importlib.import_module("roi_data_layer.minibatch_bus")
    lb = importlib.import_module("roi_data_layer.layer_bus")
    lj = importlib.import_module("roi_data_layer.layer_bus_joint")
    cfg.TRAIN.USE_ROTATION = False                  # skimage.transform.rotate is not pinnable
    cfg.TRAIN.IMS_PER_BATCH = IMS_PER_BATCH
    cfg.TRAIN.WS_IMS_PER_BATCH = WS_IMS_PER_BATCH
    scales = []
    for name in ("_get_image_blob", "_get_image_blob_joint"):
        def wrap(f):
            def g(*a, **k):
                blob, s = f(*a, **k)
                scales.append(list(s))
                return blob, s
            return g
        setattr(mb, name, wrap(getattr(mb, name)))
    out = {}
    for train in (True, False):
        for kind in ("joint", "s", "ws"):
            np.random.seed(SEED)
            if kind == "joint":
                layer = lj.RoIDataLayerJoint(roidb_s, roidb_ws, "Resnet_train", 3, train)
            else:
                layer = lb.RoIDataLayer(roidb_s if kind == "s" else roidb_ws, "Resnet_train", 3, train, kind == "ws")
            inds = []
            orig = layer._get_next_minibatch_inds

            def logged(orig=orig, inds=inds):
                r = orig()
                inds.append(np.concatenate([np.asarray(x) for x in r]) if isinstance(r, tuple) else np.asarray(r))
                return r
            layer._get_next_minibatch_inds = logged
            for f in range(FORWARDS):
                del calls[:], scales[:]
                blobs = layer.forward()
                key = "%s_%d/f%d/" % (kind, int(train), f)
                out[key + "inds"] = inds[-1].astype(np.int64)
                out[key + "im_scales"] = np.array(scales[0], np.float64)
                out[key + "pre_shapes"] = np.array([c[0] for c in calls], np.int64)
                out[key + "resize_shapes"] = np.array([c[1] for c in calls], np.int64)
                out[key + "blob_shape"] = np.array(blobs["data"].shape, np.int64)
                for k in ("gt_boxes", "num_gt_boxes", "im_info"):
                    out[key + k] = blobs[k]
                assert blobs["gt_boxes"].dtype == np.float32 and blobs["num_gt_boxes"].dtype == np.int32
                assert blobs["im_info"].dtype == np.float32
            out["%s_%d/trailing" % (kind, int(train))] = np.array([np.random.random_sample()])
    path = os.path.join(ROOT, "tests", "golden", "data_layer.npz")
    np.savez_compressed(path, **out)
    print(path, len(out), "arrays,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
