#!/usr/bin/env python3
"""train_net for a few iterations on the temporary BUS-layout data set that tools/data_layer_demo.py writes: the data
layers, the joint train steps, a validation pass with CorLoc, log.txt / summary.jsonl, the device-drawn result pictures,
snapshots, and a second run resumed from the first of them.

    python tools/train_demo.py [--iters 4] [--depth 18] [--alter] [--keep DIR]"""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--depth", type=int, default=18)
    ap.add_argument("--alter", action="store_true", help="the alternating loop (train_net_alter)")
    ap.add_argument("--keep", default=None, help="copy the output directory here")
    a = ap.parse_args()
    from data_layer_demo import write_dataset
    from wssdl_bus_amd.datasets.factory_bus import get_imdb
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.train_bus import get_test_roidb, get_training_roidb, train_net, train_net_alter
    from wssdl_bus_amd.networks.factory_bus import get_network
    name = "Resnet_train_alter" if a.alter else "Resnet_train"
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root)
        cfg.DATA_DIR = root
        cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = 2, 2
        cfg.TRAIN.DISPLAY, cfg.TRAIN.SNAPSHOT_ITERS, cfg.TRAIN.TEST_ITERS = 1, 2, 2
        np.random.seed(cfg.RNG_SEED)
        torch.manual_seed(cfg.RNG_SEED)
        imdb_s, imdb_ws, imdb_t = get_imdb("bus_s_train"), get_imdb("bus_ws_train"), get_imdb("bus_s_train")
        roidb_s, roidb_ws, roidb_t = get_training_roidb(imdb_s), get_training_roidb(imdb_ws), get_test_roidb(imdb_t)
        out = os.path.join(root, "out")
        train = train_net_alter if a.alter else train_net

        def net():
            n = get_network(name, a.depth).cuda().to(memory_format=torch.channels_last)
            n.train()
            return n
        hist = train(net(), imdb_s, roidb_s, imdb_ws, roidb_ws, imdb_t, roidb_t, out, max_iters=a.iters, vis=True, val_ims_per_batch=2)
        print(open(os.path.join(out, "log.txt")).read())
        pictures = sorted(os.listdir(os.path.join(out, "test")))
        print("%d validation(s), %d snapshot(s), %d picture(s): %s ..." % (len(hist["validations"]), len(hist["snapshots"]),
                                                                          len(pictures), pictures[:3]))
        # a second run, resumed from the first snapshot (the same settings: another max_iters would be refused)
        again = train(net(), imdb_s, roidb_s, imdb_ws, roidb_ws, imdb_t, roidb_t, out, max_iters=a.iters, vis=False,
                      val_ims_per_batch=2, resume=hist["snapshots"][0])
        print("resumed from %s: %d validation(s), %d snapshot(s)" % (os.path.basename(hist["snapshots"][0]), len(again["validations"]),
                                                                     len(again["snapshots"])))
        if a.keep:
            shutil.copytree(out, a.keep, dirs_exist_ok=True)
    print("train_demo ok")


if __name__ == "__main__":
    main()
