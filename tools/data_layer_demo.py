#!/usr/bin/env python3
"""README's usage text, run end to end with nothing but this package: a tiny BUS-layout data set is written to a
temporary directory (8-bit grey TIFFs, VOC-style XML with <BIRADS><diag>, image-set files), read by
datasets.factory_bus.get_imdb, turned into training roidbs, and fed by RoIDataLayerJoint.forward() into
SolverWrapper.train_step_joint for a few steps.

    python tools/data_layer_demo.py [--steps 3] [--depth 18]"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

XML = ("<annotation><filename>%s.tif</filename><size><width>%d</width><height>%d</height><depth>1</depth></size>"
       "<BIRADS><diag>%d</diag></BIRADS>%s</annotation>")
OBJ = ("<object><name>%s</name><difficult>0</difficult><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax>"
       "<ymax>%d</ymax></bndbox></object>")


def write_dataset(root, n_s=6, n_ws=6, seed=0):
    from PIL import Image
    rs = np.random.RandomState(seed)
    for d in ("Annotations", "TIFFImages", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(root, d))
    for split, n in (("s_train", n_s), ("ws_train", n_ws)):
        names = []
        for i in range(n):
            name = "%s_%03d" % (split, i)
            h, w = int(rs.randint(140, 200)), int(rs.randint(200, 280))
            low = rs.uniform(0.2, 1.0, size=(h // 32 + 2, w // 32 + 2))
            plane = np.clip(rs.rayleigh(40.0, size=(h, w)) * np.kron(low, np.ones((32, 32)))[:h, :w], 0, 255).astype(np.uint8)
            Image.fromarray(plane).save(os.path.join(root, "TIFFImages", name + ".tif"))
            diag = int(rs.randint(0, 2))
            x, y = int(rs.randint(5, w // 2)), int(rs.randint(5, h // 2))
            objs = OBJ % (("benign", "malignant")[diag], x, y, x + int(rs.randint(30, w // 2 - 5)), y + int(rs.randint(30, h // 2 - 5)))
            objs += OBJ % ("__background__", 2, 2, w // 3, h // 3)
            with open(os.path.join(root, "Annotations", name + ".xml"), "w") as f:
                f.write(XML % (name, w, h, diag, objs))
            names.append(name)
        with open(os.path.join(root, "ImageSets", "Main", split + ".txt"), "w") as f:
            f.write("\n".join(names) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=18)
    a = ap.parse_args()
    from wssdl_bus_amd.datasets.factory_bus import get_imdb
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.train_bus import SolverWrapper, get_data_layer, get_training_roidb
    from wssdl_bus_amd.networks.factory_bus import get_network
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root)
        cfg.DATA_DIR = root
        cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = 2, 2
        np.random.seed(cfg.RNG_SEED)
        torch.manual_seed(cfg.RNG_SEED)
        # ---- README's usage text from here ----
        imdb_s, imdb_ws = get_imdb("bus_s_train"), get_imdb("bus_ws_train")
        roidb_s, roidb_ws = get_training_roidb(imdb_s), get_training_roidb(imdb_ws)
        net = get_network("Resnet_train", a.depth).cuda().to(memory_format=torch.channels_last)
        net.train()
        solver = SolverWrapper(net)
        layer = get_data_layer((roidb_s, roidb_ws), "Resnet_train", imdb_s.num_classes, True, is_joint=True)
        for it in range(a.steps):
            blobs = layer.forward()
            losses = solver.train_step_joint(blobs)
            loss = float(losses["loss"].detach())
            print("step %d  data %s  loss %.4f" % (it, list(blobs["data"].shape), loss), flush=True)
            assert np.isfinite(loss)
    print("data_layer_demo ok: %d + %d roidb entries" % (len(roidb_s), len(roidb_ws)))


if __name__ == "__main__":
    main()
