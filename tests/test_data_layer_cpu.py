"""The host side of the data layers, no GPU: index logic and the mini-batch plans against the reference's own
layer_bus.py / layer_bus_joint.py / minibatch_bus.py (tests/golden/data_layer.npz, made by
tests/golden/make_golden_data_layer.py with rotation off), the draws with rotation on against the NumPy oracle's
consumption of the same stream, and the dataset reader on annotations written in the sample files' layout."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden
from oracle import np_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from data_layer_inputs import FORWARDS, IMS_PER_BATCH, SEED, WS_IMS_PER_BATCH, make_roidbs  # noqa: E402
from image_inputs import nearest  # noqa: E402


@pytest.fixture
def cfg(monkeypatch):
    from wssdl_bus_amd.fast_rcnn.config import cfg
    monkeypatch.setattr(cfg.TRAIN, "IMS_PER_BATCH", IMS_PER_BATCH)
    monkeypatch.setattr(cfg.TRAIN, "WS_IMS_PER_BATCH", WS_IMS_PER_BATCH)
    return cfg


@pytest.fixture(scope="module")
def roidbs():
    roidb_s, roidb_ws, planes = make_roidbs()
    for db in (roidb_s, roidb_ws):
        for e in db:
            e["plane"] = planes[e.pop("image")]
    return roidb_s, roidb_ws


@pytest.mark.parametrize("use_rng", (False, True))
@pytest.mark.parametrize("train", (True, False))
@pytest.mark.parametrize("kind", ("joint", "s", "ws"))
def test_layers_and_plans_reproduce_the_reference(cfg, monkeypatch, roidbs, kind, train, use_rng):
    from wssdl_bus_amd.roi_data_layer import minibatch_bus as M
    from wssdl_bus_amd.roi_data_layer.layer_bus import RoIDataLayer
    from wssdl_bus_amd.roi_data_layer.layer_bus_joint import RoIDataLayerJoint
    monkeypatch.setattr(cfg.TRAIN, "USE_ROTATION", False)
    g = load_golden("data_layer")
    roidb_s, roidb_ws = roidbs
    state = np.random.get_state()
    try:
        if use_rng:
            rng = np.random.RandomState(SEED)
        else:                                   # the default: NumPy's global legacy stream, like the reference
            rng = None
            np.random.seed(SEED)
        if kind == "joint":
            layer = RoIDataLayerJoint(roidb_s, roidb_ws, "Resnet_train", 3, train, rng=rng)
        else:
            db = roidb_s if kind == "s" else roidb_ws
            layer = RoIDataLayer(db, "Resnet_train", 3, train, kind == "ws", rng=rng)
        seen = []
        for f in range(FORWARDS):
            key = "%s_%d/f%d/" % (kind, int(train), f)
            inds = layer._get_next_minibatch_inds()
            if kind == "joint":
                assert np.array_equal(np.concatenate(inds), g[key + "inds"])
                plan = M.plan_minibatch_joint([roidb_s[i] for i in inds[0]], [roidb_ws[i] for i in inds[1]], "Resnet_train",
                                              3, train, rng=rng)
            else:
                assert np.array_equal(inds, g[key + "inds"])
                plan = M.plan_minibatch([db[i] for i in inds], "Resnet_train", 3, train, kind == "ws", rng=rng)
            seen.append(tuple(g[key + "inds"]))
            assert np.array_equal(np.array(plan.im_scales, np.float64), g[key + "im_scales"])
            assert np.array_equal(np.array(plan.pre_shapes), g[key + "pre_shapes"])
            assert np.array_equal(np.array(plan.resize_shapes), g[key + "resize_shapes"])
            assert list(g[key + "blob_shape"]) == [len(plan.images)] + list(plan.blob_shape) + [3]
            for k in ("gt_boxes", "num_gt_boxes", "im_info"):
                got = getattr(plan, k)
                assert got.dtype == g[key + k].dtype and np.array_equal(got, g[key + k]), (key, k)
            assert all(im.angle is None for im in plan.images)
            assert all((im.crop is not None) == im.is_ws and (im.delta is not None) == train for im in plan.images)
        trailing = (rng or np.random).random_sample()
        assert trailing == g["%s_%d/trailing" % (kind, int(train))][0]
        assert len(set(seen)) > 1                                # (wrap / reshuffle happened inside the count)
    finally:
        np.random.set_state(state)


def test_plan_draws_with_rotation_on_match_the_oracle(cfg, monkeypatch):
    """The reference cannot run with rotation on here (no scikit-image): the plan must consume the stream as
    oracle.np_oracle.prep_im_for_blob does -- the trailing sample is equal -- and arrive at the same shapes."""
    from wssdl_bus_amd.roi_data_layer import minibatch_bus as M
    monkeypatch.setattr(cfg.TRAIN, "USE_ROTATION", True)
    monkeypatch.setattr(cfg.TRAIN, "SCALES", (48,))
    monkeypatch.setattr(cfg.TRAIN, "MAX_SIZE", 80)
    rs0 = np.random.RandomState(2)
    mk = lambda h, w, f: dict(plane=rs0.randint(0, 256, size=(h, w)).astype(np.uint8), flipped=f,       # noqa: E731
                              boxes=np.array([[1, 2, 9, 11]], np.uint16), gt_classes=np.array([2], np.int32), birads_diag=1)
    sup, weak = [mk(23, 31, True), mk(9, 300, False)], [mk(40, 57, False), mk(57, 40, True), mk(23, 31, False)]
    for train in (True, False):
        for seed in (1, 2, 3):
            rs1 = np.random.RandomState(seed)
            plan = M.plan_minibatch_joint(sup, weak, "Resnet_train", 3, train, rng=rs1)
            a = rs1.random_sample()
            rs2 = np.random.RandomState(seed)
            rs2.randint(0, high=len(cfg.TRAIN.SCALES), size=5)
            for e, im, ws in zip(sup + weak, plan.images, [False] * 2 + [True] * 3):
                _, scale, pre = O.prep_im_for_blob(e["plane"], e["flipped"], "Resnet_train", 48, 80, train, ws, rs2, nearest,
                                                   c=dict(USE_ROTATION=True))
                assert scale == im.im_scale and pre.shape[:2] == im.pre_shape
                assert (im.angle is not None) == ws and (im.crop is not None) == ws
                assert ((im.delta is not None), (im.factor is not None)) == (train, train)
            assert a == rs2.random_sample()
    # the switches gate the draws
    for name in ("USE_ROTATION", "USE_CROPPING", "USE_BRIGHTNESS_ADJUSTMENT", "USE_CONTRAST_ADJUSTMENT"):
        monkeypatch.setattr(cfg.TRAIN, name, False)
    rs1 = np.random.RandomState(4)
    plan = M.plan_minibatch_joint(sup, weak, "Resnet_train", 3, True, rng=rs1)
    rs2 = np.random.RandomState(4)
    rs2.randint(0, high=1, size=5)
    assert rs1.random_sample() == rs2.random_sample()
    assert all(im.angle is None and im.crop is None and im.delta is None and im.factor is None for im in plan.images)
    monkeypatch.setattr(cfg.TRAIN, "HAS_RPN", False)
    with pytest.raises(NotImplementedError):
        M.plan_minibatch(sup, "Resnet_train", 3, True, False)


XML = """<annotation>
   <folder>BUS</folder>
   <filename>%s.tif</filename>
   <size><width>%d</width><height>%d</height><depth>1</depth></size>
   <BIRADS><diag>%d</diag></BIRADS><segmented>0</segmented>
%s</annotation>
"""
OBJ = """   <object>
      <name>%s</name>
      <pose />
      <truncated>1</truncated>
      <difficult>%d</difficult>
      <bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox>
   </object>
"""


@pytest.fixture
def data_dir(tmp_path):
    from PIL import Image
    for d in ("Annotations", "TIFFImages", os.path.join("ImageSets", "Main")):
        os.makedirs(str(tmp_path / d))
    spec = {"FILE01": (40, 30, 0, [("benign", 0, 5, 3, 20, 12), ("__background__", 0, 2, 14, 33, 28)]),
            "FILE02": (36, 50, 1, [("  Malignant ", 0, 1, 1, 36, 50), ("benign", 1, 4, 4, 9, 9)])}
    rs = np.random.RandomState(0)
    for name, (w, h, diag, objs) in spec.items():
        (tmp_path / "Annotations" / (name + ".xml")).write_text(XML % (name, w, h, diag, "".join(OBJ % o for o in objs)))
        Image.fromarray(rs.randint(0, 256, size=(h, w)).astype(np.uint8)).save(str(tmp_path / "TIFFImages" / (name + ".tif")))
    (tmp_path / "ImageSets" / "Main" / "s_train.txt").write_text("FILE01\nFILE02 \n")
    return str(tmp_path)


def test_dataset_reader_and_training_roidb(cfg, monkeypatch, data_dir):
    from wssdl_bus_amd.datasets.bus import bus
    from wssdl_bus_amd.datasets.factory_bus import get_imdb, list_imdbs
    from wssdl_bus_amd.fast_rcnn import train_bus
    from wssdl_bus_amd.roi_data_layer.layer_bus import RoIDataLayer
    from wssdl_bus_amd.roi_data_layer.layer_bus_joint import RoIDataLayerJoint
    from wssdl_bus_amd.roi_data_layer.roidb import prepare_roidb
    d = bus("s_train", data_dir)
    assert d.name == "bus_s_train" and d.classes == ("__background__", "benign", "malignant") and d.num_classes == 3
    assert d.image_index == ["FILE01", "FILE02"] and d.num_images == 2
    assert d.image_path_at(1) == os.path.join(data_dir, "TIFFImages", "FILE02.tif")
    r = d.gt_roidb()
    assert r[0]["boxes"].dtype == np.uint16 and r[0]["boxes"].tolist() == [[4, 2, 19, 11], [1, 13, 32, 27]]
    assert r[0]["gt_classes"].dtype == np.int32 and r[0]["gt_classes"].tolist() == [1, 0] and r[0]["birads_diag"] == 1
    assert r[1]["boxes"].tolist() == [[0, 0, 35, 49]] and r[1]["gt_classes"].tolist() == [2] and r[1]["birads_diag"] == 2
    assert not r[0]["flipped"] and np.asarray(r[0]["gt_overlaps"]).tolist() == [[0, 1, 0], [1, 0, 0]]
    assert r[0]["seg_areas"].tolist() == [160.0, 480.0]
    # get_training_roidb: flipped entries appended, prepare_roidb's keys
    monkeypatch.setattr(cfg.TRAIN, "USE_FLIPPED", True)
    roidb = train_bus.get_training_roidb(d)
    assert len(roidb) == 4 and d.num_images == 4 and [e["flipped"] for e in roidb] == [False, False, True, True]
    assert roidb[2]["boxes"].tolist() == [[40 - 19 - 1, 2, 40 - 4 - 1, 11], [40 - 32 - 1, 13, 40 - 1 - 1, 27]]
    assert roidb[3]["boxes"].tolist() == [[0, 0, 35, 49]] and roidb[2]["birads_diag"] == 1 and roidb[3]["birads_diag"] == 2
    for i, e in enumerate(roidb):
        assert e["image"] == d.image_path_at(i) and (e["width"], e["height"]) == ((40, 30), (36, 50))[i % 2]
        assert e["max_classes"].tolist() == e["gt_classes"].tolist() and e["max_overlaps"].tolist() == [1.0] * len(e["gt_classes"])
    monkeypatch.setattr(cfg.TRAIN, "USE_FLIPPED", False)
    d2 = bus("s_train", data_dir)
    assert len(train_bus.get_training_roidb(d2)) == 2
    d3 = bus("s_train", data_dir)
    prepare_roidb(d3)
    assert sorted(d3.roidb[0]) == sorted(["boxes", "gt_classes", "gt_overlaps", "flipped", "seg_areas", "birads_diag", "image",
                                          "width", "height", "max_classes", "max_overlaps"])
    # the factory takes the reference's names under cfg.DATA_DIR
    monkeypatch.setattr(cfg, "DATA_DIR", data_dir)
    assert "bus_s_train" in list_imdbs() and "bus_test_normal" in list_imdbs() and len(list_imdbs()) == 20
    assert get_imdb("bus_s_train").image_index == ["FILE01", "FILE02"]
    with pytest.raises(KeyError):
        get_imdb("bus_nothing")
    with pytest.raises(IOError):
        get_imdb("bus_test")                    # no image-set file
    # get_data_layer's dispatch
    state = np.random.get_state()
    try:
        layer = train_bus.get_data_layer(roidb, "Resnet_train", 3, True, is_ws=True)
        assert isinstance(layer, RoIDataLayer) and layer._is_ws and layer._ims_per_batch == WS_IMS_PER_BATCH
        layer = train_bus.get_data_layer(roidb, "Resnet_train", 3, False)
        assert isinstance(layer, RoIDataLayer) and not layer._is_ws and layer._ims_per_batch == IMS_PER_BATCH
        assert layer._get_next_minibatch_inds().tolist() == [0, 1]
        layer = train_bus.get_data_layer((roidb, roidb[:2]), "Resnet_train", 3, True, is_joint=True)
        assert isinstance(layer, RoIDataLayerJoint) and len(layer._roidb_s) == 4 and len(layer._roidb_ws) == 2
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(cfg, "IS_MULTISCALE", True)
    with pytest.raises(NotImplementedError):
        train_bus.get_data_layer(roidb, "Resnet_train", 3, True)
    with pytest.raises(NotImplementedError):
        train_bus.get_training_roidb(bus("s_train", data_dir))
    # a plan from file-path entries equals the plan from decoded planes
    from wssdl_bus_amd.roi_data_layer import minibatch_bus as M
    from wssdl_bus_amd.utils.blob import imread
    a = M.plan_minibatch(roidb[:2], "Resnet_train", 3, True, False, rng=np.random.RandomState(1))
    b = M.plan_minibatch([dict(e, plane=imread(e["image"])) for e in roidb[:2]], "Resnet_train", 3, True, False,
                         rng=np.random.RandomState(1))
    assert np.array_equal(a.gt_boxes, b.gt_boxes) and np.array_equal(a.im_info, b.im_info) and a.resize_shapes == b.resize_shapes
