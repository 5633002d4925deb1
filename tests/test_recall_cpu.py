"""CPU: proposal recall (datasets/recall.py, bus.evaluate_recall) against the reference's own imdb.evaluate_recall,
recorded in tests/golden/proposal_recall.npz by tests/golden/make_golden_recall.py.  Every comparison is bit for bit:
integers equal, f64 values with array_equal."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from recall_cases import cases, roidb_of, tie_census  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return load_golden("proposal_recall")


def key(name, area, limit, what):
    return "%s/%s/%s/%s" % (name, area, "none" if limit is None else limit, what)


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def assert_cell_is_golden(gold, name, area, limit, cell):
    for what in ("ar", "recalls", "thresholds", "gt_overlaps"):
        assert same(cell[what], gold[key(name, area, limit, what)]), (name, area, limit, what)


def test_area_ranges_are_the_references(gold):
    from wssdl_bus_amd.datasets import recall
    names = [str(n) for n in gold["area_names"]]
    assert list(recall.ALL_EIGHT) == names and [recall.AREAS[n] for n in names] == list(range(8))
    assert np.array_equal(np.asarray(recall.AREA_RANGES, np.float64), gold["area_ranges"])


def test_cases_are_the_stored_inputs(gold):
    for name, case in cases().items():
        assert np.array_equal(np.concatenate(case["gt_boxes"], 0), gold[name + "/gt_boxes"])
        assert np.array_equal(np.concatenate(case["candidates"], 0), gold[name + "/boxes"])
        assert np.array_equal(np.cumsum([0] + [len(c) for c in case["candidates"]]), gold[name + "/box_offsets"])
        assert np.array_equal(np.cumsum([0] + [len(g) for g in case["gt_boxes"]]), gold[name + "/gt_offsets"])
        assert [str(a) for a in gold[name + "/areas"]] == list(case["areas"])
        assert gold[name + "/limits"].tolist() == [0 if l is None else l for l in case["limits"]]


@pytest.mark.parametrize("name", [n for n, c in cases().items() if not c["raises"]])
def test_host_path_equals_the_reference(gold, name):
    from wssdl_bus_amd.datasets import recall
    case = cases()[name]
    gt = recall.pack_recall_gt(roidb_of(case))
    table = recall.evaluate_recall_host(case["candidates"], gt, case["areas"], case["limits"], return_matches=True)
    assert len(table) == len(case["areas"]) * len(case["limits"])
    for (area, limit), cell in table.items():
        assert_cell_is_golden(gold, name, area, limit, cell)
        m = cell["matches"]
        assert np.array_equal(np.sort(m["overlap"]), cell["gt_overlaps"]) and len(m["gt"]) == len(m["box"]) == len(m["image"])
        lo, hi = recall.AREA_RANGES[recall.AREAS[area]]
        assert cell["num_pos"] == int(((gt["areas"] >= lo) & (gt["areas"] <= hi)).sum())


def test_hand_made_matches():
    """The rounds themselves, (gt, box, overlap) in round order."""
    from wssdl_bus_amd.datasets import recall
    c = cases()

    def rows(name):
        m = recall.evaluate_recall_host(c[name]["candidates"], roidb_of(c[name]), ("all",), return_matches=True)[("all", None)]["matches"]
        return list(zip(m["gt"].tolist(), m["box"].tolist(), m["overlap"].tolist()))
    assert rows("tie_box") == [(0, 0, 0.5)]
    assert rows("tie_gt") == [(0, 1, 0.5), (1, 0, 0.5)]
    assert rows("shared_best") == [(1, 0, 110.0 / 120.0), (0, 1, 100.0 / 150.0)]
    assert rows("zero_overlap") == [(1, 0, 1.0), (0, 1, 0.0)]


def test_random_set_holds_every_tie_class():
    from wssdl_bus_amd.datasets import recall
    census = tie_census(cases()["random200"], recall.overlaps_host, recall.AREA_RANGES, recall.AREAS)
    assert all(v > 0 for v in census.values()), census


def test_fewer_boxes_than_gts_raises(gold):
    from wssdl_bus_amd.datasets import recall
    case = cases()["too_few"]
    assert bool(gold[key("too_few", "all", None, "raises")])
    with pytest.raises(AssertionError, match="image 0"):
        recall.evaluate_recall_host(case["candidates"], roidb_of(case), case["areas"], case["limits"])


def test_flipped_entries_raise_key_error():
    from wssdl_bus_amd.datasets import recall
    roidb = roidb_of(cases()["tie_gt"])
    twin = {k: v for k, v in roidb[0].items() if k != "seg_areas"}
    twin["flipped"] = True
    with pytest.raises(KeyError, match="seg_areas"):
        recall.pack_recall_gt(roidb + [twin])


def test_unknown_area_is_the_references_assertion():
    from wssdl_bus_amd.datasets import recall
    case = cases()["tie_box"]
    with pytest.raises(AssertionError, match="unknown area range: huge"):
        recall.evaluate_recall_host(case["candidates"], roidb_of(case), ("huge",))


XML = "<annotation><BIRADS><diag>%d</diag></BIRADS>%s</annotation>"
OBJ = ("<object><name>%s</name><difficult>0</difficult><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax>"
       "<ymax>%d</ymax></bndbox></object>")


def write_dataset(root, gt_boxes, background=None):
    """A BUS data set whose image i holds gt_boxes[i] as 'benign' objects and background[i] as '__background__'
    objects (class 0: the rows evaluate_recall(candidate_boxes=None) evaluates)."""
    from PIL import Image
    for d in ("Annotations", "TIFFImages", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(root, d))
    names = ["IM%02d" % i for i in range(len(gt_boxes))]
    for i, name in enumerate(names):
        objs = [("benign",) + tuple(int(v) + 1 for v in b) for b in gt_boxes[i]]
        objs += [("__background__",) + tuple(int(v) + 1 for v in b) for b in (background[i] if background else [])]
        with open(os.path.join(root, "Annotations", name + ".xml"), "w") as f:
            f.write(XML % (0, "".join(OBJ % o for o in objs)))
        Image.fromarray(np.zeros((8, 8), np.uint8)).save(os.path.join(root, "TIFFImages", name + ".tif"))
    with open(os.path.join(root, "ImageSets", "Main", "s_test.txt"), "w") as f:
        f.write("".join(n + "\n" for n in names))
    return root


def test_bus_evaluate_recall(gold, tmp_path):
    from wssdl_bus_amd.datasets.bus import bus
    # candidate boxes given: the case `mixed`, every stored cell
    case = cases()["mixed"]
    d = bus("s_test", write_dataset(str(tmp_path / "mixed"), case["gt_boxes"]))
    for area in case["areas"]:
        for limit in case["limits"]:
            with np.errstate(all="ignore"):
                r = d.evaluate_recall(candidate_boxes=case["candidates"], area=area, limit=limit)
            assert sorted(r) == ["ar", "gt_overlaps", "recalls", "thresholds"]
            assert_cell_is_golden(gold, "mixed", area, limit, r)
    # candidate_boxes=None: the roidb's gt_classes == 0 rows (the integer boxes of `tie_box`)
    case = cases()["tie_box"]
    d = bus("s_test", write_dataset(str(tmp_path / "tie"), case["gt_boxes"], case["candidates"]))
    assert_cell_is_golden(gold, "tie_box", "all", None, d.evaluate_recall())
    thr = np.array([0.25, 0.5, 0.75])
    r = d.evaluate_recall(thresholds=thr)
    assert r["thresholds"] is thr and r["recalls"].tolist() == [1.0, 1.0, 0.0] and r["ar"] == r["recalls"].mean()
    with pytest.raises(AssertionError, match="unknown area range: huge"):
        d.evaluate_recall(area="huge")
    # fewer boxes than gts
    case = cases()["too_few"]
    d = bus("s_test", write_dataset(str(tmp_path / "few"), case["gt_boxes"]))
    with pytest.raises(AssertionError):
        d.evaluate_recall(candidate_boxes=case["candidates"])
    # a flipped roidb has no seg_areas
    d = bus("s_test", write_dataset(str(tmp_path / "flip"), [[[0, 0, 3, 3]]]))
    d.append_flipped_images()
    with pytest.raises(KeyError, match="seg_areas"):
        d.evaluate_recall()
