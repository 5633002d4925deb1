#!/usr/bin/env python3
"""Generate tests/golden/proposal_recall.npz: the reference's own imdb.evaluate_recall (datasets/imdb.py:125-213) on
the cases of tests/recall_cases.py.

Run in the build container only:  python tests/golden/make_golden_recall.py
datasets/imdb.py is Python 2: it is copied to a temporary directory OUTSIDE the repository, converted there by
lib2to3 (print statements, xrange, and the has_key fixer for line 149) and imported from there, next to the scratch
tree of oracle/ref_python_stage.py, which supplies fast_rcnn.config and utils.cython_bbox (built from the
reference's .pyx into oracle/_ref) and the np.float alias.  A subclass of imdb with a hand-set roidb is evaluated for
every (area, limit) cell of every case.  Data only goes into the .npz: the inputs and the values the reference
returned, plus the bounds of its area ranges, read from the method's source as numbers.  Re-running reproduces the
file.
"""
import ast
import importlib.util
import io
import os
import shutil
import sys
import tempfile
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("WSSDL_REFERENCE", "/root/reference")
REF_MODULE = os.path.join(REFERENCE, "code", "lib", "datasets", "imdb.py")
OUT = os.path.join(HERE, "proposal_recall.npz")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def available():
    return os.path.exists(REF_MODULE)


def stage_reference(tmp):
    """The reference's module, converted to Python 3 in `tmp` and imported from there."""
    from lib2to3.main import main as lib2to3_main
    from oracle import ref_python_stage
    ref_python_stage.stage()
    dst = os.path.join(tmp, "ref_imdb.py")
    shutil.copyfile(REF_MODULE, dst)
    saved = sys.stdout, sys.stderr
    try:
        with open(os.devnull, "w") as null:
            sys.stdout = sys.stderr = null
            rc = lib2to3_main("lib2to3.fixes", ["-w", "-n", dst])
    finally:
        sys.stdout, sys.stderr = saved
    assert rc == 0
    spec = importlib.util.spec_from_file_location("ref_imdb", dst)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, dst


def reference_area_table(path):
    """The numbers of evaluate_recall's `areas` and `area_ranges` literals."""
    tree = ast.parse(open(path).read())
    found = {}
    for fn in ast.walk(tree):
        if isinstance(fn, ast.FunctionDef) and fn.name == "evaluate_recall":
            for node in ast.walk(fn):
                if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and node.targets[0].id in ("areas", "area_ranges"):
                    found[node.targets[0].id] = eval(compile(ast.Expression(node.value), path, "eval"), {})
    names = sorted(found["areas"], key=found["areas"].get)
    assert [found["areas"][n] for n in names] == list(range(len(names)))
    return names, np.asarray(found["area_ranges"], np.float64)


def make_imdb(mod, case):
    import scipy.sparse
    from recall_cases import roidb_of

    class hand_set(mod.imdb):
        def __init__(self, roidb):
            with redirect_stdout(io.StringIO()):
                mod.imdb.__init__(self, "recall_case")
            self._classes = ("__background__", "benign", "malignant")
            self._image_index = list(range(len(roidb)))
            self._roidb = roidb

    roidb = roidb_of(case)
    for e in roidb:
        e["gt_overlaps"] = scipy.sparse.csr_matrix(e["gt_overlaps"])
    return hand_set(roidb)


def key(name, area, limit, what):
    return "%s/%s/%s/%s" % (name, area, "none" if limit is None else limit, what)


def generate():
    """{name: array} of the committed file."""
    from recall_cases import cases
    tmp = tempfile.mkdtemp(prefix="wssdl_golden_recall_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        mod, path = stage_reference(tmp)
        names, ranges = reference_area_table(path)
        out = {"area_names": np.array(names), "area_ranges": ranges}
        for name, case in cases().items():
            db = make_imdb(mod, case)
            n = len(case["candidates"])
            out[name + "/gt_boxes"] = np.concatenate(case["gt_boxes"], 0)
            out[name + "/gt_offsets"] = np.cumsum([0] + [len(g) for g in case["gt_boxes"]]).astype(np.int32)
            out[name + "/boxes"] = np.concatenate(case["candidates"], 0)
            out[name + "/box_offsets"] = np.cumsum([0] + [len(c) for c in case["candidates"]]).astype(np.int32)
            out[name + "/areas"] = np.array(case["areas"])
            out[name + "/limits"] = np.array([0 if l is None else l for l in case["limits"]], np.int32)
            for area in case["areas"]:
                for limit in case["limits"]:
                    if case["raises"]:
                        try:
                            db.evaluate_recall(candidate_boxes=case["candidates"], area=area, limit=limit)
                        except AssertionError:
                            out[key(name, area, limit, "raises")] = np.array(True)
                            continue
                        raise RuntimeError("the reference did not raise on case %s" % name)
                    with np.errstate(all="ignore"):
                        r = db.evaluate_recall(candidate_boxes=case["candidates"], area=area, limit=limit)
                    assert len(case["candidates"]) == n
                    for what in ("ar", "recalls", "thresholds", "gt_overlaps"):
                        out[key(name, area, limit, what)] = np.asarray(r[what], np.float64)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if not available():
        sys.exit("the reference is not on this machine: %s" % REF_MODULE)
    np.savez_compressed(OUT, **generate())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
