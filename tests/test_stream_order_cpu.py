"""The parts of the stream-order work that need no GPU: the shared case table's count, the SYNCS table against the
package's docstrings, and the pure-Python parts of tests/stream_order.py (decoy rule, vacuity floor, uncovered share)."""
import os

import numpy as np
import pytest
import torch

import guarded_alloc as ga
import stream_order as so


def test_case_table_count():
    import device_op_cases as D
    assert D.N_MEMORY_CONTRACT_CASES == 407
    assert D.N_STREAM_ORDER_ADDED == 17 and len(D.CASES) == 424
    added = list(D.CASES)[407:]
    for prefix, n in (("bbox-overlaps-ui-", 3), ("bbox-overlaps-", 6), ("shifted-anchors-", 2), ("roi-targets-", 3),
                      ("mil-loss-", 1), ("roi-pool-bwd-i32-no-workspace", 1), ("roi-candidates-", 2), ("loss-libm-probe-", 2)):
        assert sum(a.startswith(prefix) for a in added) == n, prefix
    for shape in ("1x1", "70x3", "257x20"):
        assert "bbox-overlaps-" + shape in D.CASES and "bbox-overlaps-ui-" + shape in D.CASES
    assert "shifted-anchors-1x1" in D.CASES and "shifted-anchors-14x17" in D.CASES


def test_syncs_table_is_backed_by_the_wrappers():
    """every listed prefix names a case and quotes a sentence that stands, verbatim, in a docstring of the package"""
    import device_op_cases as D
    import test_gpu_stream_order as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    texts = []
    for top, _dirs, files in os.walk(os.path.join(root, "wssdl_bus_amd")):
        texts += [open(os.path.join(top, f)).read() for f in files if f.endswith(".py")]
    flat = [" ".join(t.replace("*", " ").replace("#", " ").split()) for t in texts]
    for prefixes, sentence in T.SYNCS:
        assert all(any(n.startswith(p) for n in D.CASES) for p in prefixes), prefixes
        assert len(sentence.split()) >= 4, sentence
        assert any(" ".join(sentence.split()) in t for t in flat), (prefixes, sentence)
    for table in (T.SYNCS, T.DECOYS, T.VACUOUS_OK):
        for name in D.CASES:
            assert sum(name.startswith(row[0]) for row in table) <= 1, name
    assert all(isinstance(row[-1], str) and len(row[-1].split()) >= 4 for row in T.VACUOUS_OK + T.DECOYS)
    n_free = sum(T.sync_free(n) for n in D.CASES)
    n_vac = sum(T._lookup(T.VACUOUS_OK, n) is not None for n in D.CASES)
    print("stream-order tables: %d cases, %d sync-free, %d with the vacuity floor waived" % (len(D.CASES), n_free, n_vac))
    assert n_free >= len(D.CASES) // 2, "most of the table has to stay under the harness's full view"


def test_default_decoy_halves_floats_and_keeps_the_rest():
    x = torch.tensor([[4.0, -3.0], [0.0, 1e-3]], dtype=torch.float32)
    cl = torch.randn(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    inputs = {"x": x, "d": x.double(), "i": torch.tensor([3, -1], dtype=torch.int32), "b": torch.tensor([True, False]),
              "u": torch.tensor([255, 7], dtype=torch.uint8), "l": torch.tensor([5], dtype=torch.int64), "cl": cl, "n": 7}
    d = so.default_decoy(inputs)
    assert sorted(d, key=str) == sorted(inputs, key=str) and d["n"] == 7
    assert torch.equal(d["x"], x * 0.5) and d["x"].dtype == torch.float32
    assert torch.equal(d["d"], x.double() * 0.5) and d["d"].dtype == torch.float64
    for k in ("i", "b", "u", "l"):
        assert torch.equal(d[k], inputs[k]) and d[k].dtype == inputs[k].dtype and d[k].data_ptr() != inputs[k].data_ptr()
    assert d["cl"].stride() == cl.stride()
    assert torch.equal(inputs["x"], torch.tensor([[4.0, -3.0], [0.0, 1e-3]]))          # the inputs are untouched
    # boxes stay ordered, sorted lists stay sorted, values only shrink towards zero
    boxes = torch.tensor([[0.0, 2.0, 10.0, 30.0, 40.0], [1.0, 5.0, 5.0, 5.0, 6.0]])
    h = so.default_decoy([boxes])[0]
    assert bool((h[:, 3] >= h[:, 1]).all()) and bool((h[:, 4] >= h[:, 2]).all()) and bool((h.abs() <= boxes.abs()).all())
    assert bool((h[1:, 0] >= h[:-1, 0]).all())
    # a sequence stays a sequence
    assert isinstance(so.default_decoy([x, 3]), list) and so.default_decoy([x, 3])[1] == 3


def test_reversed_rows_decoy():
    dets = torch.arange(15.0).reshape(3, 5)
    d = so.reversed_rows("dets")({"dets": dets, "other": torch.tensor([1.0, 2.0])})
    assert torch.equal(d["dets"], dets.flip(0)) and d["dets"].is_contiguous() and torch.equal(d["other"], torch.tensor([1.0, 2.0]))


def test_vacuity_floor():
    flat = lambda r: ga._flatten(r, "result", [])                                    # noqa: E731
    base = (torch.tensor([1.0, 2.0]), [np.array([3, 4]), 5])
    so.check_vacuity("c", flat(base), flat((torch.tensor([1.0, 2.5]), [np.array([3, 4]), 5])), False)
    so.check_vacuity("c", flat(base), flat((torch.tensor([1.0, 2.0]), [np.array([3, 4]), 6])), False)
    with pytest.raises(so.VacuousDecoy, match="decoy tests nothing"):
        so.check_vacuity("c", flat(base), flat((torch.tensor([1.0, 2.0]), [np.array([3, 4]), 5])), False)
    with pytest.raises(so.VacuousDecoy, match="decoy tests nothing"):                 # a flag: no specified input
        so.check_vacuity("c", flat(base), flat((torch.tensor([9.0, 2.0]), [np.array([3, 4]), 5])), True)
    # only the defined part counts: a difference in a region that was cut away does not make a decoy
    cut = lambda r: (r[0], None)                                                      # noqa: E731
    with pytest.raises(so.VacuousDecoy):
        so.check_vacuity("c", flat(cut(base)), flat(cut((torch.tensor([1.0, 2.0]), [np.array([0, 0]), 0]))), False)


def test_uncovered_share_arithmetic():
    rec = lambda d, h, f: dict(delay_ms=d, host_ms=h, sync_free=f)                    # noqa: E731
    assert not so.is_uncovered(rec(5.2, 0.4, True))
    assert so.is_uncovered(rec(5.2, 6.0, True))
    assert not so.is_uncovered(rec(5.2, 6.0, False))                                  # a synchronising case is not counted
    assert not so.is_uncovered(rec(5.0, 5.0, True))                                   # shorter, not equal
    recorded = [rec(5.1, 0.3, True)] * 97 + [rec(5.1, 7.9, True)] * 2 + [rec(5.1, 40.0, False)] * 20
    assert so.uncovered_share(recorded) == (2, 99, 2.0 / 99.0)
    with pytest.raises(AssertionError, match="2 of 99"):
        so.assert_uncovered_share(recorded)                                           # 2.02 % > 2 %
    assert so.assert_uncovered_share(recorded + [rec(5.1, 0.3, True)]) == (2, 100, 0.02)   # exactly 2 % passes
    with pytest.raises(AssertionError, match="no sync-free case"):
        so.assert_uncovered_share([rec(5.1, 40.0, False)])
    assert so.uncovered_share([]) == (0, 0, 0.0)
    assert so.delay_ms_for(0.2) == 5.0 and so.delay_ms_for(10.0) == 30.0
