"""Position classes of the per-RoI head's 3x3 convolutions (networks/_plumbing.py: TapPlan) against a
brute-force enumeration of the valid (output position, tap) pairs.  CPU only: no kernels run."""
import itertools

import numpy as np
import pytest

from wssdl_bus_amd.networks import _plumbing
from wssdl_bus_amd.networks.backbones import _same_pad

SHAPES = [(7, 7, 2), (4, 4, 1), (5, 6, 1), (6, 6, 2), (3, 3, 1), (1, 1, 1), (2, 5, 2), (8, 8, 1)]


def _valid_pairs(h, w, s):
    pt, pl = _same_pad(h, 3, s)[0], _same_pad(w, 3, s)[0]
    oh, ow = -(-h // s), -(-w // s)
    return {((oy, ox), ky * 3 + kx)
            for oy, ox, ky, kx in itertools.product(range(oh), range(ow), range(3), range(3))
            if 0 <= oy * s + ky - pt < h and 0 <= ox * s + kx - pl < w}


@pytest.mark.parametrize("h,w,s", SHAPES)
def test_classes_cover_exactly_the_valid_pairs(h, w, s):
    p = _plumbing.TapPlan(h, w, s)
    got = [(pos, t) for taps, poss in p.classes for pos in poss for t in taps]
    assert len(got) == len(set(got))
    assert set(got) == _valid_pairs(h, w, s)
    # every output position in exactly one class, slots in class order
    assert sorted(p.slots) == sorted(itertools.product(range(p.oh), range(p.ow)))
    assert p.slots == [pos for _, poss in p.classes for pos in poss]
    assert p.units == len(got) and p.wunits == sum(len(t) for t, _ in p.classes)
    # classes ordered centre | edges | corners (taps, then positions, descending); groups = equal shapes
    keys = [(len(t), len(q)) for t, q in p.classes]
    assert keys == sorted(keys, reverse=True)
    assert sum(g[1] for g in p.groups) == len(p.classes)
    for k0, n, npos, ntaps in p.groups:
        assert all(keys[k] == (ntaps, npos) for k in range(k0, k0 + n))


def test_head_shapes_have_nine_classes_in_three_groups():
    for h, s in ((7, 2), (4, 1)):
        p = _plumbing.TapPlan(h, h, s)
        assert p.ok and (p.oh, p.ow) == (4, 4)
        assert [(n, npos, ntaps) for _, n, npos, ntaps in p.groups] == [(1, 4, 9), (4, 2, 6), (4, 1, 4)]
        assert p.units == 100                      # of 16 * 9 = 144 dense (position, tap) pairs
    assert _plumbing.TapPlan(7, 7, 2).slots == _plumbing.TapPlan(4, 4, 1).slots


@pytest.mark.parametrize("h,w,s", SHAPES)
def test_device_table_matches_plan(h, w, s):
    p = _plumbing.TapPlan(h, w, s)
    if not p.ok:
        return
    T = p.table
    assert T.dtype == np.int32 and T.shape == (_plumbing._TAB_INTS,)
    assert list(T[:10]) == [len(p.classes), h, w, p.oh, p.ow, s, p.pt, p.pl, p.units, p.wunits]
    for k, (taps, poss) in enumerate(p.classes):
        b = _plumbing._TAB_CLS + _plumbing._CLS_STRIDE * k
        assert list(T[b:b + 5]) == [len(poss), len(taps), p.slot_base[k], p.cum[k], p.wcum[k]]
        assert list(T[b + 6:b + 6 + len(taps)]) == taps
        for t in range(9):
            assert T[b + 15 + t] == (taps.index(t) if t in taps else -1)
    for sl, (y, x) in enumerate(p.slots):
        assert T[_plumbing._TAB_SLOTPOS + sl] == y * p.ow + x
        assert T[_plumbing._TAB_POSSLOT + y * p.ow + x] == sl
        k = T[_plumbing._TAB_SLOTCLS + sl]
        assert (y, x) in p.classes[k][1]


def test_dense_switch_and_cpu_tensors_keep_the_dense_route(monkeypatch):
    import torch
    x = torch.zeros((2, 7, 7, 8))
    assert not _plumbing.taps_usable(x)                    # CPU tensor
    assert _plumbing.TAPS_MIN_ROIS <= 8512                 # the default workload's head takes the new route
    monkeypatch.setenv("WSSDL_HEAD_DENSE_3X3", "1")
    assert not _plumbing.taps_usable(x)
