"""The reference optimisers and schedules of wssdl_bus_amd/fast_rcnn/optim.py without a GPU: the per-parameter chain of
torch ops (what CPU tensors and WSSDL_TORCH_OPTIM=1 take) against the f64 statement and the counted bounds of
tests/optim_reference.py, the schedules against hand-worked sequences, and the solver's wiring.  The one-launch HIP
kernel is held to the same reference in test_gpu_optim.py."""
import math

import numpy as np
import pytest
import torch

import optim_reference as R
from wssdl_bus_amd.fast_rcnn import optim as O
from wssdl_bus_amd.fast_rcnn.config import cfg
from wssdl_bus_amd.fast_rcnn.train_bus import SolverWrapper
from wssdl_bus_amd.networks import _plumbing as P

KINDS = ("adam", "amsgrad", "sgd")
LR = 5e-4


def _params(seed=0):
    """numel 1, 3, a matrix, a channels_last weight; the last one never gets a gradient"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g) * 0.05
    ps = [rn(1), rn(3), rn(5, 7), rn(4, 3, 3, 3).contiguous(memory_format=torch.channels_last), rn(6)]
    return [p.requires_grad_() for p in ps]


def _inject_state(opt, seed=1):
    """a state that is not all zero: m of mixed signs, v >= 0, vhat above v at some elements and below at others"""
    g = torch.Generator().manual_seed(seed)
    sd = opt.state_dict()
    for i, slots in sd["state"].items():
        for name, view in slots.items():
            r = torch.randn(view.shape, generator=g)
            if name in ("m", "accum"):
                view.copy_(r * 0.02)
            elif name == "v":
                view.copy_(r * r * 1e-3)
            else:
                view.copy_(slots["v"] * (1.0 + 0.5 * torch.sign(r)))
    opt.load_state_dict(sd)


def _set_grads(params, seed, skip_last=True):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        if skip_last and i == len(params) - 1:
            p.grad = None
        elif i == 2:
            p.grad = (torch.randn(p.shape[::-1], generator=g) * 0.01).t()      # strides differ from the parameter's
        else:
            p.grad = torch.randn(p.shape, generator=g).mul_(0.01).contiguous(memory_format=torch.contiguous_format)


_np, _snapshot = R.to_numpy, R.snapshot


@pytest.mark.parametrize("kind", KINDS)
def test_torch_form_inside_the_counted_bounds(kind):
    params = _params()
    opt = O.ReferenceOptimizer(params, kind, LR, momentum=0.9)
    assert not O.hip_usable(params)
    _inject_state(opt)
    worst = 0.0
    for t in (1, 2, 3):
        _set_grads(params, 10 + t)
        before = _snapshot(opt)                 # the f64 state is re-seeded from the f32 state: bounds stay per step
        opt.step()
        worst = max(worst, R.check_step(opt, before, t, LR, 0.9, what="cpu"))
        opt.zero_grad()
        assert all(p.grad is None for p in params)
    assert opt.t == 3
    print("%s torch-op form on the CPU: worst error / bound %.3f" % (kind, worst))


def test_nesterov_torch_form_equals_f32_numpy_bit_for_bit():
    params = _params()
    opt = O.ReferenceOptimizer(params, "sgd", LR, momentum=0.9)
    _inject_state(opt)
    for t in (1, 2, 3):
        _set_grads(params, 20 + t)
        before = _snapshot(opt)
        opt.step()
        for i, (p, b) in enumerate(zip(params, before)):
            if b["g"] is None:
                continue
            want_p, want_acc = R.nesterov_f32(b["p"], b["g"], b["accum"], LR, 0.9)
            assert np.array_equal(_np(p), want_p) and np.array_equal(_np(opt.views["accum"][i]), want_acc), (t, i)


@pytest.mark.parametrize("kind", KINDS)
def test_parameter_without_gradient_is_untouched_state_included(kind):
    params = _params()
    opt = O.ReferenceOptimizer(params, kind, LR)
    _inject_state(opt)
    _set_grads(params, 5)
    before = _snapshot(opt)
    opt.step()
    assert before[-1]["g"] is None
    assert np.array_equal(_np(params[-1]), before[-1]["p"])
    for s, v in opt.views.items():
        assert np.array_equal(_np(v[-1]), before[-1][s]) and np.abs(before[-1][s]).max() > 0
    assert not np.array_equal(_np(params[0]), before[0]["p"])


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_round_trip_continues_identically(kind):
    a_params, b_params = _params(), _params()
    a = O.ReferenceOptimizer(a_params, kind, LR)
    for t in (1, 2):
        _set_grads(a_params, 30 + t)
        a.step()
    sd = a.state_dict()
    assert sd["step"] == 2 and sorted(sd["state"][0]) == sorted(O.SLOTS[kind])
    assert sd["state"][3]["m" if kind != "sgd" else "accum"].stride() == a_params[3].stride()
    b = O.ReferenceOptimizer(b_params, kind, 123.0)
    with torch.no_grad():
        for p, q in zip(b_params, a_params):
            p.copy_(q)
    b.load_state_dict(sd)
    assert b.t == 2 and b.param_groups[0]["lr"] == LR
    for t in (3, 4):
        _set_grads(a_params, 30 + t, skip_last=False)
        _set_grads(b_params, 30 + t, skip_last=False)
        a.step()
        b.step()
    for p, q in zip(a_params, b_params):
        assert torch.equal(p, q)
    for s in O.SLOTS[kind]:
        for x, y in zip(a.views[s], b.views[s]):
            assert torch.equal(x, y)
    with pytest.raises(ValueError):
        O.ReferenceOptimizer(b_params, "sgd" if kind != "sgd" else "adam", LR).load_state_dict(sd)


def test_state_is_flat_and_every_parameter_starts_on_a_float4():
    params = _params()
    opt = O.ReferenceOptimizer(params, "amsgrad", LR)
    assert opt.offsets == [0, 4, 8, 44, 152] and all(o % O.ALIGN == 0 for o in opt.offsets)
    for s in ("m", "v", "vhat"):
        assert opt.buffers[s].numel() == 160
        for v, off in zip(opt.views[s], opt.offsets):
            assert v.data_ptr() == opt.buffers[s].data_ptr() + 4 * off
    t = O._Table([torch.zeros(3), torch.zeros(2 * O.CHUNK + 5).view(-1, 1), torch.zeros(1)], [0, 4, 2 * O.CHUNK + 12])
    assert t.chunks.tolist() == [[0, 0, 3, 0], [1, 0, O.CHUNK, 4], [1, O.CHUNK, O.CHUNK, 4 + O.CHUNK],
                                 [1, 2 * O.CHUNK, 5, 4 + 2 * O.CHUNK], [2, 0, 1, 2 * O.CHUNK + 12]]
    assert "WSSDL_TORCH_OPTIM" in P.SWITCHES


# ---------------------------------------------------------------- schedules

def test_piecewise_constant_schedule_hand_worked():
    # max_iters = 10: the boundary is int(7.5) = 7; TF's piecewise_constant keeps the first value while
    # global_step <= 7, so the steps that start from global_step 0..7 run at lr and those from 8, 9 at 0.1 * lr
    want = [LR] * 8 + [LR * 0.1] * 2
    assert [O.piecewise_lr(LR, s, 10) for s in range(10)] == want
    assert [R.piecewise_lr(LR, s, 10) for s in range(10)] == want


# 12 validation losses, patience 2, epsilon 1e-3, factor 0.5, min_lr 0.3, from lr 1.0; worked by hand:
#   loss    event                                                          best  wait  lr
#   1.0     first loss: new best                                           1.0   0     1.0
#   1.0     no improvement; wait 0 < 2                                     1.0   1     1.0
#   0.9995  better by 5e-4 only (< epsilon): no improvement; wait 1 < 2    1.0   2     1.0
#   1.2     wait 2 >= 2: REDUCED to 0.5, wait cleared, then counted        1.0   1     0.5
#   1.1     wait 1 < 2                                                     1.0   2     0.5
#   0.8     new best                                                       0.8   0     0.5
#   0.8     wait 0 < 2                                                     0.8   1     0.5
#   0.9     wait 1 < 2                                                     0.8   2     0.5
#   0.85    wait 2 >= 2: 0.25 is under the floor: REDUCED to min_lr 0.3    0.8   1     0.3
#   0.81    wait 1 < 2                                                     0.8   2     0.3
#   0.8     wait 2 >= 2 but the rate is not above min_lr: nothing          0.8   3     0.3
#   0.8     the same; wait keeps growing                                   0.8   4     0.3
ROP_LOSSES = [1.0, 1.0, 0.9995, 1.2, 1.1, 0.8, 0.8, 0.9, 0.85, 0.81, 0.8, 0.8]
ROP_LRS = [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.3, 0.3, 0.3, 0.3]
ROP_WAIT = [0, 1, 2, 1, 2, 0, 1, 2, 1, 2, 3, 4]
ROP_BEST = [1.0, 1.0, 1.0, 1.0, 1.0, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8]


def test_reduce_lr_on_plateau_hand_worked():
    h = O.ReduceLROnPlateau(1.0, factor=0.5, patience=2, mode="min", epsilon=1e-3, cooldown=0, min_lr=0.3)
    lrs, waits, bests = [], [], []
    for x in ROP_LOSSES:
        h.on_val_end(x)
        lrs.append(h.get_cur_lr()), waits.append(h.wait), bests.append(h.best)
    assert lrs == ROP_LRS and waits == ROP_WAIT and bests == ROP_BEST
    assert R.plateau_lrs(ROP_LOSSES, 1.0, 0.5, 2, 1e-3, 0.3) == ROP_LRS
    # the reference's calling convention: the list of every loss so far
    h2 = O.ReduceLROnPlateau(1.0, patience=2, epsilon=1e-3, min_lr=0.3)
    for i in range(len(ROP_LOSSES)):
        h2.on_val_end(ROP_LOSSES[:i + 1])
    assert h2.get_cur_lr() == 0.3 and h2.wait == 4
    with pytest.raises(ValueError):
        O.ReduceLROnPlateau(1.0, factor=1.0)


def test_reduce_lr_on_plateau_reference_settings_first_reduction_at_the_seventh_loss():
    # patience 5 (train_bus.py:281): losses that never improve after the first; wait reaches 5 at the sixth loss,
    # the seventh reduces; wait is 1 right after, so the next reduction is five losses later, at the twelfth
    h = O.ReduceLROnPlateau(LR, factor=0.5, patience=5, mode="min", epsilon=1e-3, cooldown=0, min_lr=0)
    lrs = []
    for _ in range(12):
        h.on_val_end(2.0)
        lrs.append(h.get_cur_lr())
    assert lrs == [LR] * 6 + [LR * 0.5] * 5 + [LR * 0.25]


# ---------------------------------------------------------------- the solver's wiring

class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(3, 2)


class _Solver(SolverWrapper):
    """the two backward halves replaced by something a CPU can do; records the global step each half saw"""

    def __init__(self, *a, **k):
        super().__init__(_Net(), *a, **k)
        self.seen = []

    def _fake(self, _blobs=None):
        self.seen.append(self.global_step)
        loss = (self.net.fc.weight ** 2).sum() + self.net.fc.bias.sum()
        loss.backward()
        return {"loss": loss} if _blobs == "s" else loss

    supervised_backward = weak_backward = _fake


def test_unknown_opt_or_schedule_raises():
    for bad in ("Adam", "rmsprop", "", 0):
        with pytest.raises(ValueError):
            SolverWrapper(_Net(), opt=bad)
    with pytest.raises(ValueError):
        SolverWrapper(_Net(), lr_scheduling="cosine")
    with pytest.raises(ValueError):
        SolverWrapper(_Net(), lr_scheduling="pc")               # needs max_iters
    with pytest.raises(ValueError):
        O.ReferenceOptimizer([torch.zeros(1)], "nadam", LR)


def test_default_optimizer_is_still_torch_adam():
    s = SolverWrapper(_Net())
    assert type(s.optimizer) is torch.optim.Adam and s.opt is None and s.lr_scheduling == "const"
    assert s.optimizer.defaults["eps"] == 0.1 and s.optimizer.defaults["lr"] == cfg.TRAIN.LEARNING_RATE


@pytest.mark.parametrize("opt,steps_seen,final", [("sgd", [0, 1, 2, 3], 4), ("adam", [0, 0, 1, 1], 2),
                                                  ("amsgrad", [0, 0, 1, 1], 2), (None, [0, 0, 1, 1], 2)])
def test_alternating_global_step_rule(opt, steps_seen, final):
    """train_bus.py:293: under 'sgd' the supervised op is given the global step too, so both halves count it; the weak
    half (whose MIL scale factor reads the count) then sees 1, 3, ...; under the others only the weak half counts."""
    assert cfg.TRAIN.MOMENTUM == 0.9
    s = _Solver(opt=opt)
    for _ in range(2):
        s.train_step_alter("s", "ws")
    assert s.seen == steps_seen and s.global_step == final
    assert s.optimizer_ws is not None and s.optimizer_ws is not s.optimizer
    if opt is not None:
        assert s.optimizer.kind == s.optimizer_ws.kind == opt
        assert s.optimizer.t == s.optimizer_ws.t == 2            # each keeps its own state and step count
        assert s.optimizer.views is not s.optimizer_ws.views
        if opt == "sgd":
            assert s.optimizer.momentum == cfg.TRAIN.MOMENTUM


def test_schedules_reach_either_optimizer_family_before_each_step():
    for opt in (None, "adam", "sgd"):
        s = _Solver(opt=opt, lr=LR, lr_scheduling="pc", max_iters=4)          # boundary int(3.0) = 3
        used = []
        for _ in range(6):
            s._fake()
            s._apply()
            used.append(s.optimizer.param_groups[0]["lr"])
        assert used == [LR, LR, LR, LR, LR * 0.1, LR * 0.1], opt
        s = _Solver(opt=opt, lr=LR, lr_scheduling="rop")
        assert (s.rop.patience, s.rop.factor, s.rop.epsilon, s.rop.min_lr, s.rop.cooldown) == (5, 0.5, 1e-3, 0, 0)
        for _ in range(7):
            s.on_val_end(1.0)
        s._fake()
        s._apply()
        assert s.current_lr() == LR * 0.5 and s.optimizer.param_groups[0]["lr"] == LR * 0.5, opt
    s = _Solver(opt="adam")
    s.on_val_end(1.0)                                            # nothing to feed under 'const'
    assert s.current_lr() == s.lr


# ---------------------------------------------------------------- why the feature exists

def test_torch_adam_first_step_is_about_thirty_times_the_reference_forms():
    """At t = 1 both forms have m1 = (1 - b1) g and v1 = (1 - b2) g^2 = 1e-3 g^2.  TF's step is
    lr sqrt(1 - b2) / (1 - b1) * m1 / (sqrt(v1) + eps); torch's is lr / (1 - b1) * m1 / (sqrt(v1) / sqrt(1 - b2) + eps)
    = lr sqrt(1 - b2) / (1 - b1) * m1 / (sqrt(v1) + eps sqrt(1 - b2)).  The ratio torch / TF is therefore
        (sqrt(v1) + eps) / (sqrt(v1) + eps sqrt(1 - b2)).
    With |g| = 1e-2: sqrt(v1) = sqrt(1e-3) * 1e-2 = 3.162e-4, eps sqrt(1 - b2) = 0.1 * 3.162e-2 = 3.162e-3, so the
    ratio is (3.162e-4 + 0.1) / (3.162e-4 + 3.162e-3) = 0.1003162 / 0.0034785 = 28.84.  As |g| -> 0 it tends to
    1 / sqrt(1 - b2) = 31.62 and it falls as |g| grows, so for |g| around 1e-2 (half to twice: 30.2 .. 26.5) it lies in
    [25, 32]: that interval is asserted."""
    g0 = 1e-2
    ratio_formula = (math.sqrt(1e-3) * g0 + 0.1) / (math.sqrt(1e-3) * g0 + 0.1 * math.sqrt(1e-3))
    assert abs(ratio_formula - 28.84) < 0.01
    for sign in (1.0, -1.0):
        grad = torch.full((4,), sign * g0)
        a, b = torch.zeros(4, requires_grad=True), torch.zeros(4, requires_grad=True)
        a.grad, b.grad = grad.clone(), grad.clone()
        torch.optim.Adam([a], lr=LR, eps=0.1).step()
        O.ReferenceOptimizer([b], "adam", LR, eps=0.1).step()
        assert (a.detach() * sign < 0).all() and (b.detach() * sign < 0).all()
        ratio = float((a.detach() / b.detach()).mean())
        print("torch.optim.Adam step / reference-form step at t = 1, |g| = 1e-2: %.2f" % ratio)
        assert 25.0 <= ratio <= 32.0
        assert abs(ratio - ratio_formula) <= 1e-3 * ratio_formula
