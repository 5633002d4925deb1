"""No GPU: the five bag functions of mil/core.py on the host -- hand-computed answers of disc-max and mean-ben, the host
mil_loss under all 25 pairs against the f64 statement of tests/mil_pool_reference.py (value and autograd gradient),
the name table and SolverWrapper's mil_funcs, --mil_funcs on both training command lines, and validation_losses'
unchanged default.

The host route is torch's own f32 arithmetic: its tolerance is mil_pool_reference.host_tolerance, reasoned there."""
import inspect

import pytest
import torch

import loss_reference as R
import mil_pool_reference as P

from wssdl_bus_amd.fast_rcnn import train_bus as T
from wssdl_bus_amd.fast_rcnn.config import cfg
from wssdl_bus_amd.mil import core as M


def _funcs(sel):
    return [M.MIL_FUNCS[P.NAMES[sel[0]]], M.MIL_FUNCS[P.NAMES[sel[1]]]]


# ---------------------------------------------------------------- known answers

def test_disc_max_known_answers():
    a = torch.tensor([[0.0, 1.0, 0.5], [0.0, 0.25, 3.0], [5.0, 3.0, -1.0], [9.0, 2.5, 2.75]])
    # keys 1, 3 (class 2), 3 (class 1), 2.75: rows 1 and 2 tie, the first wins
    assert M.get_disc_max_logit(a).tolist() == [[0.0, 0.25, 3.0]]
    # the largest foreground logit is class 1's (4 > 3): mal-max would take row 1
    b = torch.tensor([[0.0, 4.0, 1.0], [0.0, 1.0, 3.0]])
    assert M.get_disc_max_logit(b).tolist() == [[0.0, 4.0, 1.0]]
    assert M.get_mal_max_logit(b).tolist() == [[0.0, 1.0, 3.0]]
    # ... and class 2's (5 > 1): ben-max would take row 0; background never counts (row 2)
    c = torch.tensor([[0.0, 1.0, 0.5], [0.0, 0.5, 5.0], [99.0, 0.0, 0.0]])
    assert M.get_disc_max_logit(c).tolist() == [[0.0, 0.5, 5.0]]
    assert M.get_ben_max_logit(c).tolist() == [[0.0, 1.0, 0.5]]


def test_mean_ben_known_answers():
    a = torch.tensor([[9.0, 1.0, 7.0], [9.0, 2.0, 7.0], [9.0, 6.0, 7.0]])
    assert M.get_mean_ben_logit(a).tolist() == [[0.0, 3.0, 0.0]]
    assert M.get_mean_ben_logit(a[:1]).tolist() == [[0.0, 1.0, 0.0]]
    five = torch.tensor([[1.0, -2.0, 3.0, 4.0, 5.0], [1.0, 4.0, 3.0, 4.0, 5.0]])
    assert M.get_mean_ben_logit(five).tolist() == [[0.0, 1.0, 0.0, 0.0, 0.0]]


def test_get_bag_logit_takes_the_two_new_functions():
    logits = torch.tensor([[0.0, 1.0, 0.5], [0.0, 0.25, 3.0], [5.0, 3.0, -1.0],        # bag 0, label 1: disc-max
                           [9.0, 1.0, 7.0], [9.0, 2.0, 7.0], [9.0, 6.0, 7.0]],         # bag 1, label 2: mean-ben
                          requires_grad=True)
    inds = torch.tensor([0.0, 0, 0, 1, 1, 1])
    bag, scale = M.get_bag_logit(logits, inds, 3, torch.tensor([1, 2]), 2, [M.get_disc_max_logit, M.get_mean_ben_logit])
    assert bag.tolist() == [[0.0, 0.25, 3.0], [0.0, 3.0, 0.0]]
    want = torch.softmax(torch.tensor([[0.0, 0.25, 3.0], [0.0, 3.0, 0.0]]), 1)
    assert torch.allclose(scale, torch.stack([want[0, 1], want[1, 2]]))
    bag[1, 1].backward()                                          # the mean spreads its gradient over the bag
    assert torch.allclose(logits.grad[3:, 1], torch.full((3,), 1.0 / 3.0))
    assert not bool(logits.grad[:3].any()) and not bool(logits.grad[:, [0, 2]].any())
    # swapped pair, labels swapped: the same functions meet the same bags
    bag2, _ = M.get_bag_logit(logits.detach(), inds, 3, torch.tensor([2, 1]), 2, [M.get_mean_ben_logit, M.get_disc_max_logit])
    assert bag2.tolist() == bag.tolist()


# ---------------------------------------------------------------- the host loss under every pair

@pytest.fixture(scope="module")
def allowance():
    """the CPU's expf / log1pf are not measured; the reference's bounds are not used here, only its values"""
    old = dict(R.ALLOW)
    R.ALLOW.update(exp=R.MAX_ALLOWANCE, log1p=R.MAX_ALLOWANCE)
    yield
    R.ALLOW.clear()
    R.ALLOW.update(old)


@pytest.mark.parametrize("sel", P.ALL_PAIRS, ids=["%s-%s" % (P.NAMES[a], P.NAMES[b]) for a, b in P.ALL_PAIRS])
def test_host_mil_loss_every_pair(allowance, sel):
    step = 4100
    c = P.make_host_case(sel, seed=sel[0] * 5 + sel[1])
    pct = float(cfg.TRAIN.WS_MAL_PCT)
    c["cw"] = torch.tensor([0.0, pct, 1.0 - pct], dtype=torch.float64).float()
    c["scale"] = float(T._mil_scale(step))
    ref = P.reference(c)
    x = c["logits"].clone().requires_grad_(True)
    loss = T.mil_loss(x, c["col"], c["bag_labels"], c["n_bags"], step, _funcs(sel))
    loss.backward()

    tol_loss, tol_g = P.host_tolerance(c, ref)
    print("host %s loss %.9g ref %.9g tol %.3g" % (sel, float(loss.detach()), ref["loss"], tol_loss))
    assert abs(float(loss.detach()) - ref["loss"]) <= tol_loss
    err = (x.grad.double() - ref["grad"]).abs()
    print("host %s worst gradient error / tolerance %.3g" % (sel, R.ratio(x.grad, ref["grad"], tol_g)))
    assert bool((err <= tol_g).all())
    assert not bool((x.grad[ref["zero"]] != 0).any())


# ---------------------------------------------------------------- the reference's bounds hold a model of the kernels

MODEL_PAIRS = [(3, 4), (4, 3), (4, 4), (3, 3), (4, 0), (2, 4)]


@pytest.mark.parametrize("name", list(P.CASES))
def test_kernel_model_inside_the_counted_bounds(allowance, name):
    """the f32 model of csrc/mil.hip (mil_pool_reference.model) against the f64 statement: rows and counts equal, every
    output inside its bound, exact zeros where they must be -- and a mean accumulated in f32 is NOT inside (the
    nearly cancelling bag), so the bound of the mean is no wider than an f64 accumulation needs"""
    for sel in MODEL_PAIRS:
        c = P.make_case(name, sel)
        ref = P.reference(c)
        rows, counts, bag_logits, bag_loss, loss, grad = P.model(c)
        assert torch.equal(rows, ref["rows"]) and torch.equal(counts, ref["counts"])
        R.check_ratios("model %s %s" % (name, sel), P.ratios(ref, loss, bag_loss, grad, bag_logits))
        assert not bool((grad[ref["zero"]] != 0).any())
        assert bool(ref["zero"].any()) and not bool(ref["zero"].all())
    c = P.make_case("mixed_k3", (4, 4))
    ref = P.reference(c)
    _, _, members = P.select(c)
    acc = torch.zeros((), dtype=torch.float32)
    for v in c["logits"][members[2], 1]:                           # an f32 running sum in row order
        acc = acc + v
    assert abs(float(acc / 257.0) - float(ref["bag_logits"][2, 1])) > float(ref["b_logits"][2, 1])


# ---------------------------------------------------------------- names, solver, command lines

def test_every_name_resolves():
    assert list(M.MIL_FUNCS) == list(P.NAMES)
    assert [M._SELECTORS[M.MIL_FUNCS[n]] for n in P.NAMES] == [0, 1, 2, 3, 4]
    for a in P.NAMES:
        for b in P.NAMES:
            assert M.resolve_funcs((a, b)) == [M.MIL_FUNCS[a], M.MIL_FUNCS[b]]
    assert M.resolve_funcs([M.get_disc_max_logit, "mean_ben"]) == [M.get_disc_max_logit, M.get_mean_ben_logit]


def test_solver_takes_names_and_rejects_the_rest():
    net = torch.nn.Linear(2, 2)
    assert T.SolverWrapper(net).mil_funcs is None
    s = T.SolverWrapper(net, mil_funcs=("disc_max", "mean_ben"))
    assert s.mil_funcs == [M.get_disc_max_logit, M.get_mean_ben_logit]
    assert T.SolverWrapper(net, mil_funcs=[M.get_ben_max_logit, "mal_max"]).mil_funcs == [M.get_ben_max_logit, M.get_mal_max_logit]
    for bad in (("disc_max", "mean"), ("mal_max", "mal_max", "mal_max"), ("mal_max",), "mal_max", (max, "mal_max"), 3):
        with pytest.raises(ValueError):
            T.SolverWrapper(net, mil_funcs=bad)
    with pytest.raises(TypeError):                                # keyword-only
        T.SolverWrapper(net, None, None, None, "const", None, ("mal_max", "mal_max"))
    for fn in (T.train_net, T.train_net_alter):
        p = inspect.signature(fn).parameters["mil_funcs"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


@pytest.mark.parametrize("module", ["train", "train_alter"])
def test_mil_funcs_flag_parses(module, capsys):
    import importlib
    main = importlib.import_module("wssdl_bus_amd.main." + module)
    args = main.parser().parse_args(["--output_dir", "out", "--mil_funcs", "disc_max,mean_ben"])
    assert args.mil_funcs == [M.get_disc_max_logit, M.get_mean_ben_logit]
    assert main.parser().parse_args(["--output_dir", "out"]).mil_funcs is None
    for bad in ("disc_max", "disc_max,mean", "a,b,c"):
        with pytest.raises(SystemExit):
            main.parser().parse_args(["--output_dir", "out", "--mil_funcs", bad])
    capsys.readouterr()


def test_train_passes_the_pair_to_the_solver(monkeypatch):
    """train_net / train_net_alter -> train_loop._train -> SolverWrapper(mil_funcs=...)"""
    from wssdl_bus_amd.fast_rcnn import train_loop
    seen = []

    class Stop(Exception):
        pass

    def solver(*a, **k):
        seen.append(k.get("mil_funcs"))
        raise Stop

    monkeypatch.setattr(T, "SolverWrapper", solver)
    for fn in (T.train_net, T.train_net_alter):
        for pair in (None, ("disc_max", "mean_ben")):
            with pytest.raises(Stop):
                fn(None, None, None, None, None, None, None, "out", mil_funcs=pair)
    assert seen == [None, ("disc_max", "mean_ben")] * 2
    assert train_loop._train.__defaults__ == (None,)


# ---------------------------------------------------------------- validation_losses

def test_validation_losses_default_unchanged(monkeypatch):
    """funcs=None: the wiring's own pair, as before; a given pair goes through"""
    from wssdl_bus_amd.fast_rcnn import loss_op
    assert inspect.signature(T.validation_losses).parameters["funcs"].default is None
    assert T.default_mil_funcs(True) == [M.get_mass_max_logit, M.get_mal_max_logit]
    assert T.default_mil_funcs(False) == [M.get_mal_max_logit, M.get_mal_max_logit]
    seen = []
    monkeypatch.setattr(loss_op, "multi_task_loss_per_image", lambda *a: (torch.zeros((2, 4)), None))
    monkeypatch.setattr(T, "_mil_per_image", lambda cls, col, lab, n, step, funcs: seen.append(list(funcs)) or torch.zeros(2))
    layers = {k: None for k in ("rpn_cls_score", "rpn_bbox_pred", "bbox_pred", "rpn-data")}
    layers["cls_score"] = torch.zeros((6, 3))
    layers["roi-data"] = (torch.zeros((6, 5)),)
    im_info = torch.ones((2, 4))
    T.validation_losses(layers, im_info, 2, 0, True)
    T.validation_losses(layers, im_info, 2, 0, False)
    T.validation_losses(layers, im_info, 2, 0, True, [M.get_disc_max_logit, M.get_mean_ben_logit])
    assert seen == [[M.get_mass_max_logit, M.get_mal_max_logit], [M.get_mal_max_logit, M.get_mal_max_logit],
                    [M.get_disc_max_logit, M.get_mean_ben_logit]]
