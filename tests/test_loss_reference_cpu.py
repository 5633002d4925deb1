"""The f64 references and bounds of tests/loss_reference.py, established without a GPU.

* The references' values agree with oracle/np_oracle.py (loss_rpn_cross_entropy, loss_rpn_box, loss_rcnn_cross_entropy,
  loss_rcnn_box on every multi-task case; loss_mil on the three-class MIL cases) to 1e-12 relative, and the gradient
  references with torch autograd through a plain f64 log_softmax chain.
* The clean kernel model (model_mt / model_mil: the kernels' f32 arithmetic restated in torch, torch's f32 exp / log1p
  standing in for the device's under an allowance measured the same way) stays inside every bound on every case, with
  every exact-zero set exactly zero and no subnormal exp result outside the case "underflow".
* Each seeded defect misses a bound -- for the MIL selection an exact row index -- on a named case:
    lse_sum             backward probabilities through m + lz (the code before the difference form)   shift12 (both ops)
    log_of_sum          forward logf(1 + z) in place of log1pf(z)                                     below_block
    p_minus_1           the label's component as p_l - 1                                              below_block
    all_anchor_count    RPN mean over all anchors                                                     full_blocks
    box_images          box gradient live on image n_box_images                                       partial_nb1
    drop_tail           the last partial 2048-block skipped                                           partial_nb1
    le_threshold        |d| <= 1                                                                      below_block
    iw_once             9 iw d                                                                        below_block
    last_tie            MIL selects the last extremum                                                 five_alt
    bag_mean_nonempty   MIL mean over the non-empty bags                                              five_alt
"""
import numpy as np
import pytest
import torch

import loss_reference as R
from oracle import np_oracle as O

LOG = {}


@pytest.fixture(scope="module", autouse=True)
def allowance():
    """torch's own f32 exp / log1p on the CPU, measured like the device's"""
    ex, lg = R.lib_grids()
    we = R.lib_accuracy(torch.exp(ex), torch.exp(ex.double()))
    wl = R.lib_accuracy(torch.log1p(lg), torch.log1p(lg.double()))
    print("loss-lib-ulp cpu expf %.3f (subnormal %.3f, flushed %d) log1pf %.3f (subnormal %.3f, flushed %d)" % (we + wl))
    print("loss-lib-allowance cpu %s" % R.set_allowance(we[0], wl[0]))
    yield
    for k in sorted(LOG):
        print("loss-worst %s %.4g" % (k, LOG[k]))


def _mt_model_ratios(name, defects=()):
    c = R.make_mt_case(name)
    ref = R.mt_reference(c)
    terms, grads = R.model_mt(c, defects)
    return c, ref, R.mt_ratios(ref, terms, grads), R.mt_zero_violations(ref, grads)


def _mil_model(name, defects=()):
    c = R.make_mil_case(name)
    ref = R.mil_reference(c)
    rows, bag_loss, loss, grad = R.model_mil(c, defects)
    return c, ref, rows, R.mil_ratios(ref, loss, bag_loss, grad), int((grad[ref["zero"]] != 0).sum())


@pytest.mark.parametrize("name", list(R.MT_CASES))
def test_clean_model_inside_every_bound_multi_task(name):
    c, ref, ratios, zeros = _mt_model_ratios(name)
    R.check_ratios("cpu-model " + name, ratios, LOG)
    assert not any(zeros.values()), "%s: elements that must be exactly 0 are not: %s" % (name, zeros)
    assert (ref["sub"] > 0) == (name == "underflow"), "%s holds %d subnormal exp results" % (name, ref["sub"])
    if c["n_rows"] == 0:
        assert np.isnan(ref["terms"][2]) and not ref["grads"]["cls"].any() and not ref["grads"]["box"].any()


@pytest.mark.parametrize("name", list(R.MIL_CASES))
def test_clean_model_inside_every_bound_mil(name):
    c, ref, rows, ratios, nonzero = _mil_model(name)
    assert torch.equal(rows, ref["rows"])
    R.check_ratios("cpu-model mil " + name, ratios, LOG)
    assert nonzero == 0, "%s: %d gradient elements outside the selected rows are not 0" % (name, nonzero)
    assert (ref["sub"] > 0) == (name == "underflow"), "%s holds %d subnormal exp results" % (name, ref["sub"])
    empty = torch.tensor(c["sizes"]) == 0
    assert torch.equal(ref["rows"].cpu() < 0, empty) and not ref["bag_loss"][empty].any()


def test_case_makers_reach_what_they_claim():
    """every multi-task case with room for them holds the box specials; the MIL cases hold every kind of tie, each a
    real tie at the extremum whose first row the reference selects"""
    for name in R.MT_CASES:
        c = R.make_mt_case(name)
        _, lab, (tg, iw, ow) = R.rpn_views(c)
        d = (c["rpn_box"] - tg).reshape(-1)
        iw, ow = iw.reshape(-1), ow.reshape(-1)
        live = ow > 0
        assert float(ow.max()) > 0 and bool((d[live] == 1.0).any()) and bool((iw == 0.5).any()), name
        if int((lab >= 0).sum()) * 4 >= len(R._BOX_SPECIALS):
            for v in (-1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23, -1.0 - 2.0 ** -23, -1.0 + 2.0 ** -23, 0.0):
                assert bool((d[live] == v).any()), (name, v)
            assert bool(((iw == 0) & live & (d.abs() >= 1.0)).any()), name
        assert set(iw.tolist()) <= {0.0, 0.5, 1.0}, name
    kinds = set()
    for name in R.MIL_CASES:
        c = R.make_mil_case(name)
        rows, bag = R.mil_select(c), R.mil_bag_of_row(c)
        assert int((bag < 0).sum()) == 3 and int((bag >= c["n_bags"]).sum()) == 4, name
        for b, kind in c["ties"]:
            kinds.add(kind)
            col, sign = R.SEL_COL[c["sel"][0] if int(c["bag_labels"][b]) == 1 else c["sel"][1]]
            idx = (bag == b).nonzero().squeeze(1)
            v = sign * c["logits"][idx, col]
            at = idx[v == v.max()]
            assert at.numel() >= 2 and int(rows[b]) == int(at[0]), (name, b)
            if kind:
                assert at.tolist() == [int(at[0]), int(at[0]) + kind], (name, b, kind)
            else:
                assert at.numel() == idx.numel(), (name, b)
    assert kinds == {0, 1, 128, 256}


def _rel(a, b):
    """|a - b| relative to |b|, after the 4e (absolute) that the oracle's own log(sum exp) costs a cross-entropy: it
    rounds 1 + z to f64, which loses e of a term that may itself be as small as z"""
    return max(abs(a - b) - 4 * R.E, 0.0) / max(abs(b), 1e-300)


@pytest.mark.parametrize("name", list(R.MT_CASES))
def test_reference_values_equal_the_oracle_multi_task(name):
    c = R.make_mt_case(name)
    ref = R.mt_reference(c)
    npf = lambda t: t.numpy()
    N, H, W, A, nbi = c["dims"]
    lab = npf(c["labels"]).reshape(-1)
    live = lab >= 0
    want = [O.loss_rpn_cross_entropy(O.reshape_layer(npf(c["rpn_cls"]), 2), npf(c["rpn_labels"])),
            O.loss_rpn_box(npf(c["rpn_box"]), [npf(c[k]) for k in ("rpn_labels", "rpn_tg", "rpn_inw", "rpn_outw")], nbi)]
    if live.any():
        want.append(O.loss_rcnn_cross_entropy(npf(c["cls"])[:lab.size][live], lab[live]))
        want.append(O.loss_rcnn_box(npf(c["box"])[:lab.size][live], npf(c["tg"])[live], npf(c["inw"])[live],
                                    npf(c["outw"])[live]))
    else:
        assert np.isnan(ref["terms"][2]) and ref["terms"][3] == 0.0
    for i, w in enumerate(want):
        assert _rel(ref["terms"][i], w) <= 1e-12, (name, i, ref["terms"][i], w)


@pytest.mark.parametrize("name", [n for n, v in R.MIL_CASES.items() if v[0] == 3])
def test_reference_values_equal_the_oracle_mil(name):
    c = R.make_mil_case(name)
    ref = R.mil_reference(c)
    funcs = {0: O.mil_mal_max, 1: O.mil_ben_max, 2: O.mil_mass_max}
    bag = R.mil_bag_of_row(c).numpy()
    keep = [b for b in range(c["n_bags"]) if c["sizes"][b] > 0]         # the oracle has no notion of an empty bag
    rows = np.concatenate([np.nonzero(bag == b)[0] for b in keep])
    inds = np.repeat(np.arange(len(keep)), [c["sizes"][b] for b in keep])
    scale = float(torch.tensor(c["scale"], dtype=torch.float32).double())
    want = O.loss_mil(c["logits"].numpy()[rows], inds, c["bag_labels"].numpy()[keep], len(keep), 0,
                      [funcs[c["sel"][0]], funcs[c["sel"][1]]],
                      dict(WS_LOSS_USE_ADAPTIVE_SCALE_FACTOR=False, WS_LOSS_SCALE_FACTOR=scale,
                           WS_MAL_PCT=float(c["cw"][1].double()))) * len(keep) / c["n_bags"]
    # the class prior's third entry is the f32 of 1 - p here and 1 - the f32 of p there: 1e-7 apart at most
    assert _rel(ref["loss"], want) <= 2e-7, (name, ref["loss"], want)


@pytest.mark.parametrize("name", ["normal_k3", "partial_nb2", "shift10", "tie2"])
def test_reference_gradients_equal_autograd_in_float64(name):
    """The supervised chain in plain f64 torch ops (log_softmax, the box formulas with the f32 decisions as masks)"""
    c = R.make_mt_case(name)
    ref = R.mt_reference(c)
    N, H, W, A, nbi = c["dims"]
    K, n_rows = c["K"], c["n_rows"]
    leaves = [c[k].double().requires_grad_(True) for k in ("rpn_cls", "rpn_box", "cls", "box")]
    rpn_cls, rpn_box, cls, box = leaves
    s2 = rpn_cls.view(N, H, W, 2, A).permute(0, 1, 2, 4, 3).reshape(-1, 2)
    _, lab, (tg, iw, ow) = R.rpn_views(c)
    on = lab >= 0
    t0 = torch.nn.functional.cross_entropy(s2[on], lab[on])
    d = rpn_box - tg.double()
    inner = ((c["rpn_box"] - tg).abs() < 1.0).double()
    per = ow.double() * (0.5 * (iw.double() * d * 3) ** 2 * inner + (d.abs() - 0.5 / 9.0) * (1 - inner))
    t1 = per[:nbi].sum() * 10.0 / (nbi * 4 * A)
    labr = c["labels"].reshape(-1).long()
    live = labr >= 0
    t2 = torch.nn.functional.cross_entropy(cls[:n_rows][live], labr[live])
    bd32 = c["box"][:n_rows] - c["tg"]
    # |d| with the f32 sign (decisions are data): sgn32(d) * d
    t3 = (c["outw"].double() * c["inw"].double() * torch.sign(bd32).double() * (box[:n_rows] - c["tg"].double())).sum() / live.sum()
    terms = torch.stack([t0, t1, t2, t3])
    for i in range(4):
        assert _rel(float(terms[i].detach()), ref["terms"][i]) <= 1e-12, (name, i)
    (terms * c["gl"].double()).sum().backward()
    for k, leaf in zip(("rpn_cls", "rpn_box", "cls", "box"), leaves):
        g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        err = float((g - ref["grads"][k]).abs().max())
        assert err <= 1e-12 * max(float(g.abs().max()), 1e-30), (name, k, err)


DEFECT_CASES = [("lse_sum", "mt", "shift12"), ("lse_sum", "mil", "shift12"), ("log_of_sum", "mt", "below_block"),
                ("log_of_sum", "mil", "bags65"), ("p_minus_1", "mt", "below_block"), ("p_minus_1", "mil", "bags65"),
                ("all_anchor_count", "mt", "full_blocks"), ("box_images", "mt", "partial_nb1"),
                ("drop_tail", "mt", "partial_nb1"), ("le_threshold", "mt", "below_block"),
                ("iw_once", "mt", "below_block"), ("last_tie", "mil", "five_alt"),
                ("bag_mean_nonempty", "mil", "five_alt")]


def test_every_defect_has_a_case():
    assert {d for d, _, _ in DEFECT_CASES} == set(R.DEFECTS)


@pytest.mark.parametrize("defect,op,name", DEFECT_CASES)
def test_seeded_defect_misses_a_bound(defect, op, name):
    if op == "mt":
        _, _, ratios, zeros = _mt_model_ratios(name, (defect,))
        rows_differ = False
        ratios.update({"zero_" + k: float("inf") for k, v in zeros.items() if v})
    else:
        _, ref, rows, ratios, nonzero = _mil_model(name, (defect,))
        rows_differ = not torch.equal(rows, ref["rows"])
    missed = {k: v for k, v in ratios.items() if v > 1.0}
    print("loss-defect %s on %s %s: misses %s%s" % (defect, op, name, {k: "%.3g" % v for k, v in missed.items()},
                                                     ", selected rows differ" if rows_differ else ""))
    assert missed or rows_differ, "%s goes unnoticed on %s: %s" % (defect, name, ratios)
    if defect == "last_tie":
        assert rows_differ
