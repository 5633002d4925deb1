#!/usr/bin/env python
"""Record what the RoI-pool exports answer on calls that never launch a kernel -> roi_pool_host_contract.json.

    python tests/golden/make_golden_roi_pool_host_contract.py

Three parts (tests/test_roi_pool_host_contract.py asserts that the library still gives them):
  status : the status code of every RoI-pool export that takes pointers, on argument sets that are rejected (or are
           a no-op) before the first HIP call -- NULL pointers, R == 0 / N == 0, bad rounding, unsupported shapes,
           plan ids out of range, too-small workspaces.  "fake" pointers are non-NULL values that are compared and
           aligned but never dereferenced; they appear only in cases whose other arguments stop the call first.
  rules  : the pure host rules and size queries over a grid of launch shapes, run-length coded (a run of equal values as [value, count]).
  tuned  : the rules that follow a tuning knob, under that knob.
No GPU is needed: nothing here reaches a launch.  A case that would launch must not be added (on a machine with a
GPU the fake pointers would be written through).
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "roi_pool_host_contract.json")

FAKE = 0x10000000                      # 256-byte aligned, never dereferenced
GOOD = dict(N=2, H=12, W=17, C=256, R=64, PH=7, PW=7, rounding=0, plan=0, owner=0, segments=1,
            ws_bytes=1 << 40, scratch_bytes=1 << 40, table_bytes=1 << 40, blocks_bytes=1 << 40)

# ---- the grid of part (b)
RS = (0, 256, 1024, 1536, 2048, 4000, 4128, 8512)
NS = (1, 2, 3, 4, 8)
HWS = ((38, 63), (37, 62), (63, 100), (12, 17))
CS = (64, 96, 256, 512, 768, 1024, 2048)
POOLED = (7, 8, 14)
SEGMENTS = (2, 17)
OWNER_PLANS = (0, 9, 12)


def _p(v):
    return ctypes.c_void_p(v) if v else None


def _call(L, name, a, ptrs):
    """One call of export `name` with the scalar arguments of `a`; every device pointer is ptrs[key] (default NULL)."""
    g = lambda k: _p(ptrs.get(k, ptrs.get("all", 0)))
    N, H, W, C, R, PH, PW, rd = a["N"], a["H"], a["W"], a["C"], a["R"], a["PH"], a["PW"], a["rounding"]
    sc = 0.0625
    if name == "wssdl_roi_pool_forward":
        return L[name](g("bottom"), N, H, W, C, g("rois"), R, PH, PW, sc, rd, g("top"), g("argmax"), None)
    if name == "wssdl_roi_pool_backward":
        return L[name](g("top_diff"), g("argmax"), g("rois"), R, N, H, W, C, PH, PW, sc, g("bottom_diff"), None)
    if name == "wssdl_roi_pool_backward_ws":
        return L[name](g("top_diff"), g("argmax"), g("rois"), R, N, H, W, C, PH, PW, sc, g("bottom_diff"), g("workspace"),
                       a["ws_bytes"], None)
    if name == "wssdl_roi_pool_forward_compact":
        return L[name](g("bottom"), N, H, W, C, g("rois"), R, PH, PW, sc, rd, g("top"), g("argmax"), g("overflow"), None)
    if name == "wssdl_roi_pool_forward_windows":
        return L[name](g("rois"), R, N, H, W, C, PH, PW, sc, rd, g("table"), a["table_bytes"], g("overflow"), None)
    if name == "wssdl_roi_pool_forward_compact_windows":
        return L[name](g("bottom"), N, H, W, C, g("rois"), R, PH, PW, sc, rd, g("table"), g("top"), g("argmax"), None)
    if name == "wssdl_roi_pool_forward_windows_blocks":
        return L[name](g("rois"), R, N, H, W, C, PH, PW, sc, rd, g("table"), a["table_bytes"], g("overflow"), g("blocks"),
                       a["blocks_bytes"], None)
    if name == "wssdl_roi_pool_forward_blocks_prepare":
        return L[name](g("bottom"), N, H, W, C, R, PH, PW, g("table"), g("blocks"), a["blocks_bytes"], None)
    if name == "wssdl_roi_pool_forward_compact_blocks":
        return L[name](g("bottom"), N, H, W, C, R, PH, PW, g("table"), g("blocks"), a["blocks_bytes"], g("top"), g("argmax"), None)
    if name == "wssdl_roi_pool_backward_prepare":
        plan = ctypes.c_int32(77)          # a real host word: the call writes -1 into it before it decides
        rc = L[name](g("rois"), R, N, H, W, C, PH, PW, sc, rd, g("workspace"), a["ws_bytes"],
                     ctypes.byref(plan) if a.get("plan_host", True) else None, None)
        return [rc, int(plan.value)]
    if name == "wssdl_roi_pool_backward_compact":
        return L[name](g("top_diff"), g("argmax"), g("rois"), R, N, H, W, C, PH, PW, sc, rd, g("bottom_diff"), g("workspace"),
                       a["ws_bytes"], a["plan"], None)
    if name == "wssdl_roi_pool_backward_compact_split":
        return L[name](g("top_diff"), g("argmax"), g("rois"), R, N, H, W, C, PH, PW, sc, rd, g("bottom_diff"), g("workspace"),
                       a["ws_bytes"], a["plan"], a["segments"], g("scratch"), a["scratch_bytes"], None)
    if name == "wssdl_roi_pool_backward_owner_prepare":
        return L[name](g("rois"), R, N, H, W, C, PH, PW, sc, rd, g("workspace"), a["ws_bytes"], a["owner"], None)
    if name == "wssdl_roi_pool_backward_compact_owner":
        return L[name](g("top_diff"), g("argmax"), g("rois"), R, N, H, W, C, PH, PW, sc, rd, g("bottom_diff"), g("workspace"),
                       a["ws_bytes"], a["owner"], g("scratch"), a["scratch_bytes"], None)
    if name == "wssdl_roi_pool_backward_compact_owner_split":
        return L[name](g("top_diff"), g("argmax"), g("rois"), R, N, H, W, C, PH, PW, sc, rd, g("bottom_diff"), g("workspace"),
                       a["ws_bytes"], a["owner"], a["segments"], g("scratch"), a["scratch_bytes"], None)
    if name == "wssdl_roi_pool_backward_owner_i32":
        return L[name](g("top_diff"), g("argmax"), g("rois"), R, N, H, W, C, PH, PW, sc, g("bottom_diff"), g("workspace"),
                       a["ws_bytes"], a["owner"], g("scratch"), a["scratch_bytes"], None)
    if name == "wssdl_roi_argmax_expand":
        return L[name](g("argmax8"), g("rois"), R, H, W, C, PH, PW, sc, rd, g("argmax"), None)
    raise KeyError(name)


EXPORTS = ("wssdl_roi_pool_forward", "wssdl_roi_pool_backward", "wssdl_roi_pool_backward_ws",
           "wssdl_roi_pool_forward_compact", "wssdl_roi_pool_forward_windows", "wssdl_roi_pool_forward_compact_windows",
           "wssdl_roi_pool_forward_windows_blocks", "wssdl_roi_pool_forward_blocks_prepare",
           "wssdl_roi_pool_forward_compact_blocks", "wssdl_roi_pool_backward_prepare", "wssdl_roi_pool_backward_compact",
           "wssdl_roi_pool_backward_compact_split", "wssdl_roi_pool_backward_owner_prepare",
           "wssdl_roi_pool_backward_compact_owner", "wssdl_roi_pool_backward_compact_owner_split",
           "wssdl_roi_pool_backward_owner_i32", "wssdl_roi_argmax_expand")

# every export, every pointer NULL: the first pointer check (or an earlier one) ends the call
NULL_SCENARIOS = (
    ("good", {}),
    ("R0", dict(R=0)),
    ("N0", dict(N=0)),
    ("R0_N0", dict(R=0, N=0)),
    ("R_neg", dict(R=-1)),
    ("N_neg", dict(N=-1)),
    ("rounding3", dict(rounding=3)),
    ("rounding3_R0", dict(rounding=3, R=0)),
    ("rounding3_N0", dict(rounding=3, N=0)),
    ("C70", dict(C=70)),
    ("C70_R0", dict(C=70, R=0)),
    ("C70_N0", dict(C=70, N=0)),
    ("H98_C64", dict(H=98, C=64)),
    ("H98_C64_R0", dict(H=98, C=64, R=0)),
    ("pooled1", dict(PH=1, PW=1)),
    ("pooled1_N0", dict(PH=1, PW=1, N=0)),
    ("pooled9", dict(PH=9, PW=9)),
    ("pooled9_R0", dict(PH=9, PW=9, R=0)),
    ("plan_neg", dict(plan=-1)),
    ("plan26", dict(plan=26)),
    ("owner12", dict(owner=12)),
    ("segments0", dict(segments=0)),
    ("no_plan_host", dict(plan_host=False)),
)

# the list-driven exports with every pointer a fake value: what stops the call is named by the case.  Only
# combinations that return before a launch (read off the source: a plan / segment / shape / size check, or the
# carving of a workspace that is too small).
_LIST = ("wssdl_roi_pool_backward_compact", "wssdl_roi_pool_backward_compact_split", "wssdl_roi_pool_backward_owner_prepare",
         "wssdl_roi_pool_backward_compact_owner", "wssdl_roi_pool_backward_compact_owner_split",
         "wssdl_roi_pool_backward_owner_i32", "wssdl_roi_pool_backward_prepare")
FAKE_SCENARIOS = (
    # (case, exports, scalar overrides, pointer overrides)
    ("ws16", _LIST, dict(ws_bytes=16), {}),
    ("ws16_rounding3", _LIST, dict(ws_bytes=16, rounding=3), {}),
    ("ws16_C70", _LIST, dict(ws_bytes=16, C=70), {}),
    ("ws16_N0", _LIST, dict(ws_bytes=16, N=0), {}),
    ("pooled9", tuple(e for e in _LIST if e != "wssdl_roi_pool_backward_prepare"), dict(PH=9, PW=9), {}),
    ("pooled9_null_ws", ("wssdl_roi_pool_backward_prepare",), dict(PH=9, PW=9), dict(workspace=0)),
    ("null_ws", ("wssdl_roi_pool_backward_prepare",), {}, dict(workspace=0)),
    ("null_ws_R0", ("wssdl_roi_pool_backward_prepare",), dict(R=0), dict(workspace=0)),
    ("plan26", ("wssdl_roi_pool_backward_compact", "wssdl_roi_pool_backward_compact_split"), dict(plan=26), {}),
    ("plan26_ws16", ("wssdl_roi_pool_backward_compact", "wssdl_roi_pool_backward_compact_split"), dict(plan=26, ws_bytes=16), {}),
    ("plan_neg", ("wssdl_roi_pool_backward_compact_split",), dict(plan=-1), {}),
    ("plan0_null_ws", ("wssdl_roi_pool_backward_compact", "wssdl_roi_pool_backward_compact_split"), {}, dict(workspace=0)),
    ("segments0", ("wssdl_roi_pool_backward_compact_split", "wssdl_roi_pool_backward_compact_owner_split"), dict(segments=0), {}),
    ("segments17_ws16", ("wssdl_roi_pool_backward_compact_split", "wssdl_roi_pool_backward_compact_owner_split"),
     dict(segments=17, ws_bytes=16), {}),
    ("segments2_scratch16", ("wssdl_roi_pool_backward_compact_split", "wssdl_roi_pool_backward_compact_owner_split"),
     dict(segments=2, scratch_bytes=16), {}),
    ("segments2_null_scratch", ("wssdl_roi_pool_backward_compact_split", "wssdl_roi_pool_backward_compact_owner_split"),
     dict(segments=2), dict(scratch=0)),
    ("segments2_scratch16_plan_neg", ("wssdl_roi_pool_backward_compact_split",), dict(segments=2, scratch_bytes=16, plan=-1), {}),
    ("segments0_scratch16",("wssdl_roi_pool_backward_compact_owner_split",), dict(segments=0, scratch_bytes=16), {}),
    ("owner12", ("wssdl_roi_pool_backward_owner_prepare", "wssdl_roi_pool_backward_compact_owner",
                 "wssdl_roi_pool_backward_compact_owner_split", "wssdl_roi_pool_backward_owner_i32"), dict(owner=12), {}),
    ("owner12_scratch16", ("wssdl_roi_pool_backward_compact_owner", "wssdl_roi_pool_backward_compact_owner_split",
                           "wssdl_roi_pool_backward_owner_i32"), dict(owner=12, scratch_bytes=16), {}),
    ("owner_neg", ("wssdl_roi_pool_backward_owner_prepare", "wssdl_roi_pool_backward_compact_owner",
                   "wssdl_roi_pool_backward_compact_owner_split", "wssdl_roi_pool_backward_owner_i32"), dict(owner=-1), {}),
    ("scratch16", ("wssdl_roi_pool_backward_compact_owner", "wssdl_roi_pool_backward_compact_owner_split",
                   "wssdl_roi_pool_backward_owner_i32"), dict(scratch_bytes=16), {}),
    ("null_scratch", ("wssdl_roi_pool_backward_compact_owner", "wssdl_roi_pool_backward_compact_owner_split",
                      "wssdl_roi_pool_backward_owner_i32"), {}, dict(scratch=0)),
    ("scratch_misaligned", ("wssdl_roi_pool_backward_compact_owner", "wssdl_roi_pool_backward_compact_owner_split",
                            "wssdl_roi_pool_backward_owner_i32"), {}, dict(scratch=FAKE + 4)),
    ("bottom_diff_misaligned", ("wssdl_roi_pool_backward_compact_owner", "wssdl_roi_pool_backward_compact_owner_split",
                                "wssdl_roi_pool_backward_owner_i32"), {}, dict(bottom_diff=FAKE + 4)),
    ("argmax_misaligned", ("wssdl_roi_pool_backward_owner_i32",), {}, dict(argmax=FAKE + 4)),
    ("top_diff_misaligned", ("wssdl_roi_pool_backward_owner_i32",), {}, dict(top_diff=FAKE + 4)),
    ("C96", ("wssdl_roi_pool_backward_owner_i32",), dict(C=96), {}),                 # not a power of two: no i32 walk
    ("C66_ws16", ("wssdl_roi_pool_backward_owner_prepare", "wssdl_roi_pool_backward_compact_owner"), dict(C=66, ws_bytes=16), {}),
    ("null_rois", ("wssdl_roi_pool_backward_owner_prepare", "wssdl_roi_pool_backward_prepare"), {}, dict(rois=0)),
    ("null_rois_R0_ws16", ("wssdl_roi_pool_backward_owner_prepare", "wssdl_roi_pool_backward_prepare"), dict(R=0, ws_bytes=16),
     dict(rois=0)),
    # the forward's tables
    ("table16", ("wssdl_roi_pool_forward_windows", "wssdl_roi_pool_forward_windows_blocks"), dict(table_bytes=16), {}),
    ("table_misaligned", ("wssdl_roi_pool_forward_windows", "wssdl_roi_pool_forward_windows_blocks"), {}, dict(table=FAKE + 4)),
    ("table_misaligned_R0", ("wssdl_roi_pool_forward_windows", "wssdl_roi_pool_forward_windows_blocks"), dict(R=0),
     dict(table=FAKE + 4)),
    ("table16_rounding3", ("wssdl_roi_pool_forward_windows", "wssdl_roi_pool_forward_windows_blocks"),
     dict(table_bytes=16, rounding=3), {}),
    ("pooled8", ("wssdl_roi_pool_forward_windows", "wssdl_roi_pool_forward_windows_blocks", "wssdl_roi_pool_forward_compact_windows",
                 "wssdl_roi_pool_forward_blocks_prepare", "wssdl_roi_pool_forward_compact_blocks"), dict(PH=8, PW=8), {}),
    ("C768", ("wssdl_roi_pool_forward_windows", "wssdl_roi_pool_forward_windows_blocks", "wssdl_roi_pool_forward_compact_windows",
              "wssdl_roi_pool_forward_blocks_prepare", "wssdl_roi_pool_forward_compact_blocks"), dict(C=768), {}),
    ("N0", ("wssdl_roi_pool_forward_windows", "wssdl_roi_pool_forward_windows_blocks", "wssdl_roi_pool_forward_blocks_prepare",
            "wssdl_roi_pool_forward_compact_blocks"), dict(N=0), {}),
    ("blocks16", ("wssdl_roi_pool_forward_windows_blocks", "wssdl_roi_pool_forward_blocks_prepare",
                  "wssdl_roi_pool_forward_compact_blocks"), dict(blocks_bytes=16), {}),
    ("blocks_misaligned", ("wssdl_roi_pool_forward_windows_blocks", "wssdl_roi_pool_forward_blocks_prepare",
                           "wssdl_roi_pool_forward_compact_blocks"), {}, dict(blocks=FAKE + 16)),
    ("H3", ("wssdl_roi_pool_forward_windows_blocks", "wssdl_roi_pool_forward_blocks_prepare",
            "wssdl_roi_pool_forward_compact_blocks"), dict(H=3), {}),
    ("bottom_misaligned", ("wssdl_roi_pool_forward_compact", "wssdl_roi_pool_forward_compact_windows",
                           "wssdl_roi_pool_forward_blocks_prepare", "wssdl_roi_pool_forward_compact_blocks"), {},
     dict(bottom=FAKE + 4)),
    ("top_misaligned", ("wssdl_roi_pool_forward_compact", "wssdl_roi_pool_forward_compact_windows",
                        "wssdl_roi_pool_forward_compact_blocks"), {}, dict(top=FAKE + 4)),
    ("argmax_misaligned", ("wssdl_roi_pool_forward_compact", "wssdl_roi_pool_forward_compact_windows",
                           "wssdl_roi_pool_forward_compact_blocks"), {}, dict(argmax=FAKE + 1)),
    ("argmax_misaligned", ("wssdl_roi_argmax_expand",), {}, dict(argmax=FAKE + 4)),
    ("argmax8_misaligned", ("wssdl_roi_argmax_expand",), {}, dict(argmax8=FAKE + 1)),
    # (wssdl_roi_argmax_expand does not look at the rounding mode before it launches: no such case for it)
    ("rounding3", ("wssdl_roi_pool_forward_compact", "wssdl_roi_pool_forward_compact_windows"), dict(rounding=3), {}),
    ("C70", ("wssdl_roi_pool_forward_compact", "wssdl_roi_pool_forward_compact_windows", "wssdl_roi_argmax_expand"), dict(C=70), {}),
    ("N0", ("wssdl_roi_pool_forward_compact", "wssdl_roi_pool_forward_compact_windows"), dict(N=0), {}),
    ("R0", ("wssdl_roi_pool_forward_compact", "wssdl_roi_pool_forward_compact_windows", "wssdl_roi_argmax_expand",
            "wssdl_roi_pool_forward", "wssdl_roi_pool_forward_windows"), dict(R=0), {}),
    ("N0", ("wssdl_roi_pool_backward", "wssdl_roi_pool_backward_ws") + _LIST[:6], dict(N=0), {}),
)


def record_status(L):
    out = {}
    for case, over in NULL_SCENARIOS:
        a = dict(GOOD, **over)
        for e in EXPORTS:
            out["%s|null|%s" % (e, case)] = _call(L, e, a, {})
    for case, exports, over, ptrs in FAKE_SCENARIOS:
        a = dict(GOOD, **over)
        for e in exports:
            out["%s|fake|%s" % (e, case)] = _call(L, e, a, dict(dict(all=FAKE), **ptrs))
    return out


def _rle(values):
    """[v, v, v, w] -> [[v, 3], w]: a run of equal values as a pair, a single value as itself."""
    runs = []
    for v in values:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([int(v), 1])
    return [r if r[1] > 1 else r[0] for r in runs]


def _hw(args):          # ((H, W), ...) pairs flattened in place
    flat = []
    for x in args:
        flat += list(x) if isinstance(x, tuple) else [x]
    return flat


# export -> the axes of its grid, in argument order ("P" = pooled_h, pooled_w)
RULES = (
    ("wssdl_roi_pool_backward_split_segments", (RS, NS, HWS, CS)),
    ("wssdl_roi_pool_backward_owner_plan", (RS, NS, HWS, CS)),
    ("wssdl_roi_pool_backward_owner_plan_for", (RS, NS, HWS, CS, "P")),
    ("wssdl_roi_pool_backward_owner_segments", (RS, NS, HWS, CS)),
    ("wssdl_roi_pool_forward_blocks_auto", (RS, NS, HWS, CS, "P")),
    ("wssdl_roi_pool_backward_workspace_bytes", (RS, NS, HWS, "P")),
    ("wssdl_roi_pool_backward_status_offset", (RS, NS, HWS, "P")),
    ("wssdl_roi_pool_forward_windows_bytes", (RS, HWS, CS, "P")),
    ("wssdl_roi_pool_forward_blocks_bytes", (RS, NS, HWS, CS, "P")),
    ("wssdl_roi_pool_backward_split_scratch_bytes", (NS, HWS, CS, SEGMENTS)),
    ("wssdl_roi_pool_backward_owner_scratch_bytes", (NS, HWS, CS, OWNER_PLANS)),
    ("wssdl_roi_pool_backward_owner_split_scratch_bytes", (NS, HWS, CS, OWNER_PLANS, SEGMENTS)),
    ("wssdl_roi_pool_compact_supported", (HWS, CS, "P")),
)
TUNED = (
    ("roi_bwd_owner", -2, ("wssdl_roi_pool_backward_owner_plan", "wssdl_roi_pool_backward_owner_plan_for")),
    ("roi_bwd_owner_segments", 3, ("wssdl_roi_pool_backward_owner_segments",)),
    ("roi_fwd_blocks", 0, ("wssdl_roi_pool_forward_blocks_auto",)),
    ("roi_fwd_blocks", 1, ("wssdl_roi_pool_forward_blocks_auto",)),
)


def _grid(L, name):
    axes = [tuple((p, p) for p in POOLED) if ax == "P" else ax for ax in dict(RULES)[name]]
    return _rle(L[name](*_hw(args)) for args in itertools.product(*axes))


def record(lib_module):
    """{"status": .., "rules": .., "tuned": ..} from the loaded library (wssdl_bus_amd._lib)."""
    L = lib_module.lib()
    fns = {name: getattr(L, name) for name in EXPORTS + tuple(n for n, _ in RULES)}
    out = dict(status=record_status(fns), rules={name: _grid(fns, name) for name, _ in RULES}, tuned={})
    for knob, value, names in TUNED:
        with lib_module.tuned(**{knob: value}):
            for name in names:
                out["tuned"]["%s=%d|%s" % (knob, value, name)] = _grid(fns, name)
    return out


def main():
    from wssdl_bus_amd import _lib, build
    build.build(verbose=False)
    got = record(_lib)
    with open(OUT, "w") as f:
        f.write("{\n")
        for i, part in enumerate(("status", "rules", "tuned")):
            f.write(' "%s": {\n' % part)
            items = sorted(got[part].items())
            f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in items))
            f.write("\n }%s\n" % ("," if i < 2 else ""))
        f.write("}\n")
    n = sum(len(v) for p in ("rules", "tuned") for v in got[p].values()) + len(got["status"])
    assert 3 not in [v if isinstance(v, int) else v[0] for v in got["status"].values()], "a case reached a launch"
    print("wrote %s: %d status codes, %d integers in all, %d bytes" % (OUT, len(got["status"]), n, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
