"""-m gpu: the stream-order contract of the device ops (tests/stream_order.py) over the shared case table.

Every case of tests/device_op_cases.py runs once on the default stream (the baseline), once on a decoy input, and twice
on a non-blocking side stream: behind a delay and an input copy on that stream (the producer leg), and next to a delay on
the default stream (the busy-default leg).  Both side-stream results must have the baseline's bits.  See stream_order.py
for what each leg catches and for what the harness cannot see.

Three tables keep the exceptions in one place:
  SYNCS        case prefixes whose wrapper synchronises the host, each with the sentence of the wrapper's docstring that
               says it returns host values (tests/test_stream_order_cpu.py holds the sentences to the package).  Every
               other case runs under torch.cuda.set_sync_debug_mode("error"); a listed case must in fact synchronise.
  DECOYS       case prefixes whose result does not move when every value is halved, with the decoy they get instead.
  VACUOUS_OK   case prefixes for which no decoy can exist, with the reason.  Their producer leg distinguishes nothing; the
               busy-default leg still does.

The last tests prove the harness on fake ops made of torch elementwise operators: one correct op passes, four defective
ones are rejected."""
import pytest
import torch

import stream_order as so
from device_op_cases import CASES, N_MEMORY_CONTRACT_CASES, N_STREAM_ORDER_ADDED, _defined_for, _flags

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOTALS = {}
RECORDS = []

assert N_MEMORY_CONTRACT_CASES == 407 and len(CASES) == 407 + N_STREAM_ORDER_ADDED == 424, len(CASES)

# (case prefixes, the sentence of the wrapper's docstring that says the call returns host values or reads the device back)
_PROPOSAL_MAPS = ("one_cell", "below_one_run", "below_one_run-empty", "over_one_run")
_ANCHOR_REFERENCE = ("1x1_small-single", "1x1_small-joint", "1x1_outside-joint", "3x4_small_fg-single", "3x4_small_joint-joint",
                     "14x17_fg-single", "14x17_joint-joint", "14x17_all-single")
SYNCS = (
    (("nms-",), "Synchronises the host: the number of kept boxes is read back to size the result."),
    (tuple("proposal-%s-%s-compact" % (m, t) for m in _PROPOSAL_MAPS for t in ("train", "test")),
     "Without cfg.PADDED_ROIS the per-image counts are read back to compact the blob, which synchronises the host"),
    (tuple("anchor-%s-reference" % a for a in _ANCHOR_REFERENCE),
     "on a host copy of the labels, consuming `rng` (numpy.random by default) exactly like the reference."),
    (("roi-targets-r1-joint", "roi-targets-r70-joint", "roi-targets-r257-joint"),
     "Rows of the weak `images`, in order (hint from the proposal layer, else read-back)."),
    (("roi-targets-r1-single-reference", "roi-targets-r70-single-reference", "roi-targets-r257-single-reference"),
     "the overlaps are read back and the rows are drawn on the host, which synchronises it"),
    (("roi-align-mixed-tables", "roi-align-axes-tables"),
     "The axis tables of the RoIs on a map of `shape` = (N, H, W, C): a dict of NumPy arrays"),
    (("image-batch-blob-",), "Every plane goes up in a blocking copy of its own, which synchronises the host once per image."),
    (("val-detect-mixed-bounds", "val-detect-one_row-bounds", "val-detect-wide-bounds"),
     "With im_shapes the bounds go up in a blocking copy from the host, which synchronises it"),
    (("eval-detections-",), "GPU inputs: one device op and one read-back of the small outputs."),
    (("proposal-recall-",), "One read-back of the summary (hits, num_pos, flags), one of the overlaps the cells' gt_overlaps are sorted from"),
    (("draw-detections-",),
     "The planes go up in one copy, the op runs once for all N images, and the output arena comes back in one copy."),
    (("optimiser-",), "Built once per parameter list, with two blocking copies from the host that synchronise it"),
)

# (case prefixes, decoy, why halving changes nothing)
DECOYS = (
    (("nms-",), so.reversed_rows("dets"),
     "greedy NMS returns indices: halving every box and score keeps the order and (up to the +1 pixel) the overlaps"),
    (("image-prep-", "image-adjust-f64-"), so.complemented_u8,
     "the input is a uint8 grey plane, which the default decoy leaves alone: its complement 255 - x is another image"),
)

# (case prefixes, why no decoy can change the result)
VACUOUS_OK = (
    (tuple("nms-%s-n1-" % r for r in ("nms", "nms_new")), "one box: keep is [0] whatever the box holds"),
    (("anchor-1x1_outside-",), "every anchor of the map lies outside the image: no label depends on a ground-truth value"),
    (("roi-align-empty-",), "no RoI: empty outputs and a zero gradient whatever the map holds"),
    (("image-warp-constant-clip",), "the one output pixel maps outside the source: it is cval whatever the image holds"),
    (("image-batch-blob-", "proposal-recall-", "shifted-anchors-"),
     "the op is fed from host arrays that the wrapper uploads itself: the case has no device input to hold a decoy"),
    (("l2-decay",), "the parameters are the case's own leaves (their .grad is the result), not tensors the harness can swap"),
    (("post-detect-per-class-r0", "post-detect-per-class-batched-r0", "post-detect-agnostic-r0", "post-detect-agnostic-batched-r0"),
     "no rows: every count is zero whatever the inputs hold"),
    (("post-detect-per-class-batched-r1", "post-detect-agnostic-batched-r1"),
     "the one row belongs to no image (batch index -1): every count is zero whatever it holds"),
    (("groupnorm-2x65x1024-large-first_last_dead",), "both samples are dead under the mask: every output is zero whatever x holds"),
)


def _lookup(table, name):
    hit = [row for row in table if name.startswith(row[0])]
    assert len(hit) <= 1, (name, [row[0] for row in hit])
    return hit[0] if hit else None


def sync_free(name):
    return _lookup(SYNCS, name) is None


@pytest.fixture(scope="module", autouse=True)
def _totals():
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    _lib.lib()
    print("\nstream-order delay calibration: %.0f sleep cycles per ms" % so.cycles_per_ms())
    yield
    if RECORDS:
        unc, free, share = so.uncovered_share(RECORDS)
        print("\nstream-order totals: cases=%d sync_free=%d uncovered=%d (%.2f %%) vacuity_overrides=%d default_delay_pending=%d "
              "len(SYNCS)=%d" % (TOTALS.get("cases", 0), free, unc, 100.0 * share, TOTALS.get("vacuity_overrides", 0),
                                 sum(r["default_pending"] for r in RECORDS), len(SYNCS)))
        so.assert_uncovered_share(RECORDS)


@pytest.mark.parametrize("name", list(CASES))
def test_stream_order(name):
    builder, _floor = CASES[name]
    spec = builder()
    fn, inputs = spec["fn"], spec["inputs"]
    flags = _flags() if spec.get("flags", True) else None
    free = sync_free(name)
    decoy = _lookup(DECOYS, name)
    try:
        fn(inputs)                                  # warm-up: allocator, module-level caches (not under the debugger)
        if free:
            so.assert_sync_free(fn, inputs, name)
        else:
            assert so.synchronises(fn, inputs), "stream-order %s is listed in SYNCS and does not synchronise" % name
        if flags is not None:
            flags()                                 # cleared: what this case raises is this case's
        so.run_case(fn, inputs, name=name, decoy=spec.get("decoy", decoy[1] if decoy else None), defined=_defined_for(name),
                    flags_raised=flags, sync_free=free, vacuous_ok=_lookup(VACUOUS_OK, name) is not None, totals=TOTALS,
                    records=RECORDS)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("stream-order %s: the device faulted (%s); nothing more is started on it" % (name, e), returncode=3)
        raise


def test_every_table_prefix_names_a_case():
    for table in (SYNCS, DECOYS, VACUOUS_OK):
        for row in table:
            assert all(any(n.startswith(p) for n in CASES) for p in row[0]), row[0]


# ------------------------------------------------------------------------------------------ the harness is live -----
# Fake ops: torch elementwise operators on 4 KiB tensors.  No custom kernel, nothing that can fault.

def _fake_inputs():
    g = torch.Generator(device=DEV).manual_seed(3)
    return {"x": torch.randn((1024,), device=DEV, generator=g) + 3.0, "k": torch.arange(1024, device=DEV, dtype=torch.int32)}


def _work(x, k):
    return (x * 2.0 + 1.0) * (k % 7 + 1).to(x.dtype)


def test_harness_passes_a_correct_op():
    recs = []
    so.run_case(lambda inp: (_work(inp["x"], inp["k"]),), _fake_inputs(), name="fake-correct", records=recs)
    assert len(recs) == 1 and not recs[0]["vacuous"]


def test_harness_rejects_work_on_the_default_stream():
    def fn(inp):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return (_work(inp["x"], inp["k"]),)
    with pytest.raises(so.StreamOrderViolation) as e:
        so.run_case(fn, _fake_inputs(), name="fake-default-stream")
    torch.cuda.synchronize()
    print("rejected: %s" % str(e.value)[:160])


def test_harness_rejects_work_on_a_private_stream_that_does_not_wait():
    private = torch.cuda.Stream()

    def fn(inp):
        with torch.cuda.stream(private):
            return (_work(inp["x"], inp["k"]),)
    with pytest.raises(so.StreamOrderViolation) as e:
        so.run_case(fn, _fake_inputs(), name="fake-private-stream")
    torch.cuda.synchronize()
    print("rejected: %s" % str(e.value)[:160])


def test_harness_rejects_a_table_cached_on_the_first_stream_seen():
    """the op keeps a device table per input buffer, built from the inputs on the stream of its very first call and never
    ordered against the caller's stream: fresh buffers on a side stream get a table computed before their values landed"""
    state = {"stream": None, "tables": {}}

    def fn(inp):
        if state["stream"] is None:
            state["stream"] = torch.cuda.current_stream()
        key = inp["x"].data_ptr()
        if key not in state["tables"]:
            with torch.cuda.stream(state["stream"]):
                state["tables"][key] = inp["x"] * 3.0
        return (_work(inp["x"], inp["k"]) + state["tables"][key],)
    with pytest.raises(so.StreamOrderViolation) as e:
        so.run_case(fn, _fake_inputs(), name="fake-cached-table")
    torch.cuda.synchronize()
    print("rejected: %s" % str(e.value)[:160])


def test_harness_rejects_a_decoy_that_tests_nothing():
    with pytest.raises(so.VacuousDecoy, match="decoy tests nothing") as e:
        so.run_case(lambda inp: ((inp["x"] > 0.0), inp["k"] + 1), _fake_inputs(), name="fake-vacuous")
    torch.cuda.synchronize()
    print("rejected: %s" % str(e.value)[:160])
