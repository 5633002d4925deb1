"""Stream-order harness for the device ops: does an op enqueue ALL of its work on the caller's stream?

include/wssdl_bus_hip.h promises that every call "only enqueues kernels on `stream`".  On torch's default stream, where
every other test runs, a kernel, memset or copy that goes to stream 0 instead, a cached device table built on whichever
stream was current first, or a hidden dependency on the null stream all give the right bits.  ``run_case`` makes them
visible.  For one op ``fn(inputs)``:

1. baseline: ``fn(inputs)`` on the default stream, then a device synchronise;
2. decoy baseline: ``fn(decoy(inputs))`` on the default stream.  The default decoy halves every floating tensor and
   leaves integer, bool and uint8 tensors as they are: boxes stay ordered, indices stay in range, sorted lists stay
   sorted.  A case may bring its own decoy; it must be an input the op is specified for.  The decoy result must differ
   from the baseline in a defined leaf and raise no flag (the vacuity floor), else the case fails with "decoy tests
   nothing";
3. producer leg: on a non-blocking side stream S, inputs allocated on S and holding the decoy; then, with no host
   synchronisation in between: a delay kernel, ``x_side.copy_(x)`` for every input, ``fn(side_inputs)``, a clone of every
   result tensor.  S is synchronised and the clones must have the baseline's bits.  Work enqueued anywhere but S runs
   before the copy lands: it computes the decoy's result or reads intermediates nobody wrote yet;
4. busy-default leg: a scrub run of ``fn`` on the decoy on S (so that the blocks the allocator hands out again hold the
   decoy's intermediates, not the right ones), the inputs put back, a synchronise; then the same delay on the DEFAULT
   stream, ``fn`` on S, the clones on S, and a synchronise of S only.  Work wrongly placed on stream 0 sits behind the
   delay and the clones hold stale bits.  Whether the delay was still pending when S finished is printed, never asserted.

The delay is ``torch.cuda._sleep``: one workgroup, so it takes no compute unit from an op whose workgroups wait for each
other (the fused NMS launch).  Its length is max(5 ms, 3 x the host wall time of fn in the baseline run).  In the producer
leg the delay is timed with events on S and fn's host time is taken in that very run: a case whose delay came out shorter
than its host time had a window in which late launches could not be told apart, and counts as UNCOVERED.  Nothing is
re-run; ``uncovered_share`` caps the share of such cases over a module.

Results are compared with ``guarded_alloc.bit_differences`` on their defined part (the caller's UNDEFINED cuts).

What this cannot see:
  * kernels launched after a wrapper's own host synchronisation (by then S has drained: the delay and the copy are done);
  * captured graphs (a capture records the stream of every node; replay order is the graph's, not the streams');
  * two ops running at once (one op runs at a time here; contention between ops is not exercised);
  * more than one device.
"""
import time

import numpy as np
import torch

import guarded_alloc as ga

MIN_DELAY_MS = 5.0
DELAY_FACTOR = 3.0
MAX_UNCOVERED_SHARE = 0.02


class StreamOrderViolation(AssertionError):
    pass


class VacuousDecoy(AssertionError):
    pass


# ---- the decoy -----------------------------------------------------------------------------------------------------
def _map_tensors(inputs, f):
    if isinstance(inputs, dict):
        return {k: (f(k, v) if isinstance(v, torch.Tensor) else v) for k, v in inputs.items()}
    return [f(i, v) if isinstance(v, torch.Tensor) else v for i, v in enumerate(inputs)]


def halved(t):
    """the default decoy of one tensor: floating values halved (exact: no rounding but at the subnormal end), everything
    else a plain copy; strides are kept"""
    t = t.detach()
    if t.is_floating_point():
        return t * 0.5
    return t.clone(memory_format=torch.preserve_format)


def default_decoy(inputs):
    return _map_tensors(inputs, lambda _k, v: halved(v))


def reversed_rows(key):
    """a decoy for ops whose result does not move when every value is halved (greedy NMS: same order, same overlaps up
    to the +1 pixel): the rows of inputs[key] in reverse order, every other input as it is"""
    def decoy(inputs):
        return _map_tensors(inputs, lambda k, v: v.detach().flip(0).contiguous() if k == key
                            else v.detach().clone(memory_format=torch.preserve_format))
    return decoy


def complemented_u8(inputs):
    """a decoy for ops that read uint8 images, which halving leaves alone: every uint8 tensor becomes 255 - x (another
    valid image), every other tensor gets the default rule"""
    return _map_tensors(inputs, lambda _k, v: (255 - v.detach()) if v.dtype == torch.uint8 else halved(v))


# ---- the vacuity floor ---------------------------------------------------------------------------------------------
def check_vacuity(name, base_flat, decoy_flat, flag_up):
    """base_flat / decoy_flat: guarded_alloc._flatten of the two defined results.  Raises VacuousDecoy unless the decoy's
    result differs from the baseline in at least one defined leaf and raised no device flag."""
    if flag_up:
        raise VacuousDecoy("stream-order %s: decoy tests nothing: the decoy raised a device flag, it is no input the op "
                           "is specified for" % name)
    if not ga._diff_flat(base_flat, decoy_flat, "result"):
        raise VacuousDecoy("stream-order %s: decoy tests nothing: the decoy's result has the baseline's bits in every "
                           "defined leaf" % name)


# ---- the uncovered share -------------------------------------------------------------------------------------------
def is_uncovered(record):
    """record: dict(delay_ms=, host_ms=, sync_free=).  Only a sync-free case can be uncovered: a case that synchronises
    drains S itself, and what it launches afterwards is outside what the harness sees (module docstring)."""
    return bool(record["sync_free"]) and record["delay_ms"] < record["host_ms"]


def uncovered_share(records):
    """(uncovered, sync_free, share) over the recorded cases; share = uncovered / sync_free (0 without sync-free cases)"""
    free = [r for r in records if r["sync_free"]]
    unc = [r for r in free if is_uncovered(r)]
    return len(unc), len(free), (len(unc) / float(len(free)) if free else 0.0)


def assert_uncovered_share(records, cap=MAX_UNCOVERED_SHARE):
    unc, free, share = uncovered_share(records)
    assert free > 0, "stream-order: no sync-free case was recorded: the harness tested nothing"
    assert share <= cap, ("stream-order: %d of %d sync-free cases uncovered (%.1f %% > %.1f %%): their delay ended before "
                          "the host had enqueued the op" % (unc, free, 100.0 * share, 100.0 * cap))
    return unc, free, share


# ---- the delay -----------------------------------------------------------------------------------------------------
_cycles_per_ms = {}


def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond on the current device, measured once with events"""
    dev = torch.cuda.current_device()
    if dev not in _cycles_per_ms:
        def timed(cycles):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(int(cycles))
            b.record()
            b.synchronize()
            return a.elapsed_time(b)
        timed(1000)                                           # the kernel's first launch is not timed
        cycles, ms = 100000, 0.0
        for _ in range(6):                                    # grow until the launch itself no longer shows: >= 2 ms
            ms = timed(cycles)
            if ms >= 2.0:
                break
            cycles *= 8
        assert ms > 0.0
        _cycles_per_ms[dev] = cycles / ms
    return _cycles_per_ms[dev]


def delay_ms_for(host_ms):
    return max(MIN_DELAY_MS, DELAY_FACTOR * host_ms)


def _sleep_ms(ms):
    torch.cuda._sleep(int(ms * cycles_per_ms()))


# ---- results -------------------------------------------------------------------------------------------------------
def clone_result(x):
    """the result with every tensor cloned on the current stream (arrays and plain values as they are)"""
    if isinstance(x, torch.Tensor):
        return x.detach().clone(memory_format=torch.preserve_format)
    if isinstance(x, dict):
        return {k: clone_result(v) for k, v in x.items()}
    if isinstance(x, list):
        return [clone_result(v) for v in x]
    if isinstance(x, tuple):
        return tuple(clone_result(v) for v in x)
    return x


def run_case(fn, inputs, name="case", decoy=None, defined=None, flags_raised=None, sync_free=True, vacuous_ok=False,
             totals=None, records=None):
    """The four steps of the module docstring for one op.  ``inputs`` is a dict or a sequence whose tensors are the op's
    inputs; ``defined`` maps a result to its defined part; ``flags_raised()`` reads and clears the device flags;
    ``sync_free`` says whether the op is free of host synchronisation (it decides whether the case can count as
    uncovered); ``vacuous_ok`` waives the vacuity floor for an op that has no device input or whose result does not
    depend on its values (the caller lists those with a reason).  Raises StreamOrderViolation / VacuousDecoy."""
    cut = defined if defined is not None else (lambda r: r)
    tens = ga._tensors(inputs)
    keep = {k: v.detach().clone(memory_format=torch.preserve_format) for k, v in tens}
    decoy_inputs = (decoy or default_decoy)(inputs)

    def flag(tag):
        if flags_raised is not None and flags_raised():
            raise StreamOrderViolation("stream-order %s %s: a device flag was raised" % (name, tag))

    def intact(tag, ins):
        for k, v in ga._tensors(ins):
            d = ga.bit_differences(keep[k], v, "input %r" % (k,))
            if d:
                raise StreamOrderViolation("stream-order %s %s: the op's inputs changed: %s" % (name, tag, "; ".join(d)))

    # 1. baseline
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    base = fn(inputs)
    base_host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    base_flat = ga._flatten(cut(base), "result", [])
    flag("baseline")
    intact("baseline", inputs)

    # 2. decoy baseline and the vacuity floor
    dec = fn(decoy_inputs)
    torch.cuda.synchronize()
    dec_flat = ga._flatten(cut(dec), "result", [])
    flag_up = bool(flags_raised()) if flags_raised is not None else False
    vacuous = False
    try:
        check_vacuity(name, base_flat, dec_flat, flag_up)
    except VacuousDecoy:
        if not vacuous_ok or flag_up:
            raise
        vacuous = True
    del dec

    def compare(tag, got):
        d = ga._diff_flat(base_flat, ga._flatten(cut(got), "result", []), "result")
        if d:
            stale = not ga._diff_flat(dec_flat, ga._flatten(cut(got), "result", []), "result")
            raise StreamOrderViolation(
                "stream-order %s %s: the result on the side stream is not the baseline's%s: %s"
                % (name, tag, " (it is the decoy's: work ran before the inputs landed)" if stale else "", "; ".join(d)))

    delay = delay_ms_for(base_host_ms)
    S = torch.cuda.Stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def put(side, src):
        for k, v in ga._tensors(side):
            v.copy_(src[k])

    # 3. producer leg
    with torch.cuda.stream(S):
        side = _map_tensors(inputs, lambda _k, v: torch.empty_like(v))
        put(side, decoy_inputs)
        S.synchronize()
        ev0.record(S)
        _sleep_ms(delay)
        ev1.record(S)
        put(side, inputs)
        t0 = time.perf_counter()
        got = fn(side)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = clone_result(got)
        S.synchronize()
    delay_seen = ev0.elapsed_time(ev1)
    compare("producer leg", got)
    torch.cuda.synchronize()
    flag("producer leg")
    intact("producer leg", side)
    del got

    # 4. busy-default leg
    with torch.cuda.stream(S):
        put(side, decoy_inputs)
        scrub = fn(side)
        del scrub
        put(side, inputs)
    torch.cuda.synchronize()
    if flags_raised is not None:
        flags_raised()                                        # (the decoy's, read above as well: cleared)
    _sleep_ms(delay)                                          # on the default stream
    with torch.cuda.stream(S):
        got = clone_result(fn(side))
        S.synchronize()
    pending = not torch.cuda.default_stream().query()
    compare("busy-default leg", got)
    torch.cuda.synchronize()
    flag("busy-default leg")
    intact("busy-default leg", side)

    rec = dict(name=name, delay_ms=delay_seen, host_ms=host_ms, sync_free=bool(sync_free), vacuous=vacuous,
               default_pending=pending)
    print("stream-order %s delay_ms=%.2f host_ms=%.2f sync_free=%d uncovered=%d vacuous=%d default_delay_pending=%d ok"
          % (name, delay_seen, host_ms, sync_free, is_uncovered(rec), vacuous, pending))
    if records is not None:
        records.append(rec)
    if totals is not None:
        totals["cases"] = totals.get("cases", 0) + 1
        totals["vacuity_overrides"] = totals.get("vacuity_overrides", 0) + int(vacuous)
    return base


# ---- the host-synchronisation debugger -----------------------------------------------------------------------------
def synchronises(fn, inputs):
    """True when fn(inputs) makes torch synchronise the host (a read-back, a blocking upload, an .item()): run once
    under torch.cuda.set_sync_debug_mode('warn') after the caller's warm-up"""
    import warnings
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn(inputs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return any("synchroniz" in str(x.message).lower() for x in w)


def assert_sync_free(fn, inputs, name="case"):
    """fn(inputs) under torch.cuda.set_sync_debug_mode('error'), after the caller's warm-up"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fn(inputs)
    except RuntimeError as e:
        if "synchroniz" in str(e).lower():
            raise AssertionError("stream-order %s: the op synchronises the host and is not listed in SYNCS: %s" % (name, e))
        raise
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
