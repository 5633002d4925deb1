"""Guard-band and poison harness for the memory contracts of the device ops.

A value test reads only the bytes an op is meant to produce.  This module makes two other
kinds of mistake visible:

* a write outside a caller-sized buffer (a workspace, a table, an output), which the caching
  allocator otherwise hides in rounding slack or in a neighbouring tensor;
* a read of memory nobody wrote, which in a fresh pytest process mostly reads zeros.

``guarded(poison)`` replaces ``torch.empty``, ``torch.empty_like``, ``torch.zeros`` and
``Tensor.new_empty`` while it is active.  A dense allocation of ``nbytes > 0`` on a guarded
device type becomes a view into a ``uint8`` buffer laid out as ``GUARD + nbytes + GUARD``: the
view starts at byte ``GUARD`` (256-byte alignment is kept) and ends at exactly ``nbytes`` (the
size is not rounded, the first byte after the tensor is guard).  Guards hold ``0xA5``; the
interior holds the poison byte for ``empty*`` and zeros for ``zeros``.

Passed through unguarded: ``device="meta"``, CPU or pinned memory (unless the CPU is named as
a guarded device type, which is how the harness is proved on fake ops), zero-size requests and
every call with a ``memory_format`` or another layout keyword.  A CUDA allocation among them
is still poisoned.

``run_case`` runs one op once with the plain allocator and once per poison under ``guarded``
and asserts the four properties in its docstring.

What this cannot see: an overrun of more than ``GUARD`` bytes, memory that is not allocated
through the four patched calls (``clone``, ``zeros_like``, ``new_zeros``, ``full``, results of
torch operators), and graph-captured runs.
"""
import contextlib
import os
import sys

import numpy as np
import torch

GUARD = 65536
GUARD_BYTE = 0xA5
# zero first: "fresh memory".  0xFF: NaN as f32/f64, -1 as i32, the maximum as u64.
# 0x7F7F7F7F = +3.39e38 and 0xFEFEFEFE = -1.69e38: finite, because max/min reductions built on
# v_max/v_min skip NaN and NaN poison alone would pass a stale read in them.
POISONS = (0x00, 0xFF, 0x7F, 0xFE)

_THIS_FILE = os.path.abspath(__file__).replace(".pyc", ".py")
_PLAIN_KW = frozenset(("dtype", "device", "requires_grad"))


class GuardViolation(AssertionError):
    pass


class _Record(object):
    __slots__ = ("buf", "nbytes", "site")

    def __init__(self, buf, nbytes, site):
        self.buf, self.nbytes, self.site = buf, nbytes, site


def _call_site():
    """file:line of the nearest frame outside this module."""
    f = sys._getframe(1)
    while f is not None:
        fn = os.path.abspath(f.f_code.co_filename)
        if fn != _THIS_FILE:
            return "%s:%d" % (f.f_code.co_filename, f.f_lineno)
        f = f.f_back
    return "<unknown>:0"


def _size_of(args):
    """The size arguments of empty/zeros/new_empty as a tuple of ints, or None when they are
    not plain ints (symbolic sizes, tensors): such a call is passed through."""
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    out = []
    for a in args:
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)):
            return None
        out.append(int(a))
    return tuple(out)


class Registry(object):
    """Every guarded allocation of one ``guarded`` block."""

    def __init__(self, poison, devices):
        self.poison = int(poison)
        self.devices = tuple(devices)
        self.records = []
        self.passed_through = 0
        self._orig = {}

    # ---- allocation -----------------------------------------------------------------
    def _fill_storage(self, t, byte):
        st = t.untyped_storage()
        if st.nbytes() > 0:
            torch.tensor([], dtype=torch.uint8, device=t.device).set_(st).fill_(byte)

    def _alloc(self, kind, orig, args, kwargs, size, dtype, device, interior):
        """Guarded allocation when the request is plain, else the original call (poisoned when
        it lands on a guarded CUDA device)."""
        plain = size is not None
        nbytes = 0
        if plain:
            n = 1
            for s in size:
                n *= s
            nbytes = n * dtype.itemsize if n > 0 else 0
        if not plain or nbytes <= 0 or device.type not in self.devices:
            t = orig(*args, **kwargs)
            self.passed_through += 1
            if t.device.type == "cuda" and t.layout == torch.strided and interior is not None \
                    and kind != "zeros" and t.numel() > 0:
                self._fill_storage(t, interior)
            return t
        empty = self._orig["empty"]
        buf = empty((GUARD + nbytes + GUARD,), dtype=torch.uint8, device=device)
        buf[:GUARD].fill_(GUARD_BYTE)
        buf[GUARD:GUARD + nbytes].fill_(0 if kind == "zeros" else interior)
        buf[GUARD + nbytes:].fill_(GUARD_BYTE)
        self.records.append(_Record(buf, nbytes, _call_site()))
        t = buf[GUARD:GUARD + nbytes].view(dtype).view(size)
        if kwargs.get("requires_grad", False):
            t.requires_grad_(True)
        return t

    @staticmethod
    def _device(dev, like=None):
        if dev is None:
            if like is not None:
                return like.device
            get = getattr(torch, "get_default_device", None)
            return get() if get is not None else torch.device("cpu")
        if isinstance(dev, int):
            return torch.device("cuda", dev)
        d = torch.device(dev)
        if d.type == "cuda" and d.index is None and torch.cuda.is_available():
            d = torch.device("cuda", torch.cuda.current_device())
        return d

    def _empty(self, *args, **kwargs):
        return self._factory("empty", args, kwargs)

    def _zeros(self, *args, **kwargs):
        return self._factory("zeros", args, kwargs)

    def _factory(self, kind, args, kwargs):
        kw = dict(kwargs)
        size_args = (kw.pop("size"),) if ("size" in kw and not args) else args
        size = _size_of(size_args) if set(kw) <= _PLAIN_KW else None
        dtype = kw.get("dtype") or torch.get_default_dtype()
        return self._alloc(kind, self._orig[kind], args, kwargs, size, dtype, self._device(kw.get("device")),
                           self.poison)

    def _empty_like(self, x, *args, **kwargs):
        orig = self._orig["empty_like"]
        dense = isinstance(x, torch.Tensor) and x.layout == torch.strided and x.is_contiguous()
        if args or not dense or not set(kwargs) <= _PLAIN_KW:
            return self._alloc("empty_like", orig, (x,) + args, kwargs, None, None,
                               x.device if isinstance(x, torch.Tensor) else torch.device("cpu"), self.poison)
        dtype = kwargs.get("dtype") or x.dtype
        device = self._device(kwargs.get("device"), like=x)
        return self._alloc("empty_like", orig, (x,), kwargs, tuple(x.shape), dtype, device, self.poison)

    def _new_empty(self, x, *args, **kwargs):
        orig = self._orig["new_empty"]
        if "size" in kwargs and not args:
            args, kwargs = (kwargs["size"],), {k: v for k, v in kwargs.items() if k != "size"}
        size = _size_of(args) if (x.layout == torch.strided and set(kwargs) <= _PLAIN_KW) else None
        dtype = kwargs.get("dtype") or x.dtype
        device = self._device(kwargs.get("device"), like=x)
        return self._alloc("new_empty", orig, (x,) + tuple(args), kwargs, size, dtype, device, self.poison)

    # ---- patching -------------------------------------------------------------------
    def install(self):
        self._orig = {"empty": torch.empty, "zeros": torch.zeros, "empty_like": torch.empty_like,
                      "new_empty": torch.Tensor.new_empty}
        torch.empty, torch.zeros, torch.empty_like = self._empty, self._zeros, self._empty_like
        reg = self
        torch.Tensor.new_empty = lambda x, *a, **k: reg._new_empty(x, *a, **k)

    def uninstall(self):
        torch.empty, torch.zeros = self._orig["empty"], self._orig["zeros"]
        torch.empty_like = self._orig["empty_like"]
        torch.Tensor.new_empty = self._orig["new_empty"]

    # ---- the log line ---------------------------------------------------------------
    def count(self):
        return len(self.records)

    def guarded_bytes(self):
        return sum(r.nbytes for r in self.records)

    # ---- the check ------------------------------------------------------------------
    def violations(self):
        """[(site, side, lowest offset, highest offset, nbytes of that allocation)]; offsets are
        relative to the tensor's first byte, so 'before' offsets are negative and 'after' offsets
        start at nbytes."""
        if any(r.buf.is_cuda for r in self.records):
            torch.cuda.synchronize()
        if not self.records:
            return []
        flags = []
        for r in self.records:
            flags.append((r.buf[:GUARD] != GUARD_BYTE).any())
            flags.append((r.buf[GUARD + r.nbytes:] != GUARD_BYTE).any())
        by_dev = {}
        for i, f in enumerate(flags):
            by_dev.setdefault(f.device, []).append((i, f))
        hit = []
        for dev, lst in by_dev.items():
            got = torch.stack([f for _, f in lst]).cpu().numpy()
            hit += [i for (i, _), g in zip(lst, got) if g]
        out = []
        for i in sorted(hit):
            r, after = self.records[i // 2], i % 2
            g = r.buf[GUARD + r.nbytes:] if after else r.buf[:GUARD]
            idx = (g != GUARD_BYTE).nonzero().flatten().cpu().numpy()
            base = r.nbytes if after else -GUARD
            out.append((r.site, "after" if after else "before", base + int(idx.min()), base + int(idx.max()), r.nbytes))
        return out

    def check(self):
        v = self.violations()
        if v:
            raise GuardViolation("; ".join(_violation_text(x) for x in v))


def _violation_text(v):
    site, side, lo, hi, nbytes = v
    return "guard %s the %d-byte allocation of %s overwritten at offsets %d..%d" % (side, nbytes, site, lo, hi)


@contextlib.contextmanager
def guarded(poison, devices=("cuda",)):
    """Replace the four allocation calls; yields the Registry.  ``devices`` names the device
    types that are guarded: the product tests keep the default, the CPU self-test of the
    harness passes ("cpu",)."""
    reg = Registry(poison, devices)
    reg.install()
    try:
        yield reg
    finally:
        reg.uninstall()


# ---- result comparison ---------------------------------------------------------------
def _flatten(x, path, out):
    if isinstance(x, torch.Tensor):
        t = x.detach()
        if t.is_cuda:
            t = t.cpu()
        t = t.contiguous()
        raw = t.reshape(-1).view(torch.uint8).numpy().copy() if t.numel() else np.zeros(0, np.uint8)
        out.append((path, (str(t.dtype), tuple(t.shape)), raw))
    elif isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        out.append((path, (str(a.dtype), a.shape), a.reshape(-1).view(np.uint8).copy() if a.size else np.zeros(0, np.uint8)))
    elif isinstance(x, dict):
        for k in sorted(x, key=str):
            _flatten(x[k], "%s[%r]" % (path, k), out)
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            _flatten(v, "%s[%d]" % (path, i), out)
    elif isinstance(x, (float, np.floating)):
        out.append((path, ("float", ()), np.array([x], np.float64).view(np.uint8)))
    elif x is None or isinstance(x, (int, bool, str, np.integer, np.bool_)):
        out.append((path, (type(x).__name__, ()), np.frombuffer(repr(x).encode(), np.uint8)))
    else:
        raise TypeError("run_case: result %s of type %s cannot be compared" % (path, type(x)))
    return out


def _diff_flat(fa, fb, what):
    if [p for p, _, _ in fa] != [p for p, _, _ in fb]:
        return ["%s: structure differs" % what]
    msgs = []
    for (p, ma, ra), (_, mb, rb) in zip(fa, fb):
        if ma != mb or ra.shape != rb.shape:
            msgs.append("%s: %s vs %s" % (p, ma, mb))
        elif not np.array_equal(ra, rb):
            d = np.flatnonzero(ra != rb)
            msgs.append("%s %s: %d bytes differ, first at byte %d, last at byte %d"
                        % (p, ma, d.size, int(d[0]), int(d[-1])))
    return msgs


def bit_differences(a, b, what="result"):
    """Messages for every leaf of two nested results that is not bit-identical (floats are
    compared as bytes, so NaN equals NaN)."""
    return _diff_flat(_flatten(a, what, []), _flatten(b, what, []), what)


def _tensors(inputs):
    items = inputs.items() if isinstance(inputs, dict) else enumerate(inputs)
    return [(k, v) for k, v in items if isinstance(v, torch.Tensor)]


def run_case(fn, inputs, name="case", min_allocations=1, inplace=(), defined=None,
             flags_raised=None, poisons=POISONS, devices=("cuda",), totals=None):
    """Run ``fn(inputs)`` once with the plain allocator (the baseline) and once per poison
    under ``guarded``.  ``inputs`` is a dict or a sequence; its tensors are the op's inputs.

    Asserts, per poison:
      1. every guard band is intact;
      2. every input is bit-identical to the clone taken before the first run, except the keys
         in ``inplace`` (ops whose contract says they work in place; those are restored from
         the clone before each run);
      3. every defined result is bit-identical to the baseline (``defined`` maps a result to
         its defined part; the only callers of it are the entries of the test module's
         ``UNDEFINED`` table);
      4. ``flags_raised()`` is false, where one is given.
    A run under which fewer than ``min_allocations`` (at least 1) allocations were guarded
    fails: a case that guards nothing tests nothing.
    Returns the baseline result."""
    assert min_allocations >= 1, "the vacuity floor is at least 1"
    tens = _tensors(inputs)
    clones = {k: v.detach().clone() for k, v in tens}

    def restore():
        for k, v in tens:
            if k in inplace:
                with torch.no_grad():
                    v.copy_(clones[k])

    def inputs_intact(tag):
        for k, v in tens:
            if k in inplace:
                continue
            d = bit_differences(clones[k], v, "input %r" % (k,))
            assert not d, "memcheck %s %s: the op wrote to an input: %s" % (name, tag, "; ".join(d))

    cut = defined if defined is not None else (lambda r: r)
    restore()
    base = fn(inputs)
    base_cut = _flatten(cut(base), "result", [])
    inputs_intact("baseline")
    for poison in poisons:
        restore()
        with guarded(poison, devices) as reg:
            got = fn(inputs)
            got_cut = cut(got)
            if any(r.buf.is_cuda for r in reg.records):
                torch.cuda.synchronize()
        tag = "poison=0x%02X" % poison
        v = reg.violations()
        assert not v, "memcheck %s %s: %s" % (name, tag, "; ".join(_violation_text(x) for x in v))
        inputs_intact(tag)
        d = _diff_flat(base_cut, _flatten(got_cut, "result", []), "result")
        assert not d, ("memcheck %s %s: the result depends on what the allocations held: %s; allocations of this "
                       "run: %s" % (name, tag, "; ".join(d), ", ".join(sorted(set(r.site for r in reg.records)))))
        if flags_raised is not None:
            assert not flags_raised(), "memcheck %s %s: a device flag was raised" % (name, tag)
        assert reg.count() >= min_allocations, (
            "memcheck %s %s: %d allocations guarded, the case declares at least %d"
            % (name, tag, reg.count(), min_allocations))
        print("memcheck %s %s allocations=%d guarded_bytes=%d ok" % (name, tag, reg.count(), reg.guarded_bytes()))
        if totals is not None:
            totals["allocations"] = totals.get("allocations", 0) + reg.count()
            totals["guarded_bytes"] = totals.get("guarded_bytes", 0) + reg.guarded_bytes()
            totals["runs"] = totals.get("runs", 0) + 1
    return base
