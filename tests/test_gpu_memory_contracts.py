"""-m gpu: the memory contracts of the device ops -- guard bands and poison (tests/guarded_alloc.py).

Every case of the shared table (tests/device_op_cases.py) is a small callable built from inputs the suite already has.
guarded_alloc.run_case runs it once on the plain allocator (the baseline) and once per poison byte with every
torch.empty / empty_like / zeros / new_empty of the Python layer guarded by 64 KiB of 0xA5 on both sides, and asserts:
the guards are intact, the inputs are untouched (except where the op's contract says it works in place), every DEFINED
result has the baseline's bits under every poison, no device flag is up, and at least the declared number of
allocations was guarded.

Regions a contract leaves undefined are excluded through the one table UNDEFINED of the case module and nowhere else;
each entry quotes the sentence of include/wssdl_bus_hip.h or of the wrapper's docstring that leaves the region undefined.

No kernel is changed, built differently or made to read garbage here: the seeded defects that prove the harness live in
tests/test_guarded_alloc_cpu.py, on CPU tensors."""
import pytest
import torch

import guarded_alloc as ga
from device_op_cases import (CASES, DEV, N_MEMORY_CONTRACT_CASES, N_STREAM_ORDER_ADDED, OWNER_PLANS, UNDEFINED, _defined_for,
                             _flags)

pytestmark = pytest.mark.gpu

TOTALS = {}

assert N_MEMORY_CONTRACT_CASES == 407 and len(CASES) == 407 + N_STREAM_ORDER_ADDED == 424, len(CASES)


@pytest.fixture(scope="module", autouse=True)
def _totals():
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    _lib.lib()
    yield
    print("\nmemcheck totals: cases=%d runs=%d allocations=%d guarded_bytes=%d len(UNDEFINED)=%d"
          % (TOTALS.get("cases", 0), TOTALS.get("runs", 0), TOTALS.get("allocations", 0), TOTALS.get("guarded_bytes", 0),
             len(UNDEFINED)))


@pytest.mark.parametrize("name", list(CASES))
def test_memory_contract(name):
    builder, floor = CASES[name]
    spec = builder()
    flags = _flags() if spec.get("flags", True) else None
    if flags is not None:
        flags()                                     # cleared: what this case raises is this case's
    try:
        ga.run_case(spec["fn"], spec["inputs"], name=name, min_allocations=floor, inplace=spec.get("inplace", ()),
                    defined=_defined_for(name), flags_raised=flags, totals=TOTALS)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("memcheck %s: the device faulted (%s); nothing more is started on it" % (name, e), returncode=3)
        raise
    TOTALS["cases"] = TOTALS.get("cases", 0) + 1


def test_a_device_allocation_passed_through_unguarded_is_still_poisoned():
    """a layout keyword sends the call to the allocator as it stands: no guard bands, the poison byte in every byte"""
    with ga.guarded(0x7F) as reg:
        t = torch.empty((2, 3, 5, 7), device=DEV, memory_format=torch.channels_last)
        u = torch.empty((11,), dtype=torch.int32, device=DEV)
    assert reg.count() == 1 and reg.passed_through == 1
    assert t.is_contiguous(memory_format=torch.channels_last) and t.untyped_storage().nbytes() < 2 * ga.GUARD
    assert bool((t.view(torch.int32) == 0x7F7F7F7F).all()) and bool((u == 0x7F7F7F7F).all())
    print("memcheck pass-through poison=0x7F guarded=%d passed_through=%d ok" % (reg.count(), reg.passed_through))


def test_every_owner_plan_has_its_cases():
    from wssdl_bus_amd import _lib
    assert _lib.lib().wssdl_roi_pool_backward_owner_plan_count() == OWNER_PLANS


def test_undefined_table_is_backed_by_the_contract():
    """every excluded region quotes a sentence that stands, verbatim, in the header or in a wrapper's docstring"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    texts = []
    for top, _dirs, files in os.walk(os.path.join(root, "wssdl_bus_amd")):
        texts += [open(os.path.join(top, f)).read() for f in files if f.endswith(".py")]
    texts.append(open(os.path.join(root, "include", "wssdl_bus_hip.h")).read())
    flat = [" ".join(t.replace("*", " ").replace("#", " ").split()) for t in texts]
    for prefixes, region, sentence, _cut in UNDEFINED:
        assert all(any(n.startswith(p) for n in CASES) for p in prefixes), prefixes
        assert any(" ".join(sentence.split()) in t for t in flat), (prefixes, region, sentence)
    assert len(UNDEFINED) <= 12
