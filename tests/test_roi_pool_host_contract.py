"""The host side of the RoI-pool exports, without a GPU: the status codes of calls that are rejected (or are a no-op)
before any launch, and the pure host rules and size queries over a grid of launch shapes, against the answers
recorded in tests/golden/roi_pool_host_contract.json (tests/golden/make_golden_roi_pool_host_contract.py lists the
cases and wrote the fixture).  The launch and dispatch code may be reorganised freely; these answers may not move."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_golden_roi_pool_host_contract as contract  # noqa: E402


@pytest.fixture(scope="module")
def answers():
    from wssdl_bus_amd import _lib, build
    build.build(verbose=False)
    with open(os.path.join(GOLDEN, "roi_pool_host_contract.json")) as f:
        want = json.load(f)
    return contract.record(_lib), want


def test_case_list_covers_every_pointer_taking_export():
    from wssdl_bus_amd import _lib
    pointer_taking = sorted(n for n, (_, args) in _lib.SYMBOLS.items()
                            if ("roi_pool" in n or "roi_argmax" in n) and _lib._vp in args)
    assert sorted(contract.EXPORTS) == pointer_taking


def test_status_codes_of_calls_that_never_launch(answers):
    got, want = answers
    assert sorted(got["status"]) == sorted(want["status"])
    wrong = {k: (got["status"][k], want["status"][k]) for k in want["status"] if got["status"][k] != want["status"][k]}
    assert not wrong, wrong
    # the fixture is not vacuous: every status the checks can give appears, and so does a no-op OK
    from wssdl_bus_amd import _lib
    codes = set(v if isinstance(v, int) else v[0] for v in want["status"].values())
    assert codes == {_lib.OK, _lib.ERR_INVALID_ARGUMENT, _lib.ERR_WORKSPACE}


@pytest.mark.parametrize("part", ["rules", "tuned"])
def test_host_rules_and_sizes_over_the_grid(answers, part):
    got, want = answers
    assert sorted(got[part]) == sorted(want[part])
    for name in sorted(want[part]):
        assert got[part][name] == want[part][name], name
    # knobs are back at their defaults
    from wssdl_bus_amd import _lib
    assert _lib.get_tuning("roi_bwd_owner") == -1 and _lib.get_tuning("roi_fwd_blocks") == -1
