"""Which kernels a call launches is part of the contract of the per-function paths: the route depends on the lengths alone, never
on the sample format, and a host-side change must not move it.  Every case of tests/sample_routes.py makes its call once to
warm the context (plans and tables built at first use), then once more with the profiler on, and {launch name: launches} of that
one call must equal tests/golden/sample_routes_v1.json exactly (times are ignored).

The fixture is a recording of this very code:  TSDR_RECORD_SAMPLE_ROUTES=1 python -m pytest tests/test_sample_routes_gpu.py -m gpu
rewrites it (from the build under TSDR_HIP_LIB, if set)."""
import contextlib
import json
import os

import pytest

import sample_routes as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_routes_v1.json")
RECORD = os.environ.get("TSDR_RECORD_SAMPLE_ROUTES") == "1"
CASES = S.cases()
_RECORDED = {}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _launches(ctx, prepare):
    got = {}

    @contextlib.contextmanager
    def profiled():
        ctx.profile_reset()
        ctx.profile(True)
        try:
            yield
        finally:
            ctx.synchronize()
            got.update({k: v["launches"] for k, v in ctx.profile_results().items()})
            ctx.profile(False)
            ctx.profile_reset()
    S.run(ctx, prepare, profiled)
    return got


def test_case_ids_are_unique_and_the_fixture_lists_them_all():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids)
    if not RECORD:
        assert sorted(_golden()) == sorted(ids)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_launches_are_the_recorded_ones(ctx, case):
    name, prepare = case
    got = _launches(ctx, prepare)
    assert got, "the call launched nothing"
    if RECORD:
        _RECORDED[name] = got
        if len(_RECORDED) == len(CASES):
            with open(GOLDEN, "w") as f:
                json.dump(_RECORDED, f, indent=0, sort_keys=True)
                f.write("\n")
        return
    assert got == _golden()[name], name
