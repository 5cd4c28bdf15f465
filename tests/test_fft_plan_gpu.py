"""What a transform launches is what the FFT plan says: per kind of step one small call (the `gpu-*` cases of
tools/host_plan/fft_plan_dump.h), made once to warm the context (tables are built at first use), then once with profiling on;
the pass kernels' names and launch counts must equal the steps on that case's line of tests/golden/fft_plans_v1.txt -- the
record test_fft_plan_host.py holds the planner to."""
import numpy as np
import pytest

from test_dptr_gpu import profiled
from test_fft_plan_host import PROFILE_NAMES, golden_lines, parse

pytestmark = pytest.mark.gpu


def _c64(rng, *shape):
    return (rng.standard_normal(shape, np.float32) + 1j * rng.standard_normal(shape, np.float32)).astype(np.complex64)


def _fft(n, batch=1, inverse=False):
    def call(ctx, rng):
        return ctx.fft(_c64(rng, batch, n) if batch > 1 else _c64(rng, n), inverse=inverse)
    return call


def _autocorr(n, min_delay):
    def call(ctx, rng):
        return ctx.calculate_autocorrelation(rng.standard_normal(n, np.float32), 1.0, float(min_delay), float(n // 2))[0]
    return call


# case id -> the call that takes that plan
CASES = {
    "gpu-pow2-rows": _fft(64, 5),
    "gpu-pow2-two-pass": _fft(512),
    "gpu-pow2-three-pass": _fft(1 << 17, inverse=True),
    "gpu-generic-one-pass": _fft(100, 4),
    "gpu-generic-last": _fft(300, 4),
    "gpu-two-step": _fft(6000),
    "gpu-three-step": _fft(80000),
    "gpu-mid-two-step": _autocorr(10000, 100),
    "gpu-mid-three-step": _autocorr(180000, 1000),
    "gpu-rows-store": _fft(1000, 7),
    "gpu-rows-welch": lambda ctx, rng: ctx.getWelch(1.0, _c64(rng, 7 * 2000), 2000)[1],
    "gpu-rows-welch-generic": lambda ctx, rng: ctx.getWelch(1.0, _c64(rng, 7 * 960), 960)[1],
    "gpu-rows-waterfall": lambda ctx, rng: ctx.getWaterfall(1.0, _c64(rng, 7 * 500), 500)[2],
}


def planned(cid):
    """{profile name: launches} of the case's line"""
    (line,) = [x for x in golden_lines() if x.startswith(cid + " ")]
    _, head, steps = parse(line)
    assert head.startswith("status=0 ") and steps
    want = {}
    for name, *_ in steps:
        want[name] = want.get(name, 0) + 1
    return want


@pytest.mark.parametrize("cid", sorted(CASES))
def test_the_call_launches_the_planned_steps(ctx, cid):
    call = CASES[cid]
    call(ctx, np.random.default_rng(20263))
    with profiled(ctx) as prof:
        out = call(ctx, np.random.default_rng(20263))
        ran = prof.names()
    assert {k: v for k, v in ran.items() if k in PROFILE_NAMES} == planned(cid), ran
    out = np.asarray(out)
    assert np.isfinite(out.view(np.float32) if np.iscomplexobj(out) else out).all() and out.any()
