"""What the frame loop launches is what the image plan says: per route family one small geometry (the `gpu-*` cases of
tools/host_plan/plan_dump.h), run for two frames with profiling on; the image kernels' names and launch counts must equal the
steps on that case's line of tests/golden/image_plans_v1.txt -- the record test_image_plan_host.py holds the planner to."""
import numpy as np
import pytest

from test_dptr_gpu import profiled
from test_image_plan_host import PROFILE_NAMES, golden_lines, parse

pytestmark = pytest.mark.gpu

# case id -> (S, y_t, x_t, raster wanted, sums wanted (= do_align), precision, options)
CASES = {
    "gpu-walk-raster": (53248, 640, 832, True, True, "fast", {}),
    "gpu-taps-sums": (53248, 640, 832, False, True, "fast", {}),
    "gpu-taps": (53248, 640, 832, False, False, "fast", {}),
    "gpu-taps-ld16": (612352, 640, 832, False, True, "fast", {}),
    "gpu-walk-nonfused": (6000, 200, 300, True, True, "fast", {}),
    "gpu-direct": (40000, 20, 30, True, True, "fast", {}),
    "gpu-exact-raster": (53248, 640, 832, True, True, "exact", {}),
    "gpu-exact-taps": (53248, 640, 832, False, True, "exact", {}),
    "gpu-walk-only": (53248, 640, 832, False, True, "fast", {"fast_walk_only": 1}),
    "gpu-shear": (54080, 650, 832, True, True, "fast", {"raster_split": 1}),
    "gpu-fallback": (1000000, 20, 30, False, False, "fast", {}),
}
FRAMES = 2


def planned(cid):
    """{profile name: launches} of the case's line; the per-frame fallback pair counts once per frame"""
    (line,) = [x for x in golden_lines() if x.startswith(cid + " ")]
    _, head, steps = parse(line)
    assert head.startswith("status=0 ")
    per_frame = 2 if " fallback " in head + " " else 0
    want = {}
    for i, (name, _, _) in enumerate(steps):
        want[name] = want.get(name, 0) + (FRAMES if i >= len(steps) - per_frame else 1)
    return want


@pytest.mark.parametrize("cid", sorted(CASES))
def test_frame_loop_launches_the_planned_kernels(ctx, tsdr, cid):
    S, y_t, x_t, raster, align, precision, options = CASES[cid]
    rng = np.random.default_rng([20261, S, y_t])
    n = FRAMES * S
    iq = (rng.standard_normal(n, np.float32) + 1j * rng.standard_normal(n, np.float32)).astype(np.complex64)
    image = np.zeros((600, 800), np.float32, order="F")
    sync = tsdr.SyncXY(ctx, 600, 800) if align else None
    ctx.set_precision(precision)
    ctx.set_option("sync_guard_ppb", 0)   # (a guarded buffer may be moved to the exact sequence as a whole: another plan)
    for k, v in options.items():
        ctx.set_option(k, v)
    try:
        with profiled(ctx) as prof:
            out = ctx.frames(sync, iq, S, y_t, x_t, 0.5, image, do_align=align, want_frames=False, want_raster=raster)
            ran = prof.names()
    finally:
        for k in options:
            ctx.set_option(k, 0)
        ctx.set_precision("fast")
    assert out["n_frames"] == FRAMES
    assert {k: v for k, v in ran.items() if k in PROFILE_NAMES} == planned(cid), ran
    assert np.isfinite(image).all() and image.any()


def test_sig_to_image_launches_the_planned_kernel(ctx):
    rng = np.random.default_rng(20262)
    with profiled(ctx) as prof:
        img = ctx.sig_to_image(rng.standard_normal(6000, np.float32), 200, 300)
        ran = prof.names()
    assert {k: v for k, v in ran.items() if k in PROFILE_NAMES} == planned("gpu-real-tile") == {"raster_f32_exact": 1}
    assert img.shape == (200, 300) and np.isfinite(img).all()
