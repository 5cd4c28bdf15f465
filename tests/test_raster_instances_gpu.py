"""Every class of k_raster_fast instantiation that resample.hip builds (image_plan.h:fast_instance) runs and computes what the
oracle computes: per class one small geometry (the `gpu-inst-*` cases of tools/host_plan/plan_dump.h), two frames each.  The
case's line of tests/golden/image_plans_v1.txt names the instantiation -- test_image_plan_host.py holds the planner to that
record, so the kernel text there is the statement that the class was reached -- and here the frame loop must launch the steps of
that line and agree with the oracle at test_fast_mode_gpu's tolerance.  A launcher that lacked one of these kernels would
answer TSDR_EINVAL (an AssertionError from the binding).

What this does not show: the profile holds the kernel family's name (raster_iq, raster_down_iq, down_walk_iq), not the
instantiation.  That the tile width, the wavefront count and the format were the intended ones rests on the record's line and on
the launcher's one-to-one dispatch from a step's arguments (resample.hip:launch_fast); the comparison with the oracle is
independent of both.

  gpu-inst-ras-pw*          the raster-only walk (no in-walk downgrade) at each tile width, 4 .. 128 pixels; -vw1: a raster lower
                            than 128 lines (one wavefront per column of the workgroup); -w64: more than 128 strips (64-bit advance)
  gpu-inst-rec4-pw*-ras|nor the f32-sample walk with the downgrade at 32, 64, 128 pixels, with and without a raster to write;
                            -sc16 / -sc8 / -uc8: the same kernel per integer input format
  gpu-inst-rec-pw32-ras|nor the record walk with the downgrade (option "raster_rec4" 0)"""
import importlib

import numpy as np
import pytest

import iq8_ref as R
import oracle_lib as O
from sync_margin import fast_vs_oracle
from test_dptr_gpu import profiled
from test_fast_mode_gpu import RTOL
from test_image_plan_gpu import FRAMES, planned
from test_image_plan_host import PROFILE_NAMES, golden_lines, parse

pytestmark = pytest.mark.gpu

WALK_ONLY, REC = {"fast_walk_only": 1}, {"raster_rec4": 0}
# case id -> (S, y_t, x_t, raster wanted, input format, options)
CASES = {
    "gpu-inst-ras-pw1": (600000, 200, 300, True, "cf32", {}),
    "gpu-inst-ras-pw2": (240000, 200, 300, True, "cf32", {}),
    "gpu-inst-ras-pw4": (120000, 200, 300, True, "cf32", {}),
    "gpu-inst-ras-pw8": (66000, 200, 300, True, "cf32", {}),
    "gpu-inst-ras-pw16": (30000, 200, 300, True, "cf32", {}),
    "gpu-inst-ras-pw32": (12000, 200, 300, True, "cf32", {}),
    "gpu-inst-ras-pw32-vw1": (3000, 100, 300, True, "cf32", {}),
    "gpu-inst-ras-pw1-w64": (676000, 130, 520, True, "cf32", {}),
    "gpu-inst-rec4-pw8-ras": (1331200, 640, 832, True, "cf32", {}),
    "gpu-inst-rec4-pw8-nor": (1331200, 640, 832, False, "cf32", {}),
    "gpu-inst-rec4-pw16-ras": (612352, 640, 832, True, "cf32", {}),
    "gpu-inst-rec4-pw16-nor": (612352, 640, 832, False, "cf32", WALK_ONLY),
    "gpu-inst-rec4-pw32-ras": (266240, 640, 832, True, "cf32", {}),
    "gpu-inst-rec4-pw32-nor": (266240, 640, 832, False, "cf32", WALK_ONLY),
    "gpu-inst-rec4-pw32-ras-sc16": (266240, 640, 832, True, "sc16", {}),
    "gpu-inst-rec4-pw32-ras-sc8": (266240, 640, 832, True, "sc8", {}),
    "gpu-inst-rec4-pw32-ras-uc8": (266240, 640, 832, True, "uc8", {}),
    "gpu-inst-rec-pw32-ras": (53248, 640, 832, True, "cf32", REC),
    "gpu-inst-rec-pw32-nor": (53248, 640, 832, False, "cf32", {**REC, **WALK_ONLY}),
}
# the template arguments each case is there for: (f32w, down, pw, out, vw, rec4, iqf)
ARGS = {
    "gpu-inst-ras-pw1": "true,false,1,true,2,false,2", "gpu-inst-ras-pw2": "true,false,2,true,2,false,2",
    "gpu-inst-ras-pw4": "true,false,4,true,2,false,2", "gpu-inst-ras-pw8": "true,false,8,true,2,false,2",
    "gpu-inst-ras-pw16": "true,false,16,true,2,false,2", "gpu-inst-ras-pw32": "true,false,32,true,2,false,2",
    "gpu-inst-ras-pw32-vw1": "true,false,32,true,1,false,2",
    "gpu-inst-ras-pw1-w64": "false,false,1,true,2,false,2",
    "gpu-inst-rec4-pw8-ras": "true,true,8,true,2,true,0", "gpu-inst-rec4-pw8-nor": "true,true,8,false,2,true,0",
    "gpu-inst-rec4-pw16-ras": "true,true,16,true,2,true,0", "gpu-inst-rec4-pw16-nor": "true,true,16,false,2,true,0",
    "gpu-inst-rec4-pw32-ras": "true,true,32,true,2,true,0", "gpu-inst-rec4-pw32-nor": "true,true,32,false,2,true,0",
    "gpu-inst-rec4-pw32-ras-sc16": "true,true,32,true,2,true,1", "gpu-inst-rec4-pw32-ras-sc8": "true,true,32,true,2,true,3",
    "gpu-inst-rec4-pw32-ras-uc8": "true,true,32,true,2,true,4",
    "gpu-inst-rec-pw32-ras": "true,true,32,true,2,false,2", "gpu-inst-rec-pw32-nor": "true,true,32,false,2,false,2",
}


class IntegerIq:
    """a Context whose frames() feeds the frame loop the raw integer samples `q` (tsdr_frames_iq_d) in place of their expansion,
    so that sync_margin.fast_vs_oracle -- which hands both sides complex64 -- compares the integer loaders with the oracle"""

    def __init__(self, ctx, q, fmt, scale):
        self._ctx, self._q, self._fmt, self._scale = ctx, q, fmt, scale

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def frames(self, sync, iq, S, y_t, x_t, alpha, imageOut, do_align=True, want_frames=True, want_raster=False):
        api = importlib.import_module("tempestsdr_jl_amd.api")
        ctx, nb, npx, P = self._ctx, self._q.size // 2 // S, imageOut.size, y_t * x_t
        assert np.array_equal(np.asarray(iq), R.expand(self._q, self._fmt, self._scale))
        d_in, d_state = ctx.upload(self._q), ctx.upload(imageOut.reshape(-1, order="F"))
        d_fr, d_ix = ctx.dev_alloc(nb * npx * 4), ctx.dev_alloc(nb * 8)
        d_ra = ctx.dev_alloc(nb * P * 4) if want_raster else None
        try:
            n = api.frames_iq_d(ctx, sync, d_in, self._fmt, self._scale, nb * S, S, y_t, x_t, alpha, do_align, d_state, d_fr, d_ra, d_ix)
            ctx.synchronize()
            out = {"n_frames": n, "sync_idx": ctx.download(d_ix, (nb, 2), np.int32)}
            fr = ctx.download(d_fr, (nb, npx), np.float32)
            out["frames"] = [fr[f].reshape(imageOut.shape, order="F") for f in range(nb)]
            if want_raster:
                ra = ctx.download(d_ra, (nb, P), np.float32)
                out["raster"] = [ra[f].reshape((y_t, x_t), order="F") for f in range(nb)]
            imageOut[...] = ctx.download(d_state, (npx,), np.float32).reshape(imageOut.shape, order="F")
        finally:
            for p in (d_in, d_state, d_fr, d_ix, d_ra):
                if p is not None:
                    ctx.dev_free(p)
        return out


def test_the_cases_name_their_classes():
    """(no GPU work) the record's line of each case holds the instantiation the case is there for"""
    assert set(CASES) == set(ARGS) == {parse(x)[0] for x in golden_lines() if x.startswith("gpu-inst-")}
    for cid, args in ARGS.items():
        (line,) = [x for x in golden_lines() if x.startswith(cid + " ")]
        assert parse(line)[2][0][1] == f"k_raster_fast<true,{args}>", line


@pytest.mark.parametrize("cid", sorted(CASES))
def test_each_class_runs_as_planned_and_agrees_with_the_oracle(ctx, tsdr, synth, cid):
    S, y_t, x_t, raster, fmt, options = CASES[cid]
    z = synth.synth_leak(50.0 * S, x_t, y_t, 50.0, FRAMES * S)
    run = ctx
    if fmt != "cf32":
        q, scale = R.quantise(z, fmt)
        z, run = R.expand(q, fmt, scale), IntegerIq(ctx, q, fmt, scale)
    for k, v in options.items():
        ctx.set_option(k, v)
    try:
        # 1  the launches are the plan's (guard off: a guarded buffer may be moved to the exact sequence as a whole -- another plan)
        ctx.set_option("sync_guard_ppb", 0)
        try:
            with profiled(ctx) as prof:
                out = run.frames(tsdr.SyncXY(ctx, 600, 800), z, S, y_t, x_t, np.float32(0.1), np.zeros((600, 800), np.float32, order="F"),
                                 want_raster=raster)
                ran = prof.names()
        finally:
            ctx.set_option("sync_guard_ppb", 20000)
        assert out["n_frames"] == FRAMES
        assert {k: v for k, v in ran.items() if k in PROFILE_NAMES} == planned(cid), ran
        # 2  ... and their results the oracle's: rasters, frames, IIR state within RTOL, sync indices identical
        r = fast_vs_oracle(run, tsdr, O, z, S, y_t, x_t, 0.1, raster, RTOL)
        assert r["n_frames"] == FRAMES and not r["ties"]
    finally:
        ctx.set_option("fast_walk_only", 0)
        ctx.set_option("raster_rec4", -1)
