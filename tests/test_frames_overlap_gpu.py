"""tsdr_frames_d / _sc16_d / _iq_d leave a buffer's tail (vsync statistics, sync guard, shift + IIR) on the library's tail lane,
beside the image launch of the next call (option "frames_overlap", default 1).  The caller sees none of it: every result --
frames, rasters, sync indices, the IIR state, the SyncXY state carried across buffers, the guard's counters -- equals, bit for
bit, what the same calls give with "frames_overlap" 0, whatever else the caller does through the library between two calls.

Shapes: the smallest geometry that takes the fused kernels (S = 6000, 200 x 300: "small" of tools/host_plan/plan_dump.h) and one
that takes none (S = 600, 20 x 30: the per-frame fallback of the image step); 3 frames per
buffer, 6 buffers, so the three image / key / projection slots wrap twice.  Near-tie inputs are built the way
tests/test_fast_mode_gpu.py builds them: synth_leak(..., card="plateau"), whose flat blanking level ties neighbouring columns."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NPX = 600 * 800
NFR, NBUF = 3, 6
GEO = {"small": dict(Fs=300000.0, x_t=300, y_t=200, fv=50.0), "plain": dict(Fs=30000.0, x_t=30, y_t=20, fv=50.0)}

_BUFS = {}
_SEQ = {}   # sequential ("frames_overlap" 0) results, computed once per configuration and shared


def _bufs(synth, geo, fmt, card="box"):
    """NBUF device buffers of NFR frames (+ a ragged tail) of the leak at geometry `geo`: (tensors, scale, nEch, S)"""
    key = (geo, fmt, card)
    if key not in _BUFS:
        g = GEO[geo]
        S = synth.samples_per_frame(g["Fs"], g["fv"])
        n = S * NFR + 5
        hosts = [synth.synth_leak(g["Fs"], g["x_t"], g["y_t"], g["fv"], n, n0=b * n, card=card).view(np.float32) for b in range(NBUF)]
        scale = np.float32(1.0)
        if fmt == "sc16":
            scale = np.float32(float(max(np.max(np.abs(h)) for h in hosts)) / 2047.0)
            hosts = [np.round(h / scale).astype(np.int16) for h in hosts]
        _BUFS[key] = ([torch.from_numpy(h).to("cuda:0") for h in hosts], scale, n, S)
    return _BUFS[key]


def _call(api, ctx, sync, iq, fmt, scale, nEch, S, g, do_align, state, out, submit=False):
    fo, ro, si = out
    args = (nEch, S, g["y_t"], g["x_t"], np.float32(0.1), do_align, state, fo, ro, si if do_align else None)
    if fmt == "sc16":
        n = api.frames_sc16_d(ctx, sync, iq, scale, *args, submit=submit)
    else:
        n = (api.frames_submit_d if submit else api.frames_d)(ctx, sync, iq, *args)
    assert n == NFR


def _expected_route(overlap, calls, between=None):
    """(on_lanes, sequential, why) of tsdr_frames_overlap_stats after `calls` calls with "frames_overlap" 2 * overlap: the one
    call through tsdr_frames_submit_d counts in neither, the one TSDR_EXACT call is sequential whatever the option says"""
    n = calls - 1 if between == "submit_flush" else calls
    if not overlap:
        return 0, n, 1   # (the latest sequential call is a plain one: the option alone)
    return (n - 1, 1, 4) if between == "exact" else (n, 0, 0)


def _run(ctx, tsdr, synth, overlap, geo="small", fmt="cf32", raster=True, do_align=True, current_sy=0, reuse=False, card="box",
         between=None, ppb=None, calls=NBUF, ext_event=None):
    """Six calls on one SyncXY / IIR state; `between`: what the caller does around the fourth call.  Returns everything a caller
    can observe afterwards, as a dict of tensors / tuples.  The route the calls took is asserted (tsdr_frames_overlap_stats): a run
    with the option on that stayed on the context's stream fails here."""
    from tempestsdr_jl_amd import api
    g = GEO[geo]
    iqs, scale, nEch, S = _bufs(synth, geo, fmt, card)
    P = g["x_t"] * g["y_t"]
    other = "plain" if geo == "small" else "small"
    Pmax = max(P, GEO[other]["x_t"] * GEO[other]["y_t"]) if between == "geometry" else P
    dev = "cuda:0"
    nout = 1 if reuse else NBUF
    outs = [(torch.zeros(NFR * NPX, dtype=torch.float32, device=dev), torch.zeros(NFR * Pmax, dtype=torch.float32, device=dev) if raster else None,
             torch.zeros(2 * NFR, dtype=torch.int32, device=dev)) for _ in range(nout)]
    state = torch.zeros(NPX, dtype=torch.float32, device=dev)
    img = torch.from_numpy(np.random.default_rng(5).random(NPX).astype(np.float32)).to(dev)
    s_yx = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sync = tsdr.SyncXY(ctx, 600, 800) if do_align else None
    extra = {}
    ctx.set_option("frames_overlap", 2 * overlap)   # (2: on beside the other contexts a test session keeps alive; 1 would be off there)
    ctx.set_option("vsync_current_sy", current_sy)
    # (setting the threshold also restarts the adaptive route's window: which buffers run exactly as a whole follows from the
    # flagged-frame counts of the calls before, so both routes must start from the same history)
    ctx.set_option("sync_guard_ppb", 20000 if ppb is None else ppb)
    ctx.sync_guard_stats(reset=True)
    route0 = ctx.sync_guard_auto()
    if ext_event is not None:   # (how the tail's event is recorded: with the shift + IIR dispatch, or as a marker of its own)
        ctx.set_option("pipe_ext_event", ext_event)
    ctx.frames_overlap_stats(reset=True)
    try:
        for b in range(calls):
            out = outs[b % nout]
            act = between if b == 3 else None
            if act == "synchronize":
                ctx.synchronize()
            elif act == "download":   # no synchronize: the download itself must come behind the tail of call 2
                extra["download"] = torch.from_numpy(ctx.download(outs[2 % nout][0].data_ptr(), (NFR * NPX,), np.float32).copy())
            elif act == "vsync_d":
                rc = ctx.lib.tsdr_vsync_d(sync.h, C.c_void_p(img.data_ptr()), C.c_void_p(s_yx.data_ptr()))
                assert rc == 0
            elif act == "timer":
                ctx.timer_start()
            if act == "exact":
                ctx.set_precision("exact")
            try:
                if act == "geometry":
                    iqo, so, no, So = _bufs(synth, other, fmt)
                    _call(api, ctx, sync, iqo[b % NBUF], fmt, so, no, So, GEO[other], do_align, state, out)
                else:
                    _call(api, ctx, sync, iqs[b % NBUF], fmt, scale, nEch, S, g, do_align, state, out, submit=act == "submit_flush")
            finally:
                if act == "exact":
                    ctx.set_precision("fast")
            if act == "submit_flush":
                api.frames_flush(ctx)
            elif act == "timer":
                extra["timer_ms"] = ctx.timer_stop()
        ctx.synchronize()
        assert ctx.frames_overlap_stats() == _expected_route(overlap, calls, between), (overlap, between, ctx.frames_overlap_stats())
        res = {"state": state.clone(), "guard": ctx.sync_guard_stats(), "s_yx": s_yx.clone()}
        route1 = ctx.sync_guard_auto()   # the adaptive route: (whole buffers exactly right now, calls that ran so, route changes)
        res["route"] = (route1[0], route1[1] - route0[1], route1[2] - route0[2])
        for k, (fo, ro, si) in enumerate(outs):
            res[f"frames{k}"] = fo.clone()
            res[f"idx{k}"] = si.clone()
            if ro is not None:
                res[f"raster{k}"] = ro.clone()
        if "download" in extra:
            res["download"] = extra["download"]
        if sync is not None:   # the SyncXY state the next buffer would continue from: pending s_y (through one more vsync) and beta
            res["pending"] = tuple(int(v) for v in sync.vsync(img.cpu().numpy().reshape(800, 600).T))
            res["beta_x"] = torch.from_numpy(sync.beta("x").copy())
            res["beta_y"] = torch.from_numpy(sync.beta("y").copy())
        if "timer_ms" in extra:
            assert extra["timer_ms"] > 0.0
        return res
    finally:
        ctx.set_option("frames_overlap", 1)
        ctx.set_option("vsync_current_sy", 0)
        if ext_event is not None:
            ctx.set_option("pipe_ext_event", 1)
        if ppb is not None:
            ctx.set_option("sync_guard_ppb", 20000)
        if sync is not None:
            sync.close()


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _sequential(ctx, tsdr, synth, **cfg):
    key = tuple(sorted(cfg.items()))
    if key not in _SEQ:
        _SEQ[key] = _run(ctx, tsdr, synth, 0, **cfg)
    return _SEQ[key]


@pytest.mark.parametrize("reuse", [True, False], ids=["one_output_set", "output_set_per_call"])
@pytest.mark.parametrize("fmt", ["cf32", "sc16"])
@pytest.mark.parametrize("geo", ["small", "plain"])
def test_overlap_equals_sequential(ctx, tsdr, synth, geo, fmt, reuse):
    """rasters or not, aligned or not, either s_y ordering: frames, rasters, sync indices, IIR state, pending s_y, beta and
    the guard's counters of six calls, bit for bit"""
    for raster, do_align, current_sy in itertools.product((True, False), (True, False), (0, 1)):
        if not do_align and current_sy:
            continue   # (the option is read by the aligned path only)
        cfg = dict(geo=geo, fmt=fmt, raster=raster, do_align=do_align, current_sy=current_sy, reuse=reuse)
        _same(_sequential(ctx, tsdr, synth, **cfg), _run(ctx, tsdr, synth, 1, **cfg), cfg)


@pytest.mark.parametrize("ext_event", [1, 0])
def test_overlap_equals_sequential_with_either_tail_event(ctx, tsdr, synth, ext_event):
    """"pipe_ext_event" 1 (default): the tail's event -- what every later fence waits for -- rides on the shift + IIR dispatch;
    0: it is a marker of its own behind it.  Two implementations of the same fence, the same results."""
    cfg = dict(geo="small", fmt="cf32", raster=True, do_align=True, current_sy=0, reuse=False)
    _same(_sequential(ctx, tsdr, synth, **cfg), _run(ctx, tsdr, synth, 1, ext_event=ext_event, **cfg), ext_event)


def test_overlap_is_off_on_an_adopted_stream(ctx, tsdr, synth):
    """tsdr_set_stream to a stream of the caller's: calls stay on it (stream order alone holds there), tsdr_frames_overlap_stats
    says why (8); back on a stream of its own the context takes the lanes again.  Results equal the sequential run's."""
    from tempestsdr_jl_amd import api
    cfg = dict(geo="small", fmt="cf32", raster=True, do_align=True, current_sy=0, reuse=False)
    want = _sequential(ctx, tsdr, synth, **cfg)
    g = GEO["small"]
    iqs, scale, nEch, S = _bufs(synth, "small", "cf32")
    outs = [(torch.zeros(NFR * NPX, dtype=torch.float32, device="cuda:0"), torch.zeros(NFR * g["x_t"] * g["y_t"], dtype=torch.float32, device="cuda:0"),
             torch.zeros(2 * NFR, dtype=torch.int32, device="cuda:0")) for _ in range(NBUF)]
    state = torch.zeros(NPX, dtype=torch.float32, device="cuda:0")
    mine = torch.cuda.Stream()
    torch.cuda.synchronize()
    sync = tsdr.SyncXY(ctx, 600, 800)
    ctx.set_option("frames_overlap", 2)
    ctx.sync_guard_stats(reset=True)
    ctx.frames_overlap_stats(reset=True)
    try:
        for b in (0, 1):
            _call(api, ctx, sync, iqs[b], "cf32", scale, nEch, S, g, True, state, outs[b])
        assert ctx.frames_overlap_stats() == (2, 0, 0)
        ctx.set_stream(mine.cuda_stream)   # (with two tails in flight: ordered through the old stream first)
        try:
            for b in (2, 3):
                _call(api, ctx, sync, iqs[b], "cf32", scale, nEch, S, g, True, state, outs[b])
            assert ctx.frames_overlap_stats() == (2, 2, 8)
        finally:
            ctx.set_stream(None)
        for b in (4, 5):
            _call(api, ctx, sync, iqs[b], "cf32", scale, nEch, S, g, True, state, outs[b])
        assert ctx.frames_overlap_stats() == (4, 2, 8)
        ctx.synchronize()
        assert torch.equal(state, want["state"]) and ctx.sync_guard_stats() == want["guard"]
        for k, (fo, ro, si) in enumerate(outs):
            assert torch.equal(fo, want[f"frames{k}"]) and torch.equal(ro, want[f"raster{k}"]) and torch.equal(si, want[f"idx{k}"]), k
        # (the SyncXY state as _run reads it: the pending s_y through one more vsync of the same image, then beta)
        img = np.random.default_rng(5).random(NPX).astype(np.float32)
        assert tuple(int(v) for v in sync.vsync(img.reshape(800, 600).T)) == want["pending"]
        assert torch.equal(torch.from_numpy(sync.beta("x").copy()), want["beta_x"]) and torch.equal(torch.from_numpy(sync.beta("y").copy()), want["beta_y"])
    finally:
        ctx.set_option("frames_overlap", 1)
        sync.close()


def test_default_option_in_a_process_of_its_own():
    """The real default -- one context alone on its device, "frames_overlap" left at 1 -- in a fresh process (tests/overlap_child.py):
    six calls on the lanes, a second context turns them off for the next call (why: 1), closing it turns them on again, and all
    eight calls give what the same eight give with the option 0."""
    import json
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "overlap_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    print(line)
    assert line["alone"] == [6, 0, 0], line
    assert line["second_context"] == [6, 1, 1], line
    assert line["alone_again"] == [7, 1, 1], line
    assert line["option_0"] == [0, 8, 1], line
    assert line["equal"] is True and line["guard"][0] == 8 * NFR, line


@pytest.mark.parametrize("between", ["synchronize", "timer", "download", "vsync_d", "submit_flush", "exact", "geometry"])
def test_overlap_with_other_calls_in_between(ctx, tsdr, synth, between):
    """what a caller may do between two calls -- wait, time, read a result back, use the SyncXY state, submit to the pipeline,
    switch the precision, change the geometry -- sees completed results and leaves the sequence of results unchanged"""
    cfg = dict(geo="small", fmt="cf32", raster=True, do_align=True, between=between)
    want, got = _sequential(ctx, tsdr, synth, **cfg), _run(ctx, tsdr, synth, 1, **cfg)
    _same(want, got, between)
    if between == "download":   # read back with call 2's tail possibly still on its lane: call 2's frames
        assert torch.equal(got["download"], want["frames2"].cpu())


@pytest.mark.parametrize("raster", [True, False])
def test_overlap_guard_reevaluation_matches_sequential(ctx, tsdr, synth, raster):
    """near-tie buffers (the plateau leak) with the threshold raised so that frames ARE re-evaluated: the guard launch runs on
    the tail lane beside the next image launch, reads the call's IQ again and rewrites its images; results and counters equal
    the sequential route's"""
    cfg = dict(geo="small", fmt="cf32", raster=raster, do_align=True, card="plateau", ppb=5000000)
    want, got = _sequential(ctx, tsdr, synth, **cfg), _run(ctx, tsdr, synth, 1, **cfg)
    print("guard (checked, re-evaluated):", want["guard"], got["guard"])
    assert want["guard"][0] == NBUF * NFR and want["guard"][1] > 0
    _same(want, got, "guard")


def test_overlap_guard_route_switch_matches_sequential(ctx, tsdr, synth):
    """30 near-tie buffers (90 frames: past the 60-frame window of the adaptive route) with most frames flagged: the route
    switches to whole buffers in the exact sequence, decided on the host from the ring entries of the calls three back, which
    under overlap are written on the tail lane.  The switch happens at the same call, the same number of buffers run exactly,
    and every result and counter equals the sequential route's."""
    cfg = dict(geo="small", fmt="cf32", raster=True, do_align=True, card="plateau", ppb=50000000, calls=30, reuse=True)
    want, got = _sequential(ctx, tsdr, synth, **cfg), _run(ctx, tsdr, synth, 1, **cfg)
    print("guard (checked, re-evaluated), route (exact now, buffers exact, switches):", want["guard"], want["route"], got["guard"], got["route"])
    assert want["route"][1] > 0 and want["route"][2] >= 1, "the plateau leak should have switched the route"
    _same(want, got, "route")


def test_overlap_is_off_while_profiling(ctx, tsdr, synth):
    """ctx.profile(True) brackets every launch with its own event pair on the context's stream: the same kernels, each once
    per buffer, as with "frames_overlap" 0"""
    from tempestsdr_jl_amd import api
    g = GEO["small"]
    iqs, scale, nEch, S = _bufs(synth, "small", "cf32")
    got = {}
    for overlap in (1, 0):
        sync = tsdr.SyncXY(ctx, 600, 800)
        out = (torch.zeros(NFR * NPX, dtype=torch.float32, device="cuda:0"), torch.zeros(NFR * g["x_t"] * g["y_t"], dtype=torch.float32, device="cuda:0"),
               torch.zeros(2 * NFR, dtype=torch.int32, device="cuda:0"))
        state = torch.zeros(NPX, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.set_option("frames_overlap", 2 * overlap)
        ctx.frames_overlap_stats(reset=True)
        try:
            _call(api, ctx, sync, iqs[0], "cf32", scale, nEch, S, g, True, state, out)   # (one overlapped call in flight first)
            assert ctx.frames_overlap_stats(reset=True) == ((1, 0, 0) if overlap else (0, 1, 1))
            ctx.profile_reset()
            ctx.profile(True)
            for b in (1, 2):
                _call(api, ctx, sync, iqs[b], "cf32", scale, nEch, S, g, True, state, out)
            ctx.profile(False)
            # (both profiled calls ran on the context's stream, and profiling is why: bit 2, beside bit 1 where the option is off too)
            assert ctx.frames_overlap_stats() == (0, 2, 2 if overlap else 3)
            got[overlap] = {k: v["launches"] for k, v in ctx.profile_results().items()}
        finally:
            ctx.set_option("frames_overlap", 1)
            ctx.profile_reset()
            sync.close()
    print("launches of two buffers:", got[1])
    assert got[1] == got[0]
    # (each kernel once per buffer: four launches at the benchmark's geometry, where raster and image are one launch; more here)
    assert {"shift_iir", "sync_beta"} <= set(got[1]) and set(got[1].values()) == {2}, got[1]


def test_overlap_does_not_touch_the_pipeline_measurement(tsdr, synth):
    """tsdr_frames_d never spends buffers on trials: tsdr_frames_pipeline_info before and after is the same, measured choice or
    forced arrangement"""
    from tempestsdr_jl_amd import api
    g = GEO["small"]
    iqs, scale, nEch, S = _bufs(synth, "small", "cf32")
    c = tsdr.Context(0)
    try:
        sync = tsdr.SyncXY(c, 600, 800)
        out = (torch.zeros(NFR * NPX, dtype=torch.float32, device="cuda:0"), None, torch.zeros(2 * NFR, dtype=torch.int32, device="cuda:0"))
        state = torch.zeros(NPX, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        c.set_option("frames_overlap", 2)
        for mode in (-1, 2):
            c.set_option("pipe_mode", mode)
            before = c.pipeline_info()
            for b in range(NBUF):
                _call(api, c, sync, iqs[b], "cf32", scale, nEch, S, g, True, state, out)
            c.synchronize()
            assert c.pipeline_info() == before, mode
        c.set_option("pipe_mode", -1)
        assert c.pipeline_info()["trials_left"] == 2 * 8 + 1   # nothing measured yet: every trial still to come
        sync.close()
    finally:
        c.close()


def test_overlap_call_with_a_new_syncxy_returns_while_the_stream_is_held(tsdr, synth):
    """A call that brings another SyncXY state runs the lanes empty first.  Lanes the host has already seen complete (a
    synchronize since the last call) are not waited for again: one of them may share a hardware queue with the context's stream,
    and while that stream is held (tsdr_debug_hold_stream: a caller's unfinished work) a marker on it would hold the call as
    well.  tsdr_frames_d only enqueues here, as it does with "frames_overlap" 0; 100 ms is the bound of
    tests/test_bounded_waits_gpu.py for a call that waits for nothing that is held, the hold is three times that."""
    import time

    from tempestsdr_jl_amd import api
    g = GEO["small"]
    iqs, scale, nEch, S = _bufs(synth, "small", "cf32")
    c = tsdr.Context(0)
    try:
        syncs = [tsdr.SyncXY(c, 600, 800), tsdr.SyncXY(c, 600, 800)]   # (both alive: two addresses, so the pipeline's key changes)
        out = (torch.zeros(NFR * NPX, dtype=torch.float32, device="cuda:0"), None, torch.zeros(2 * NFR, dtype=torch.int32, device="cuda:0"))
        state = torch.zeros(NPX, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        walls = {}
        for overlap in (0, 1):
            c.set_option("frames_overlap", 2 * overlap)
            for b in range(3):   # (three complete calls: the guard entries that the held call's route decision folds)
                _call(api, c, syncs[0], iqs[b], "cf32", scale, nEch, S, g, True, state, out)
            c.synchronize()
            c.call("tsdr_debug_hold_stream", 300)
            t0 = time.perf_counter()
            _call(api, c, syncs[1], iqs[3], "cf32", scale, nEch, S, g, True, state, out)
            walls[overlap] = time.perf_counter() - t0
            c.synchronize()
        print("held call with a new SyncXY, seconds (overlap off, on):", walls)
        assert walls[0] < 0.100 and walls[1] < 0.100, walls
        for s in syncs:
            s.close()
    finally:
        c.close()
