"""What follows a tsdr_frames_d / _sc16_d / _iq_d call whose tail is still on the library's tail lane (option "frames_overlap"):
the hires loop (three streams on one raster workspace), the ring hand-over, every `_d` entry point that reads what the call writes
or overwrites what it still reads, changes of state under it, a producer on the context's stream, two contexts on one device,
and closing a context with tails in flight.

Every case runs one sequence twice on device buffers: with "frames_overlap" 0 (the reference: every call on the context's stream)
and with "frames_overlap" 2 (the lanes, whatever else is alive on the device).  Every observable output is compared bit for bit --
no tolerance appears in this file -- and tsdr_frames_overlap_stats proves the route of both runs: a lane run whose calls stayed on
the context's stream fails, it does not compare the sequential route with itself.

The contract rests on host-side fences only (run_fence in every launch and in front of a handful of copies, the ring hand-over,
fence_inputs, pipe_drain in the entry points).  A missing fence gives wrong pixels only when the timing falls badly, so every lane
run exists twice: as it comes (hold 0), and with tsdr_debug_hold_tail(40) armed before the call whose tail the following action
races.  The hold is a host-side sleep on the tail lane, behind the wait for the image launch and in front of the statistics:
frames, indices, IIR state, the guard's second look at the IQ and its rewrite of images and rasters are 40 ms late, and a consumer
that is not ordered behind the tail reads stale memory every time instead of once in a while.  40 ms stays below the 50 ms bound
of the adaptive route's wait for a guard ring entry; held runs set "sync_guard_auto" 0, so that which frames carry exact pixels
is a function of the buffers alone.  tsdr_wait_stats must not move during a case: a hold that times a wait out makes the case
invalid, not green.

HARDWARE QUEUES.  A held tail lane can share a hardware queue with the context's stream (the processes here open four queues;
the context's stream, the two lanes, the ring's copy stream and torch's streams are spread over them).  The hold then delays the
consumer on the context's stream together with the tail, and a missing fence stays hidden: a FALSE PASS of the held run, never a
false failure.  That is why every case runs both with and without the hold, and why a pass of one held case alone proves less than
the file as a whole.

TEETH.  Against a build whose run_fence returns without draining (everything else as it is) 36 of the 56 cases fail, held or
not: every hires and ring case, the displays, raster register / accum, the three overwriters and the producer case.  The other
20 cannot see that mutant -- their entry points call pipe_drain / pipe_quiesce / pipe_sync_lanes directly (beta, margins, reset,
polarity, the jump to 7 frames, two contexts, close), or read only the IQ, which no call writes (fold, cstack, search) -- and guard
those direct fences instead (NOTEBOOK.md).

Inputs: "small" (S = 6000, 200 x 300, 3 frames + 5 samples, the fused kernels) of tests/test_frames_overlap_gpu.py, and
GEOMS["125x160"] (S = 20000, 5 frames) of tests/test_hires_gpu.py for the hires loop; the plateau card with "sync_guard_ppb"
5000000 wherever the guard has to re-read the IQ and rewrite images (frames_reevaluated > 0 is asserted there).  References are
computed once per configuration and shared."""
import contextlib
import ctypes as C
import threading

import numpy as np
import pytest

from test_frames_overlap_gpu import GEO, NBUF, NFR, NPX, _bufs, _same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
HOLDS = [0, 40]          # ms on the tail lane (below the 50 ms bound of the adaptive route's ring wait)
PPB = 5000000            # the guard really re-evaluates frames of the plateau card
ALPHA = np.float32(0.1)
_REF = {}                # sequential results, once per (case, configuration, "sync_guard_auto")
_HOST = {}


def _api():
    from tempestsdr_jl_amd import api
    return api


@contextlib.contextmanager
def _options(c, overlap, auto, **more):
    """the options of one run, the counters cleared; everything restored afterwards (the hold disarmed too)"""
    c.set_option("frames_overlap", 2 * overlap)
    c.set_option("sync_guard_auto", auto)
    for k, v in more.items():
        c.set_option(k, v)
    # (setting the threshold also restarts the adaptive route's window: both routes start from the same history)
    c.set_option("sync_guard_ppb", PPB)
    c.sync_guard_stats(reset=True)
    c.frames_overlap_stats(reset=True)
    try:
        yield
    finally:
        c.debug_hold_tail(0)
        c.set_option("frames_overlap", 1)
        c.set_option("sync_guard_auto", 1)
        c.set_option("sync_guard_ppb", 20000)
        for k in more:
            c.set_option(k, 0)


def _route(c, overlap, calls):
    """every one of `calls` calls took the route the run is about"""
    on, seq, why = c.frames_overlap_stats()
    assert (on, seq, why) == ((calls, 0, 0) if overlap else (0, calls, 1)), (overlap, calls, on, seq, why)


def _compare(key, hold, run, waits):
    """reference (shared) and lane run of one case; `waits`: the contexts whose tsdr_wait_stats must not move"""
    auto = 0 if hold else 1
    before = [c.wait_stats() for c in waits]
    if (key, auto) not in _REF:
        _REF[(key, auto)] = run(0, 0, auto)
    want, got = _REF[(key, auto)], run(1, hold, auto)
    assert [c.wait_stats() for c in waits] == before, "a wait timed out: the case is invalid"
    _same(want, got, (key, hold))
    return want


def _outs(n, frames=NFR, P=0):
    return [(torch.zeros(frames * NPX, dtype=torch.float32, device=DEV), torch.zeros(frames * P, dtype=torch.float32, device=DEV) if P else None,
             torch.zeros(2 * frames, dtype=torch.int32, device=DEV)) for _ in range(n)]


def _bits(v):
    """a copy of a result as the comparison wants it: floating-point tensors as their bit patterns (a NaN equals itself, -0 is not
    +0), everything else as it is"""
    if not isinstance(v, torch.Tensor):
        return v
    v = v.clone()
    return v.view(torch.int32) if v.dtype == torch.float32 else v.view(torch.int64) if v.dtype == torch.float64 else v


def _collect(res, outs, state):
    res["state"] = _bits(state)
    for k, (fo, ro, si) in enumerate(outs):
        res[f"frames{k}"] = _bits(fo)
        res[f"idx{k}"] = _bits(si)
        if ro is not None:
            res[f"raster{k}"] = _bits(ro)
    return res


# ---------------------------------------------------------------- a. the hires loop
def _hires_bufs(synth, fmt):
    """two consecutive buffers of the plateau leak at GEOMS["125x160"]: (device tensors, scales, samples, S)"""
    from test_hires_gpu import GEOMS, _quantise
    if ("hires", fmt) not in _HOST:
        g = GEOMS["125x160"]
        S = synth.samples_per_frame(g["Fs"], g["fv"])
        n = S * g["nfr"] + g["extra"]
        devs, scales = [], []
        for b in range(2):
            iq = synth.synth_leak(g["Fs"], g["x_t"], g["y_t"], g["fv"], n, n0=b * n, card="plateau")
            q, scale = (iq.view(np.float32), 1.0) if fmt == "cf32" else _quantise(iq, fmt)
            devs.append(torch.from_numpy(np.ascontiguousarray(q)).to(DEV))
            scales.append(scale)
        _HOST[("hires", fmt)] = (devs, scales, n, S)
    return _HOST[("hires", fmt)]


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("fmt", ["cf32", "uc8"])
@pytest.mark.parametrize("refine", [0, 1])
@pytest.mark.parametrize("chunk", [0, 2])
def test_hires_loop(ctx, tsdr, synth, chunk, refine, fmt, hold):
    """tsdr_frames_hires_iq_d for two buffers in a row: every chunk is a tsdr_frames_iq_d call into ONE raster workspace, which the
    guard on the tail lane may rewrite, the registration / accumulation / shift resolution read on the context's stream, and the next
    chunk's image launch on the image lane overwrites.  Chunks of 2 + 2 + 1 frames reuse the workspace three times per call."""
    from test_hires_gpu import GEOMS
    g = GEOMS["125x160"]
    y_t, x_t, nfr = g["y_t"], g["x_t"], g["nfr"]
    iqs, scales, n, S = _hires_bufs(synth, fmt)
    chunks = 2 * (1 if chunk == 0 else -(-nfr // chunk))

    def run(overlap, hold, auto):
        st = torch.zeros(NPX, dtype=torch.float32, device=DEV)
        hs = torch.zeros(y_t * x_t, dtype=torch.float32, device=DEV)
        fr = [torch.zeros(nfr * NPX, dtype=torch.float32, device=DEV) for _ in range(2)]
        ix = [torch.zeros(2 * nfr, dtype=torch.int32, device=DEV) for _ in range(2)]
        torch.cuda.synchronize()
        sync = tsdr.SyncXY(ctx, 600, 800)
        try:
            with _options(ctx, overlap, auto, hires_chunk_frames=chunk, hires_refine=refine):
                for b in range(2):
                    if hold:   # the first chunk's tail is late while accum_launch and the second chunk's image launch follow
                        ctx.debug_hold_tail(hold)
                    assert ctx.frames_hires_d(sync, iqs[b], fmt, scales[b], n, S, y_t, x_t, ALPHA, True, st, ALPHA, hs, fr[b], ix[b]) == nfr
                shifts = ctx.hires_shifts()   # (synchronises)
                ctx.synchronize()
                _route(ctx, overlap, chunks)
                res = {"imageOut": _bits(st), "hires": _bits(hs), "shifts": torch.from_numpy(shifts.copy()), "guard": ctx.sync_guard_stats()}
                for b in range(2):
                    res[f"frames{b}"], res[f"idx{b}"] = _bits(fr[b]), _bits(ix[b])
                return res
        finally:
            sync.close()

    want = _compare(("hires", chunk, refine, fmt), hold, run, [ctx])
    print("guard (checked, re-evaluated):", want["guard"])
    assert want["shifts"].shape == (nfr, 2) and want["guard"][0] == 2 * nfr and want["guard"][1] > 0


# ---------------------------------------------------------------- b. the ring hand-over
def _ring_hosts(synth, raw):
    """8 consecutive plateau buffers at "small" as a producer would hand them over: complex64, or int16 pairs and their scale"""
    if ("ring", raw) not in _HOST:
        g = GEO["small"]
        S = synth.samples_per_frame(g["Fs"], g["fv"])
        n = S * NFR + 5
        hosts = [synth.synth_leak(g["Fs"], g["x_t"], g["y_t"], g["fv"], n, n0=b * n, card="plateau") for b in range(8)]
        scale = 1.0
        if raw:
            scale = float(max(np.max(np.abs(h.view(np.float32))) for h in hosts)) / 2047.0
            hosts = [np.round(h.view(np.float32) / np.float32(scale)).astype(np.int16) for h in hosts]
        _HOST[("ring", raw)] = (hosts, scale, n, S)
    return _HOST[("ring", raw)]


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("ring_fmt", ["cf32", "sc16raw"])
def test_ring_hand_over(ctx, tsdr, synth, ring_fmt, hold):
    """ring of depth 3, a producer thread that commits 8 buffers as fast as the ring takes them without dropping one, and the
    consumer loop tsdr_ring_take_d -> tsdr_frames_d / _sc16_d with no synchronize: the copy stream refills a device buffer that
    the guard on the tail lane of the call two takes back may still be reading.  Hold before calls 2 and 5."""
    api = _api()
    g = GEO["small"]
    P = g["x_t"] * g["y_t"]
    raw = ring_fmt == "sc16raw"
    hosts, scale, n, S = _ring_hosts(synth, raw)
    depth = 3

    def run(overlap, hold, auto):
        outs = _outs(len(hosts), P=P)
        state = torch.zeros(NPX, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        sync = tsdr.SyncXY(ctx, 600, 800)
        ring = tsdr.StagingRing(ctx, n, depth, fmt=ring_fmt, scale=scale)

        halt = threading.Event()

        def produce():   # never overwrites an unread buffer: the results must not depend on which ones the consumer saw
            for h in hosts:
                while not halt.is_set():
                    s = ring.stats()
                    if s["produced"] - s["consumed"] < depth:
                        break
                if halt.is_set():
                    return
                ring.put(h)

        th = threading.Thread(target=produce)
        try:
            with _options(ctx, overlap, auto):
                th.start()
                for k, (fo, ro, si) in enumerate(outs):
                    d = ring.take_d(20000)
                    if hold and k in (2, 5):
                        ctx.debug_hold_tail(hold)
                    if raw:
                        assert api.frames_sc16_d(ctx, sync, d, scale, n, S, g["y_t"], g["x_t"], ALPHA, True, state, fo, ro, si) == NFR
                    else:
                        assert api.frames_d(ctx, sync, d, n, S, g["y_t"], g["x_t"], ALPHA, True, state, fo, ro, si) == NFR
                th.join()
                ctx.synchronize()
                _route(ctx, overlap, len(hosts))
                st = ring.stats()
                assert (st["produced"], st["consumed"], st["overflow"]) == (len(hosts), len(hosts), 0), st
                return _collect({"guard": ctx.sync_guard_stats()}, outs, state)
        finally:
            halt.set()
            ring.stop()
            if th.is_alive():
                th.join()
            ring.close()
            sync.close()

    want = _compare(("ring", ring_fmt), hold, run, [ctx])
    assert want["guard"][0] == len(hosts) * NFR and want["guard"][1] > 0, want["guard"]


# ---------------------------------------------------------------- c. a consumer or overwriter right after call 3 of six
READERS = ["display_frames", "display_state", "raster_register", "raster_accum", "sync_beta", "guard_margins"]
IQ_READERS = ["fold", "cstack_lock", "autocorr_search"]
OVERWRITERS = ["expand_cf32", "expand_sc16", "upload"]
STATE_CHANGERS = ["sync_reset", "blank_dark", "more_frames"]
BIG = 7                  # frames per buffer after the jump of "more_frames"


def _big_bufs(synth):
    """three plateau buffers of BIG frames at "small" (the same geometry, a larger workspace)"""
    if "big" not in _HOST:
        g = GEO["small"]
        S = synth.samples_per_frame(g["Fs"], g["fv"])
        n = S * BIG + 5
        _HOST["big"] = ([torch.from_numpy(synth.synth_leak(g["Fs"], g["x_t"], g["y_t"], g["fv"], n, n0=(NBUF + b) * n, card="plateau")
                                          .view(np.float32)).to(DEV) for b in range(3)], n)
    return _HOST["big"]


def _act(action, api, ctx, sync, synth, out, state, iq, nEch, S, g, work):
    """what the caller does right behind call 3 (outputs `out`, input `iq`): -> its own outputs, device tensors (complete once
    the context's stream is) or host values"""
    y_t, x_t = g["y_t"], g["x_t"]
    P = y_t * x_t
    fo, ro, si = out
    if action == "display_frames":
        u8, rng = torch.zeros(NFR * NPX, dtype=torch.uint8, device=DEV), torch.zeros(2 * NFR, dtype=torch.float32, device=DEV)
        ctx.display_u8_d(fo, NFR, 600, 800, u8, mode="minmax", ranges_out=rng)
        return {"display": u8, "ranges": rng}
    if action == "display_state":
        u8, rng = torch.zeros(NPX, dtype=torch.uint8, device=DEV), torch.zeros(2, dtype=torch.float32, device=DEV)
        ctx.display_u8_d(state, 1, 600, 800, u8, mode="percentile", ranges_out=rng)
        return {"display": u8, "ranges": rng}
    if action == "raster_register":
        from tempestsdr_jl_amd import register
        sh = torch.zeros(2 * NFR, dtype=torch.int32, device=DEV)
        sc = torch.zeros(NFR * register.n_scores(2, 2), dtype=torch.float64, device=DEV)
        ctx.raster_register_d(ro, NFR, y_t, x_t, 2, 2, sh, shifts=si, units="image", scores=sc)
        return {"reg_shifts": sh, "reg_scores": sc}
    if action == "raster_accum":
        hs = torch.zeros(P, dtype=torch.float32, device=DEV)
        ctx.raster_accumulate_d(ro, NFR, y_t, x_t, ALPHA, hs, shifts=si, units="image")
        return {"hires": hs}
    if action == "sync_beta":
        return {"act_beta_x": torch.from_numpy(sync.beta("x").copy()), "act_beta_y": torch.from_numpy(sync.beta("y").copy())}
    if action == "guard_margins":
        m = ctx.sync_guard_margins()
        assert m.shape == (NFR, 2)
        return {"margins": torch.from_numpy(m.copy())}
    if action == "fold":
        st = torch.zeros(P, dtype=torch.float32, device=DEV)
        ctx.fold_d(iq, "cf32", 1.0, nEch, 0.0, float(S), NFR, y_t, x_t, 0.0, st)
        return {"fold": st}
    if action == "cstack_lock":
        z, mag = torch.zeros(2 * P, dtype=torch.float32, device=DEV), torch.zeros(P, dtype=torch.float32, device=DEV)
        info = torch.zeros(8, dtype=torch.float64, device=DEV)
        ctx.cstack_d(iq, "cf32", 1.0, nEch, 0.0, float(S), 0.0, 0.0, NFR, y_t, x_t, 0.0, "given", z)
        ctx.cstack_d(iq, "cf32", 1.0, nEch, 0.0, float(S), 0.01, 0.0, NFR, y_t, x_t, 0.5, "lock", z, mag, info)
        return {"zstate": z, "mag": mag, "info": info}
    if action == "autocorr_search":
        Fs, max_delay = g["Fs"], 0.03
        cnt = int(np.round(max_delay * Fs))
        lo, hi = C.c_size_t(0), C.c_size_t(0)
        assert ctx.lib.tsdr_zoom_bounds(cnt, Fs, 50.0, 90.0, C.byref(lo), C.byref(hi)) == 0
        G = torch.zeros(cnt, dtype=torch.float32, device=DEV)
        n_out, idx, val = C.c_size_t(0), C.c_size_t(0), C.c_float(0)
        ctx.call("tsdr_autocorr_search_iq_d", C.c_void_p(iq.data_ptr()), 0, C.c_float(1.0), nEch, Fs, 0.0, max_delay, 1, C.c_void_p(G.data_ptr()),
                 C.byref(n_out), lo.value - 1, hi.value - lo.value + 1, C.byref(idx), C.byref(val))
        assert n_out.value == cnt
        return {"lags": G, "peak": (int(idx.value), float(val.value))}
    # the overwriters: call 3 ran on `work`, whose IQ its guard may still be re-reading; call 4 runs on `work` as well
    if action == "expand_cf32":   # the copy path
        src = _bufs(synth, "small", "cf32", "plateau")[0][3]
        api.expand_iq_d(ctx, src, "cf32", 1.0, nEch, work)
    elif action == "expand_sc16":   # the kernel path
        q, qscale = _bufs(synth, "small", "sc16", "plateau")[:2]
        api.expand_iq_d(ctx, q[3], "sc16", qscale, nEch, work)
    elif action == "upload":
        ctx.call("tsdr_upload", C.c_void_p(work.data_ptr()), C.c_void_p(_HOST["upload"].ctypes.data), _HOST["upload"].nbytes)
    elif action == "sync_reset":
        sync.reset()
    elif action == "blank_dark":   # (back to 0 behind call 4)
        ctx.set_option("vsync_blank_dark", 1)
    return {}


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("action", READERS + IQ_READERS + OVERWRITERS + STATE_CHANGERS)
def test_what_follows_call_three(ctx, tsdr, synth, action, hold):
    """six calls on one SyncXY / IIR state, one output set per call; right behind call 3 (whose tail is held in the held run) the
    caller reads what the call writes, reads or OVERWRITES the IQ its guard may still re-read, or changes state under it.  The
    action's own output equals what it gives behind a synchronize in the reference run; everything else equals as well."""
    api = _api()
    g = GEO["small"]
    y_t, x_t = g["y_t"], g["x_t"]
    iqs, _, nEch, S = _bufs(synth, "small", "cf32", "plateau")
    big, n_big = _big_bufs(synth) if action == "more_frames" else (None, 0)
    if action == "upload" and "upload" not in _HOST:
        _HOST["upload"] = iqs[3].cpu().numpy()

    def run(overlap, hold, auto):
        outs = _outs(NBUF, frames=BIG if big else NFR, P=y_t * x_t)
        state = torch.zeros(NPX, dtype=torch.float32, device=DEV)
        work = iqs[2].clone() if action in OVERWRITERS else None
        img = torch.from_numpy(np.random.default_rng(5).random(NPX).astype(np.float32))
        torch.cuda.synchronize()
        sync = tsdr.SyncXY(ctx, 600, 800)
        extra = {}
        try:
            with _options(ctx, overlap, auto):
                try:
                    for b in range(NBUF):
                        iq, n, nfr = iqs[b], nEch, NFR
                        if work is not None and b in (2, 3):
                            iq = work
                        if big and b >= 3:   # the workspaces grow with tails in flight
                            iq, n, nfr = big[b - 3], n_big, BIG
                        if b == 2 and hold:
                            ctx.debug_hold_tail(hold)
                        if b == 3:
                            if not overlap:   # the reference: what the action gives behind a synchronize
                                ctx.synchronize()
                            extra = _act(action, api, ctx, sync, synth, outs[2], state, iqs[2], nEch, S, g, work)
                        assert api.frames_d(ctx, sync, iq, n, S, y_t, x_t, ALPHA, True, state, *outs[b]) == nfr
                        if b == 3 and action == "blank_dark":
                            ctx.set_option("vsync_blank_dark", 0)
                finally:
                    ctx.set_option("vsync_blank_dark", 0)
                ctx.synchronize()
                _route(ctx, overlap, NBUF)
                res = _collect({k: _bits(v) for k, v in extra.items()}, outs, state)
                res["guard"] = ctx.sync_guard_stats()
                res["pending"] = tuple(int(v) for v in sync.vsync(img.numpy().reshape(800, 600).T))
                res["beta_x"], res["beta_y"] = _bits(torch.from_numpy(sync.beta("x").copy())), _bits(torch.from_numpy(sync.beta("y").copy()))
                return res
        finally:
            sync.close()

    want = _compare(("call3", action), hold, run, [ctx])
    assert want["guard"][0] == (3 * NFR + 3 * BIG if big else NBUF * NFR) and want["guard"][1] > 0, want["guard"]


# ---------------------------------------------------------------- d. the caller's producer on the context's stream
@pytest.mark.parametrize("hold", HOLDS)
def test_producer_on_the_contexts_stream(ctx, tsdr, synth, hold):
    """the context's stream is held for 30 ms (a caller's unfinished work), behind it tsdr_iq_expand_d (sc16 -> cf32) writes the
    buffer tsdr_frames_d then consumes: the image lane waits for the expansion (fence_inputs).  Every call expands into the same
    buffer, so the next expansion also has to come behind the guard's second look at it.  (Four calls: the adaptive route's
    wait at call k + 3 is for a call in front of the two holds.)"""
    api = _api()
    g = GEO["small"]
    q, qscale, nEch, S = _bufs(synth, "small", "sc16", "plateau")
    calls = 4

    def run(overlap, hold, auto):
        outs = _outs(calls, P=g["x_t"] * g["y_t"])
        state = torch.zeros(NPX, dtype=torch.float32, device=DEV)
        work = torch.zeros(2 * nEch, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        sync = tsdr.SyncXY(ctx, 600, 800)
        try:
            with _options(ctx, overlap, auto):
                for b in range(calls):
                    if b == 1:
                        ctx.call("tsdr_debug_hold_stream", 30)
                        if hold:
                            ctx.debug_hold_tail(hold)
                    api.expand_iq_d(ctx, q[b], "sc16", qscale, nEch, work)
                    assert api.frames_d(ctx, sync, work, nEch, S, g["y_t"], g["x_t"], ALPHA, True, state, *outs[b]) == NFR
                ctx.synchronize()
                _route(ctx, overlap, calls)
                return _collect({"guard": ctx.sync_guard_stats()}, outs, state)
        finally:
            sync.close()

    want = _compare(("producer",), hold, run, [ctx])
    assert want["guard"][0] == calls * NFR and want["guard"][1] > 0, want["guard"]


# ---------------------------------------------------------------- e. two contexts on one device, f. close with tails in flight
def _private(tsdr, overlap, auto):
    c = tsdr.Context(0)
    c.set_option("frames_overlap", 2 * overlap)
    c.set_option("sync_guard_auto", auto)
    c.set_option("sync_guard_ppb", PPB)
    return c


def _six_setup(tsdr, c, P):
    return dict(c=c, sync=tsdr.SyncXY(c, 600, 800), outs=_outs(NBUF, P=P), state=torch.zeros(NPX, dtype=torch.float32, device=DEV))


def _six_call(api, r, iqs, b, nEch, S, g, hold):
    if hold and b == 2:
        r["c"].debug_hold_tail(hold)
    assert api.frames_d(r["c"], r["sync"], iqs[b], nEch, S, g["y_t"], g["x_t"], ALPHA, True, r["state"], *r["outs"][b]) == NFR


def _six_result(r, overlap):
    r["c"].synchronize()
    _route(r["c"], overlap, NBUF)
    return _collect({"guard": r["c"].sync_guard_stats()}, r["outs"], r["state"])


@pytest.mark.parametrize("hold", HOLDS)
def test_two_contexts_both_on_the_lanes(ctx, tsdr, synth, hold):
    """two contexts that both force the lanes ("frames_overlap" 2), each with its own SyncXY, state and outputs, six calls each,
    alternating: each context's results equal those of its own sequential run alone"""
    api = _api()
    g = GEO["small"]
    P = g["x_t"] * g["y_t"]
    inputs = [_bufs(synth, "small", "cf32", "plateau"), _bufs(synth, "small", "cf32", "box")]
    auto = 0 if hold else 1
    for who, (iqs, _, nEch, S) in enumerate(inputs):   # each context's sequential run, alone
        if (("pair", who), auto) not in _REF:
            c = _private(tsdr, 0, auto)
            try:
                r = _six_setup(tsdr, c, P)
                torch.cuda.synchronize()
                w0 = c.wait_stats()
                for b in range(NBUF):
                    _six_call(api, r, iqs, b, nEch, S, g, 0)
                _REF[(("pair", who), auto)] = _six_result(r, 0)
                assert c.wait_stats() == w0
                r["sync"].close()
            finally:
                c.close()
    cs = [_private(tsdr, 1, auto), _private(tsdr, 1, auto)]
    try:
        rs = [_six_setup(tsdr, c, P) for c in cs]
        torch.cuda.synchronize()
        w0 = [c.wait_stats() for c in cs]
        for b in range(NBUF):
            for r, (iqs, _, nEch, S) in zip(rs, inputs):
                _six_call(api, r, iqs, b, nEch, S, g, hold)
        got = [_six_result(r, 1) for r in rs]
        assert [c.wait_stats() for c in cs] == w0, "a wait timed out: the case is invalid"
        for r in rs:
            r["sync"].close()
    finally:
        for c in cs:
            c.close()
    for who in (0, 1):
        _same(_REF[(("pair", who), auto)], got[who], ("pair", who, hold))
    assert _REF[(("pair", 0), auto)]["guard"][1] > 0


@pytest.mark.parametrize("hold", HOLDS)
def test_close_with_tails_in_flight(tsdr, synth, hold):
    """a private context makes three calls and is closed with no synchronize: close() returns without error, and once the device
    is idle the test-owned outputs hold what the sequential run gives.  (tsdr_wait_stats is read right before the close: a
    closed context has none.  The SyncXY outlives its context and is dropped with it.)"""
    api = _api()
    g = GEO["small"]
    iqs, _, nEch, S = _bufs(synth, "small", "cf32", "plateau")
    auto = 0 if hold else 1

    def run(overlap, hold):
        c = _private(tsdr, overlap, auto)
        try:
            outs = _outs(3, P=g["x_t"] * g["y_t"])
            state = torch.zeros(NPX, dtype=torch.float32, device=DEV)
            sync = tsdr.SyncXY(c, 600, 800)
            torch.cuda.synchronize()
            w0 = c.wait_stats()
            for b in range(3):
                if hold and b == 2:
                    c.debug_hold_tail(hold)
                assert api.frames_d(c, sync, iqs[b], nEch, S, g["y_t"], g["x_t"], ALPHA, True, state, *outs[b]) == NFR
            _route(c, overlap, 3)
            assert c.wait_stats() == w0
        finally:
            c.close()
        assert c.h is None
        torch.cuda.synchronize()
        return _collect({}, outs, state)

    if (("close",), auto) not in _REF:
        _REF[(("close",), auto)] = run(0, 0)
    _same(_REF[(("close",), auto)], run(1, hold), ("close", hold))
