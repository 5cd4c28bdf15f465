"""GPU tests: every host-side wait of the library is bounded (round 6; VERDICT r5 "What's weak" 2).

A frame-loop call of a Julia GUI thread must never spin forever inside a ccall (GUI.jl:197-200 swallows a consumer task's
exceptions; it cannot swallow a call that does not return).  tsdr_debug_hold_stream puts a host-side delay on the context's
stream -- what a stream held by something that does not complete looks like -- and the tests show

  * tsdr_frames_d / tsdr_frames_submit_d: the adaptive route's wait for the guard entry of call k - 3 gives up after 50 ms
    (2 ms for the entries after a timed-out one), the entry goes uncounted (tsdr_wait_stats), the call returns;
  * tsdr_synchronize: TSDR_EHIP with the stage in tsdr_last_error after "wait_ms", the context usable afterwards;
  * results of the held calls are the un-held ones once the hold ends."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Fs, X_T, Y_T, NFR = 2.0e6, 1056, 628, 6


def _loop(tsdr, ctx, iq, S, n_calls, submit, hold_ms=0):
    from tempestsdr_jl_amd import api
    npx = 600 * 800
    nb = iq.size // S
    sync = tsdr.SyncXY(ctx, 600, 800)
    d_state = ctx.upload(np.zeros(npx, np.float32))
    d_in = ctx.upload(iq.view(np.float32))
    d_fr = [ctx.dev_alloc(nb * npx * 4) for _ in range(n_calls)]
    d_ix = [ctx.dev_alloc(nb * 8) for _ in range(n_calls)]
    f = api.frames_submit_d if submit else api.frames_d
    walls = []
    try:
        ctx.synchronize()
        if hold_ms:
            ctx.call("tsdr_debug_hold_stream", int(hold_ms))
        for k in range(n_calls):
            t0 = time.perf_counter()
            f(ctx, sync, d_in, nb * S, S, Y_T, X_T, np.float32(0.1), True, d_state, d_fr[k], None, d_ix[k])
            walls.append(time.perf_counter() - t0)
        stats_during = ctx.wait_stats()
        ctx.synchronize()
        out = [(ctx.download(d_fr[k], (nb * npx,), np.uint32), ctx.download(d_ix[k], (nb * 2,), np.int32)) for k in range(n_calls)]
    finally:
        sync.close()
        for p in [d_state, d_in] + d_fr + d_ix:
            ctx.dev_free(p)
    return walls, stats_during, out


@pytest.mark.parametrize("submit", [False, True])
def test_frame_loop_returns_while_its_stream_is_held(tsdr, synth, submit):
    S = synth.samples_per_frame(Fs, 60.0)
    iq = synth.synth_leak(Fs, X_T, Y_T, 60.0, S * NFR)
    ctx = tsdr.Context(0)
    try:
        if submit:
            ctx.set_option("pipe_mode", 0)    # (a fixed arrangement: no measurement trials, whose boundaries wait for the lanes)
        _loop(tsdr, ctx, iq, S, 8, submit)               # warm: workspaces, streams, kernels
        _, base_stats, ref = _loop(tsdr, ctx, iq, S, 8, submit)
        t0 = time.perf_counter()
        walls, stats, held = _loop(tsdr, ctx, iq, S, 8, submit, hold_ms=700)
        total = time.perf_counter() - t0
        # calls 0 .. 2 wait for nothing that is held (their decisions fold entries of earlier, complete calls); call 3 needs the
        # entry of call 0, which sits behind the hold: 50 ms, uncounted; the ones after it give up after 2 ms each
        assert max(walls) < 0.100, f"a frame-loop call took {max(walls) * 1e3:.1f} ms while its stream was held: {walls}"
        assert sum(walls) < 0.250, walls
        assert stats[1] - base_stats[1] >= 1, f"no guard entry went uncounted: {stats} vs {base_stats}"
        assert total > 0.5, "the hold did not hold"
        for (fa, ia), (fb, ib) in zip(ref, held):        # the held calls' results are the un-held ones
            assert np.array_equal(fa, fb) and np.array_equal(ia, ib)
        # and the route recovers: a later run folds its entries again without further uncounted ones
        _, after, again = _loop(tsdr, ctx, iq, S, 8, submit)
        _, after2, _ = _loop(tsdr, ctx, iq, S, 8, submit)
        assert after2[1] == after[1], (after, after2)
        for (fa, ia), (fb, ib) in zip(ref, again):
            assert np.array_equal(fa, fb) and np.array_equal(ia, ib)
    finally:
        ctx.close()


def test_synchronize_gives_up_after_wait_ms_and_says_where(tsdr):
    ctx = tsdr.Context(0)
    try:
        ctx.synchronize()
        ctx.set_option("wait_ms", 100)
        ctx.call("tsdr_debug_hold_stream", 800)
        t0 = time.perf_counter()
        with pytest.raises(tsdr.TempestHIPError) as e:
            ctx.synchronize()
        dt = time.perf_counter() - t0
        assert 0.08 < dt < 0.4, dt
        assert "bounded host wait" in str(e.value) and "100 ms" in str(e.value), str(e.value)
        assert ctx.wait_stats()[0] == 1
        time.sleep(0.9)
        ctx.set_option("wait_ms", 30000)
        ctx.synchronize()                                 # the hold is over: the context works as before
        y = ctx.amDemod((np.ones(1000) * (3 + 4j)).astype(np.complex64))
        assert np.array_equal(y, np.full(1000, 5.0, np.float32))
    finally:
        ctx.close()


def test_host_forms_give_up_or_finish_while_the_stream_is_held(tsdr):
    """The host-pointer forms behind a held stream (csrc/host_stage.h): vsync (its index pair lands in the context's pinned
    block), download of 4 KiB, circshift_neg on 8 x 20 (host_map).  Each either raises after "wait_ms" -- its copies stay enqueued:
    the caller's arrays are kept alive here until a later synchronize succeeds, as tempest_hip.h asks -- or returns the right data
    once the hold has passed.  Afterwards the context works, and the same calls on fresh objects give the un-held values."""
    import ctypes as C

    import sync_cases as SC
    from tempestsdr_jl_amd import api
    HOLD, BOUND = 0.6, 0.1
    img = SC.image("noise", 8, 20).ravel(order="F").copy()
    payload = np.arange(1024, dtype=np.float32)
    keep = []   # every array a call was handed, until the stream has completed

    def three(ctx, sync, d_payload):
        """-> [(value or None when the call gave up, seconds)] of the three calls"""
        def vsync():
            sy, sx = C.c_int(0), C.c_int(0)
            api.check(ctx.h, ctx.lib.tsdr_vsync(sync.h, api._ptr(img), C.byref(sy), C.byref(sx)), "tsdr_vsync")
            return sy.value, sx.value

        def download():
            out = np.zeros_like(payload)
            keep.append(out)
            ctx.call("tsdr_download", api._ptr(out), C.c_void_p(d_payload), out.nbytes)
            return out.tobytes()

        def circshift():
            out = np.zeros_like(img)
            keep.append(out)
            ctx.call("tsdr_circshift_neg", api._ptr(img), 8, 20, 3, 7, api._ptr(out))
            return out.tobytes()

        res = []
        for fn in (vsync, download, circshift):
            t0 = time.perf_counter()
            try:
                val = fn()
            except tsdr.TempestHIPError as e:
                assert "bounded host wait" in str(e), str(e)
                val = None
            res.append((val, time.perf_counter() - t0))
        return res

    ctx = tsdr.Context(0)
    syncs = [tsdr.SyncXY(ctx, 8, 20) for _ in range(4)]
    d_payload = ctx.upload(payload)
    try:
        three(ctx, syncs[0], d_payload)                              # warm: workspaces, the pinned block, kernels
        want = [v for v, _ in three(ctx, syncs[1], d_payload)]
        assert None not in want and want[1] == payload.tobytes()
        ctx.synchronize()
        ctx.set_option("wait_ms", int(BOUND * 1000))
        ctx.call("tsdr_debug_hold_stream", int(HOLD * 1000))
        held = three(ctx, syncs[2], d_payload)
        gave_up = sum(v is None for v, _ in held)
        for (v, dt), w in zip(held, want):
            assert v is None or v == w
            assert dt < HOLD + BOUND + 0.5, held
        assert ctx.wait_stats()[0] == gave_up
        time.sleep(HOLD + 0.1)
        ctx.set_option("wait_ms", 30000)
        ctx.synchronize()                                            # the hold is over: every copy left enqueued has landed
        assert [v for v, _ in three(ctx, syncs[3], d_payload)] == want
        assert ctx.wait_stats()[0] == gave_up
    finally:
        for s in syncs:
            s.close()
        ctx.synchronize()
        ctx.dev_free(d_payload)
        ctx.close()


def test_destroy_abandons_a_context_whose_stream_is_stuck(tsdr):
    """tsdr_destroy on a context whose stream does not complete within "wait_ms" returns (the context is abandoned: hipFree
    would wait for the device without a bound) instead of holding the caller."""
    ctx = tsdr.Context(0)
    ctx.set_option("wait_ms", 50)
    ctx.call("tsdr_debug_hold_stream", 600)
    t0 = time.perf_counter()
    ctx.close()
    assert time.perf_counter() - t0 < 0.3
    time.sleep(0.7)
