"""GPU tests of the 8-bit I/Q input (TSDR_IQ_SC8 / TSDR_IQ_UC8) and the generic entry points tsdr_frames_iq_d,
tsdr_frames_submit_iq_d and tsdr_autocorr_search_iq_d.  What 8-bit SDR hardware delivers -- int8 pairs (HackRF, UHD sc8), or
uint8 pairs around 127.5 (RTL-SDR) -- goes into the image kernels and the search's first pass as it is; every sample becomes
ComplexF32 by ONE f32 product in the loaders (tests/iq8_ref.py).  The bar is bit-identity, no tolerance anywhere: rasters,
frames, IIR state, sync indices, lag vectors, findmax position and value equal those of the ComplexF32 entry points on the
samples expanded on the host with the same product, on every route that reads IQ."""
import importlib

import numpy as np
import pytest

import iq8_ref as R

pytestmark = pytest.mark.gpu

NPX = 600 * 800


def _capture(synth, fmt, Fs, x_t, y_t, fv, n, card="box"):
    z = synth.synth_leak(Fs, x_t, y_t, fv, n, card=card)
    q, scale = R.quantise(z, fmt)
    return q, scale, R.expand(q, fmt, scale)


def _restart_guard_window(ctx, auto):
    """both routes of a comparison start from the same adaptive-route state (tests/conftest.py does this between tests)"""
    ctx.set_option("sync_guard_ppb", 20000)
    ctx.set_option("sync_guard_auto", auto)


def _run(ctx, tsdr, cf, q, fmt, scale, S, y_t, x_t, want_raster, pipelined=False, nsplit=1, lead=0, auto=1, ref="cf32"):
    """The same frames through the ComplexF32 entry point on the expanded samples (ref "cf32"; "named": the format's own
    named entry point on the raw ones) and through tsdr_frames_iq_d / _submit_iq_d on the raw ones, in `nsplit` calls.
    lead: samples in front of the first frame in the device buffer (1: every call with an even frame offset starts at an odd
    sample, byte offset 2 mod 4 for the 8-bit formats)."""
    api = importlib.import_module("tempestsdr_jl_amd.api")
    P = x_t * y_t
    nb = cf.size // S
    bps = R.BYTES[fmt]
    out, odd_starts = {}, 0
    for name in ("ref", "iq"):
        raw = name == "iq" or ref == "named"
        _restart_guard_window(ctx, auto)
        sync = tsdr.SyncXY(ctx, 600, 800)
        d_state = ctx.upload(np.zeros(NPX, np.float32))
        host = q if raw else cf.view(np.float32)
        pad = np.zeros(2 * lead, host.dtype)
        d_in = ctx.upload(np.concatenate([pad, host]))
        d_fr, d_ix = ctx.dev_alloc(nb * NPX * 4), ctx.dev_alloc(nb * 8)
        d_ra = ctx.dev_alloc(nb * P * 4) if want_raster else None
        try:
            per = nb // nsplit
            for c in range(nsplit):
                cnt = per if c < nsplit - 1 else nb - per * (nsplit - 1)
                first = lead + c * per * S                      # first sample of this call
                o_in = d_in + first * (bps if raw else 8)
                fr, ix = d_fr + c * per * NPX * 4, d_ix + c * per * 8
                ra = d_ra + c * per * P * 4 if want_raster else None
                if name == "iq":
                    odd_starts += (first * bps) % 4 == 2
                    n = api.frames_iq_d(ctx, sync, o_in, fmt, scale, cnt * S, S, y_t, x_t, np.float32(0.1), True, d_state, fr, ra, ix,
                                        submit=pipelined)
                elif ref == "named":
                    assert fmt == "sc16"
                    n = api.frames_sc16_d(ctx, sync, o_in, scale, cnt * S, S, y_t, x_t, np.float32(0.1), True, d_state, fr, ra, ix,
                                          submit=pipelined)
                else:
                    f = api.frames_submit_d if pipelined else api.frames_d
                    n = f(ctx, sync, o_in, cnt * S, S, y_t, x_t, np.float32(0.1), True, d_state, fr, ra, ix)
                assert n == cnt
            ctx.synchronize()
            out[name] = (ctx.download(d_fr, (nb * NPX,), np.uint32), ctx.download(d_ix, (nb * 2,), np.int32),
                         ctx.download(d_state, (NPX,), np.uint32),
                         ctx.download(d_ra, (nb * P,), np.uint32) if want_raster else np.zeros(0, np.uint32))
        finally:
            sync.close()
            for p in (d_state, d_in, d_fr, d_ix, d_ra):
                if p is not None:
                    ctx.dev_free(p)
    for what, a, b in zip(("frames", "sync_idx", "state", "raster"), out["ref"], out["iq"]):
        assert np.array_equal(a, b), what
    assert np.any(out["iq"][0]), "the frames are not all zero"
    return out["iq"], odd_starts


GEOMS = [(2.0e6, 1056, 628, 5), (20e6, 2576, 1125, 3), (2.0e6, 900, 590, 2)]   # tests/test_sc16_gpu.py's


@pytest.mark.parametrize("fmt", ["sc8", "uc8"])
@pytest.mark.parametrize("precision", ["fast", "exact"])
@pytest.mark.parametrize("want_raster", [True, False])
@pytest.mark.parametrize("geom", GEOMS)
def test_iq8_frames_equal_cf32_frames(ctx, tsdr, synth, fmt, precision, want_raster, geom):
    Fs, x_t, y_t, nfr = geom                      # (590 lines < 600: no in-walk downgrade -- the run-time-format kernels)
    S = synth.samples_per_frame(Fs, 60.0)
    q, scale, cf = _capture(synth, fmt, Fs, x_t, y_t, 60.0, S * nfr + 11)
    ctx.set_precision(precision)
    try:
        _run(ctx, tsdr, cf, q, fmt, scale, S, y_t, x_t, want_raster)
    finally:
        ctx.set_precision("fast")


@pytest.mark.parametrize("fmt", ["sc8", "uc8"])
@pytest.mark.parametrize("precision", ["fast", "exact"])
@pytest.mark.parametrize("want_raster", [True, False])
@pytest.mark.parametrize("geom", GEOMS)
def test_iq8_calls_that_start_at_an_odd_sample(ctx, tsdr, synth, fmt, precision, want_raster, geom):
    """Frame f of an 8-bit buffer starts at byte 2*f*S: nothing wider than 2 bytes is aligned.  One sample in front of the
    buffer and a split into two calls: the first call (and, S even, the second) starts at byte offset 2 mod 4; with an odd S the
    frames inside a call alternate as well."""
    Fs, x_t, y_t, nfr = geom
    nfr = max(nfr, 4)
    S = synth.samples_per_frame(Fs, 60.0)
    q, scale, cf = _capture(synth, fmt, Fs, x_t, y_t, 60.0, S * nfr)
    ctx.set_precision(precision)
    try:
        _, odd = _run(ctx, tsdr, cf, q, fmt, scale, S, y_t, x_t, want_raster, nsplit=2, lead=1)
        assert odd >= 1
    finally:
        ctx.set_precision("fast")


@pytest.mark.parametrize("fmt", ["sc8", "uc8"])
def test_iq8_through_the_sync_guard_and_the_pipeline(ctx, tsdr, synth, fmt):
    """The plateau leak is a near-tie card and flags most frames: the guard's exact re-evaluation reads the 8-bit samples too
    (one by one with "sync_guard_auto" 0, whole exact buffers with it on), and the pipelined submission takes the same
    loaders -- here from calls that start at odd samples."""
    Fs, x_t, y_t, nfr = 2.0e6, 1056, 628, 12
    S = synth.samples_per_frame(Fs, 60.0)
    q, scale, cf = _capture(synth, fmt, Fs, x_t, y_t, 60.0, S * nfr, card="plateau")
    for auto in (0, 1):
        ctx.sync_guard_stats(reset=True)
        try:
            _, odd = _run(ctx, tsdr, cf, q, fmt, scale, S, y_t, x_t, False, pipelined=True, nsplit=4, lead=1, auto=auto)
            checked, flagged = ctx.sync_guard_stats()
            assert flagged > 0, "the plateau leak should have flagged frames"
            assert odd >= 1
        finally:
            ctx.set_option("sync_guard_auto", 1)


@pytest.mark.parametrize("fmt", ["sc8", "uc8"])
def test_iq8_guard_beyond_one_guard_launch(ctx, tsdr, synth, fmt):
    """More than kGuardChunk = 256 frames in one call: the guard's later launches must find their frames' samples at
    f0 * S * 2 bytes.  The plateau leak flags frames in every launch's range."""
    Fs, x_t, y_t, nfr = 2.0e6, 1056, 628, 300
    S = synth.samples_per_frame(Fs, 60.0)
    q, scale, cf = _capture(synth, fmt, Fs, x_t, y_t, 60.0, S * nfr, card="plateau")
    ctx.sync_guard_stats(reset=True)
    try:
        _run(ctx, tsdr, cf, q, fmt, scale, S, y_t, x_t, False, auto=0)
        checked, flagged = ctx.sync_guard_stats()
        assert checked == 2 * nfr and flagged > 2      # (two runs: expanded and raw)
    finally:
        ctx.set_option("sync_guard_auto", 1)


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("precision", ["fast", "exact"])
def test_generic_entry_equals_the_named_entries(ctx, tsdr, synth, precision, pipelined):
    """iq_fmt TSDR_IQ_SC16 is tsdr_frames_sc16_d, TSDR_IQ_CF32 is tsdr_frames_d (scale ignored), bit for bit"""
    Fs, x_t, y_t, nfr = 2.0e6, 1056, 628, 4
    S = synth.samples_per_frame(Fs, 60.0)
    q, scale, cf = _capture(synth, "sc16", Fs, x_t, y_t, 60.0, S * nfr)
    ctx.set_precision(precision)
    try:
        for want_raster in (True, False):
            _run(ctx, tsdr, cf, q, "sc16", scale, S, y_t, x_t, want_raster, pipelined=pipelined, ref="named")
            _run(ctx, tsdr, cf, q, "sc16", scale, S, y_t, x_t, want_raster, pipelined=pipelined)      # and the expanded samples
            _run(ctx, tsdr, cf, cf.view(np.float32), "cf32", np.float32(123.0), S, y_t, x_t, want_raster, pipelined=pipelined)
    finally:
        ctx.set_precision("fast")


_PINNED = {}      # (fmt, want_raster) -> the capture and what one tsdr_frames_iq_d per buffer returns for it


def _pinned_case(tsdr, synth, fmt, want_raster):
    """4 buffers of 2 frames + 7 samples each at 2 MS/s, 1056 x 628 at 60 Hz, and their reference: one tsdr_frames_iq_d per
    buffer on a context and a SyncXY of its own.  Computed once per (format, rasters or not), shared by the eight arrangements."""
    if (fmt, want_raster) not in _PINNED:
        Fs, x_t, y_t, nfr, nbuf = 2.0e6, 1056, 628, 2, 4
        S = synth.samples_per_frame(Fs, 60.0)
        nEch = nfr * S + 7
        q, scale = R.quantise(synth.synth_leak(Fs, x_t, y_t, 60.0, nbuf * nEch), fmt)
        case = dict(fmt=fmt, q=q, scale=scale, S=S, nEch=nEch, x_t=x_t, y_t=y_t, nfr=nfr, nbuf=nbuf, want_raster=want_raster)
        ref = tsdr.Context(0)
        try:
            assert ref.precision == "fast"
            case["want"] = _four_buffers(ref, tsdr, case, submit=False)
        finally:
            ref.close()
        for a in case["want"] + (q,):
            a.setflags(write=False)
        _PINNED[(fmt, want_raster)] = case
    return _PINNED[(fmt, want_raster)]


def _four_buffers(ctx, tsdr, case, submit):
    """-> (frames, rasters, sync_idx, final state) of the case's buffers through tsdr_frames_iq_d or tsdr_frames_submit_iq_d + flush"""
    api = importlib.import_module("tempestsdr_jl_amd.api")
    S, nEch, x_t, y_t, nfr, nbuf, fmt = (case[k] for k in ("S", "nEch", "x_t", "y_t", "nfr", "nbuf", "fmt"))
    P, bps = x_t * y_t, R.BYTES[fmt]
    sync = tsdr.SyncXY(ctx, 600, 800)
    d_in, d_state = ctx.upload(case["q"]), ctx.upload(np.zeros(NPX, np.float32))
    d_fr, d_ix = ctx.dev_alloc(nbuf * nfr * NPX * 4), ctx.dev_alloc(nbuf * nfr * 8)
    d_ra = ctx.dev_alloc(nbuf * nfr * P * 4) if case["want_raster"] else None
    try:
        for b in range(nbuf):
            n = api.frames_iq_d(ctx, sync, d_in + b * nEch * bps, fmt, case["scale"], nEch, S, y_t, x_t, np.float32(0.1), True, d_state,
                                d_fr + b * nfr * NPX * 4, d_ra + b * nfr * P * 4 if d_ra is not None else None, d_ix + b * nfr * 8,
                                submit=submit)
            assert n == nfr
        if submit:
            api.frames_flush(ctx)
        ctx.synchronize()
        return (ctx.download(d_fr, (nbuf * nfr * NPX,), np.uint32),
                ctx.download(d_ra, (nbuf * nfr * P,), np.uint32) if d_ra is not None else np.zeros(0, np.uint32),
                ctx.download(d_ix, (nbuf * nfr * 2,), np.int32), ctx.download(d_state, (NPX,), np.uint32))
    finally:
        sync.close()
        for p in (d_in, d_state, d_fr, d_ix, d_ra):
            if p is not None:
                ctx.dev_free(p)


@pytest.mark.parametrize("pin", range(8))
@pytest.mark.parametrize("want_raster", [True, False])
@pytest.mark.parametrize("fmt", ["sc16", "uc8"])
def test_integer_iq_through_every_pinned_arrangement(ctx, tsdr, synth, fmt, want_raster, pin):
    """An integer format reaches the pipeline's arrangements other than the default choice only when one is pinned.  Every
    "pipe_pin" 0...7 (one stream, image lane + tail lane on three stream pairs, two equal lanes on three pairs, three equal lanes),
    four buffers so that the three slots wrap, FAST with do_align: tsdr_frames_submit_iq_d + flush equals one tsdr_frames_iq_d
    per buffer on a fresh context and SyncXY, bit for bit -- frames, rasters, sync indices and the final state."""
    case = _pinned_case(tsdr, synth, fmt, want_raster)
    assert ctx.precision == "fast"
    _restart_guard_window(ctx, 1)
    ctx.set_option("pipe_pin", pin)
    try:
        got = _four_buffers(ctx, tsdr, case, submit=True)
        info = ctx.pipeline_info()
        assert info["chosen"] == pin and "pinned" in info["text"], info
    finally:
        ctx.set_option("pipe_pin", -1)
    for what, a, b in zip(("frames", "raster", "sync_idx", "state"), case["want"], got):
        assert a.size == b.size and np.array_equal(a, b), what
    assert np.any(got[0]) and np.any(got[3]), "frames and state are not all zero"


# (Fs, maxDelay, samples): n = min(2 * round(maxDelay * Fs), samples)
SEARCH_LENGTHS = {
    "pow2": (1048576.0, 0.5, 1 << 20),              # n = 2^20: the power-of-two route, first pass loader
    "reference_20MSps": (20e6, 0.1, 4_000_000),     # n = 2 * round(0.1 * Fs) = 4e6: the mixed-radix route (GUI.jl:60)
    "ac_pack": (1000.0, 0.1, 200),                  # n = 200: k_ac_pack (single-pass transform)
    "padded": (500010.0, 0.1, 100_002),             # n = 2 * 50001, 50001 = 3 * 7 * 2381: zero-padded power of two
}


@pytest.mark.parametrize("fmt", ["sc16", "sc8", "uc8"])
@pytest.mark.parametrize("length", list(SEARCH_LENGTHS))
def test_search_on_raw_iq_equals_search_on_expanded_iq(ctx, tsdr, synth, fmt, length):
    Fs, max_delay, n = SEARCH_LENGTHS[length]
    z = synth.synth_leak(20e6, 2576, 1125, 60.0, n)
    q, scale = R.quantise(z, fmt)
    cf = R.expand(q, fmt, scale)
    for log in ("log", "lin"):
        G0, pos0, val0 = ctx.autocorr_search(cf, Fs, 0, max_delay, scale=log)                 # tsdr_autocorr_search_d(is_iq = 1)
        G1, pos1, val1 = ctx.autocorr_search(q, Fs, 0, max_delay, scale=log, iq_fmt=fmt, iq_scale=scale)
        assert G0.size == G1.size == int(round(max_delay * Fs))
        assert np.array_equal(G0.view(np.uint32), G1.view(np.uint32)), f"lag vector ({log})"
        assert pos0 == pos1 and np.float32(val0).view(np.uint32) == np.float32(val1).view(np.uint32)
        assert np.isfinite(G1).any() and np.any(G1 != 0)


def test_end_to_end_from_one_sc8raw_ring(ctx, tsdr, synth):
    """extract_configuration (GUI.jl:49-88) and the frame loop take their buffers from the same ring: a C2 leak quantised to 8
    bits goes through a "sc8raw" ring into the search and the frame loop without ever being expanded.  The refresh lag equals the
    one found on the unquantised capture: 333037 (float64 numpy autocorrelation of the ComplexF32 capture, of its 12-bit and of its
    8-bit quantisation, 50-90 Hz window)."""
    api = importlib.import_module("tempestsdr_jl_amd.api")
    search = importlib.import_module("tempestsdr_jl_amd.search")
    Fs, x_t, y_t = 20e6, 2576, 1125
    z = synth.synth_leak(Fs, x_t, y_t, 60.0, 4_000_000)
    q, scale = R.quantise(z, "sc8")
    assert scale == np.float32(float(np.max(np.abs(z.view(np.float32)))) / 127.0)
    _, _, fv_ref, G_ref = search.extract_configuration(ctx, z, Fs)
    ring = tsdr.StagingRing(ctx, z.size, 2, fmt="sc8raw", scale=float(scale))
    sync = tsdr.SyncXY(ctx, 600, 800)
    S = synth.samples_per_frame(Fs, 60.0)
    nfr = z.size // S
    d_state, d_fr, d_ix = ctx.upload(np.zeros(NPX, np.float32)), ctx.dev_alloc(nfr * NPX * 4), ctx.dev_alloc(nfr * 8)
    try:
        ring.put(q)
        d = ring.take_d(5000)
        assert np.array_equal(ctx.download(d, (2 * z.size,), np.int8), q)
        _, _, fv, G = search.extract_configuration(ctx, d, Fs, iq_fmt=ring.iq_fmt, iq_scale=scale, n_samples=z.size)
        # (zoom_autocorr labels lag k with index k + 1 -- the reference's off-by-one, kept: fv = Fs / (lag + 1))
        lag, lag_ref = int(round(Fs / fv)) - 1, int(round(Fs / fv_ref)) - 1
        print("refresh lag: 8-bit", lag, "unquantised", lag_ref)
        assert lag == lag_ref == 333037
        assert fv == fv_ref and G.size == G_ref.size
        _restart_guard_window(ctx, 1)
        n = api.frames_iq_d(ctx, sync, d, ring.iq_fmt, scale, z.size, S, y_t, x_t, np.float32(0.1), True, d_state, d_fr, None, d_ix)
        ctx.synchronize()
        assert n == nfr
        got = ctx.download(d_fr, (nfr * NPX,), np.uint32)
        _restart_guard_window(ctx, 1)
        sync2 = tsdr.SyncXY(ctx, 600, 800)
        want = ctx.frames(sync2, R.expand(q, "sc8", scale), S, y_t, x_t, np.float32(0.1), np.zeros((600, 800), np.float32, order="F"))
        sync2.close()
        for f in range(nfr):
            assert np.array_equal(got[f * NPX:(f + 1) * NPX], np.asarray(want["frames"][f]).reshape(-1, order="F").view(np.uint32)), f
    finally:
        sync.close()
        ring.close()
        for p in (d_state, d_fr, d_ix):
            ctx.dev_free(p)


@pytest.mark.parametrize("fmt", ["sc8", "uc8"])
def test_ring_8bit_formats(ctx, tsdr, fmt):
    """fmt 3 / 5 hand out the ComplexF32 product, 4 / 6 the stored bytes unchanged (odd and even slot lengths); a full ring
    overwrites the oldest buffer and counts it, as for fmt 0-2."""
    rng = np.random.default_rng(11)
    scale = np.float32(1.0 / 127.0)
    def same(d, b, raw, nEch):
        ctx.synchronize()
        if raw:
            return np.array_equal(ctx.download(d, (2 * nEch,), R.DTYPES[fmt]), b)
        return np.array_equal(ctx.download(d, (2 * nEch,), np.uint32), R.expand(b, fmt, scale).view(np.uint32))

    for nEch in (4096, 4097):
        bufs = [rng.integers(0, 256, 2 * nEch).astype(np.uint8).view(R.DTYPES[fmt]) for _ in range(5)]
        bufs[0][:4] = np.array([0, 255, 127, 128], np.uint8).view(R.DTYPES[fmt])      # the extreme codes
        for raw in (False, True):
            name = fmt + ("raw" if raw else "")
            ring = tsdr.StagingRing(ctx, nEch, 3, fmt=name, scale=float(scale))
            try:
                for b in bufs[:2]:
                    ring.put(b)
                for k in range(2):
                    assert same(ring.take_d(1000), bufs[k], raw, nEch), (name, nEch, k)
                st = ring.stats()
                assert (st["produced"], st["consumed"], st["overflow"]) == (2, 2, 0)
                with pytest.raises(IndexError):
                    ring.take_d(20)
                with pytest.raises(AssertionError):
                    ring.put(np.zeros(2 * nEch, np.int16))
            finally:
                ring.close()
            # depth 3, five puts before the first take: the consumer sees 3, 4, 2 and two overflows are counted
            # (tests/test_ring_gpu.py: the reference's order under overflow)
            ring = tsdr.StagingRing(ctx, nEch, 3, fmt=name, scale=float(scale))
            try:
                for b in bufs:
                    ring.put(b)
                for k in (3, 4, 2):
                    assert same(ring.take_d(1000), bufs[k], raw, nEch), (name, nEch, k)
                assert ring.stats()["overflow"] == 2
            finally:
                ring.close()


def test_unknown_format_and_misaligned_base_are_refused(ctx, tsdr, synth):
    """TSDR_EINVAL, and the context goes on working"""
    import ctypes as C
    Fs, x_t, y_t = 2.0e6, 1056, 628
    S = synth.samples_per_frame(Fs, 60.0)
    q, scale, cf = _capture(synth, "sc8", Fs, x_t, y_t, 60.0, 2 * S + 8)
    lib = ctx.lib
    sync = tsdr.SyncXY(ctx, 600, 800)
    d_in, d_state, d_fr, d_ix = ctx.upload(q), ctx.upload(np.zeros(NPX, np.float32)), ctx.dev_alloc(2 * NPX * 4), ctx.dev_alloc(16)
    d_out = ctx.dev_alloc(4 * 100)
    EINVAL = -1
    try:
        n = C.c_int(0)

        def frames(fn, ptr, code):
            return getattr(lib, fn)(ctx.h, sync.h, C.c_void_p(ptr), code, C.c_float(scale), 2 * S, S, y_t, x_t, C.c_float(0.1), 1,
                                    C.c_void_p(d_state), C.c_void_p(d_fr), None, C.c_void_p(d_ix), C.byref(n))

        def srch(ptr, code):
            no, idx, val = C.c_size_t(0), C.c_size_t(0), C.c_float(0)
            return lib.tsdr_autocorr_search_iq_d(ctx.h, C.c_void_p(ptr), code, C.c_float(scale), 200, 1000.0, 0.0, 0.1, 1,
                                                 C.c_void_p(d_out), C.byref(no), 10, 10, C.byref(idx), C.byref(val))

        assert lib.tsdr_strerror(EINVAL).lower().startswith(b"invalid")
        for fn in ("tsdr_frames_iq_d", "tsdr_frames_submit_iq_d"):
            for code in (-1, 4, 99):
                assert frames(fn, d_in, code) == EINVAL
            assert frames(fn, d_in + 1, R.CODES["sc8"]) == EINVAL      # not a multiple of one sample (2 bytes)
            assert frames(fn, d_in + 2, R.CODES["sc16"]) == EINVAL     # ... (4 bytes)
            assert frames(fn, d_in + 4, R.CODES["cf32"]) == EINVAL     # ... (8 bytes)
        for code in (-1, 4):
            assert srch(d_in, code) == EINVAL
        for code in (R.CODES["sc16"], R.CODES["sc8"], R.CODES["uc8"]):
            assert srch(d_in + 8, code) == EINVAL                       # integer IQ: 16-byte aligned base
        assert srch(d_in, R.CODES["sc8"]) == 0
        # the context is as usable as before
        assert frames("tsdr_frames_iq_d", d_in + 2, R.CODES["sc8"]) == 0 and n.value == 2
        ctx.synchronize()
        _run(ctx, tsdr, cf[:2 * S], q[:4 * S], "sc8", scale, S, y_t, x_t, False)
    finally:
        sync.close()
        for p in (d_in, d_state, d_fr, d_ix, d_out):
            ctx.dev_free(p)
