"""Float64 getWelch / getWaterfall / init_resampler on the MI355X (tsdr_welch_f64*, tsdr_waterfall_f64*,
tsdr_resampler_*_f64*): against the complex128 restatement (f64_spec_ref.py), at bars an f32 path cannot meet; edge cases and
error contract; and the f32 paths computing exactly what they compute on a fresh context while f64 calls interleave."""
import ctypes as C

import numpy as np
import pytest

import f64_spec_ref as S

pytestmark = pytest.mark.gpu

rng = np.random.default_rng(4096)
F64 = np.float64
EINVAL = -1
# the f32 test's sizes (test_fft_path_gpu.py), including the Bluestein (17) and chunked (8192) routes
SIZES = [1024, 1000, 256, 2, 6, 17, 4096, 3000, 2048, 960, 8192, 128, 512, 1200, 4000]


def _sig(n, cplx):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n) if cplx else rng.standard_normal(n)


def _check_welch(ctx, x, N):
    f, lin = ctx.getWelch(1.0, x, N, lin=True, dtype=F64)
    _, db = ctx.getWelch(1.0, x, N, dtype=F64)
    want = S.welch(x, N, lin=True)
    assert lin.dtype == F64 and db.dtype == F64 and lin.shape == (N,)
    scale = np.max(want)
    assert np.max(np.abs(lin - want)) <= 1e-12 * scale, (N, np.max(np.abs(lin - want)) / scale)
    big = want >= 1e-3 * scale
    assert np.max(np.abs(db[big] - 10 * np.log10(want[big]))) <= 1e-8, N


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("N", SIZES)
def test_welch_waterfall_f64(ctx, N, cplx):
    x = _sig(37 * N + N // 3 + 1, cplx)   # ragged tail
    _check_welch(ctx, x, N)
    t, fa, m = ctx.getWaterfall(2.0, x, N, dtype=F64)
    want = S.waterfall(x, N)
    assert m.dtype == F64 and m.shape == (N, 37) and m.flags.f_contiguous
    assert np.max(np.abs(m - want)) <= 1e-12 * np.max(want)
    assert np.allclose(t, np.arange(37) * (N / 2.0))


@pytest.mark.parametrize("N", [2, 6, 17, 128])
def test_welch_many_segments_small_sizes(ctx, N):
    x = _sig(5000 * N + 1, True)   # several tiles per workgroup / several chunks
    _check_welch(ctx, x, N)
    _, _, m = ctx.getWaterfall(1.0, x, N, dtype=F64)
    assert np.max(np.abs(m - S.waterfall(x, N))) <= 1e-12 * np.max(m)


@pytest.mark.parametrize("N", [1024, 1000])
def test_welch_full_c2_size(ctx, N):
    x = _sig(10_000_000, True)   # 9765 / 10000 segments of a C2 capture
    _check_welch(ctx, x, N)
    if N == 1024:
        _, _, m = ctx.getWaterfall(1.0, x[: 1024 * 3000], N, dtype=F64)
        assert m.shape == (1024, 3000)
        assert np.max(np.abs(m - S.waterfall(x[: 1024 * 3000], N))) <= 1e-12 * np.max(m)


@pytest.mark.parametrize("N,k", [(1024, 37), (1000, 250), (17, 3)])
def test_precision_beyond_float32(ctx, N, k):
    """1 + 1e-9 e^(2 pi i k n / N): in Float32 the input itself rounds the tone away"""
    n = np.arange(64 * N)
    x = 1.0 + 1e-9 * np.exp(2j * np.pi * k * n / N)
    _, y = ctx.getWelch(1.0, x, N, lin=True, dtype=F64)
    want = S.welch(x, N, lin=True)
    j = (k + N // 2) % N
    assert abs(y[j] - want[j]) <= 1e-5 * want[j], (y[j], want[j])
    _, _, m = ctx.getWaterfall(1.0, x, N, dtype=F64)
    assert np.max(np.abs(m[j] - S.waterfall(x, N)[j])) <= 1e-5 * np.max(S.waterfall(x, N)[j])


def test_edge_cases(ctx, tsdr):
    x = _sig(100, True)
    _, lin = ctx.getWelch(1.0, x, 128, lin=True, dtype=F64)
    _, db = ctx.getWelch(1.0, x, 128, dtype=F64)
    assert np.array_equal(lin, np.zeros(128)) and np.all(np.isneginf(db))
    _, _, m = ctx.getWaterfall(1.0, x, 128, dtype=F64)
    assert m.shape == (128, 0) and m.dtype == F64
    with pytest.raises(Exception):
        ctx.getWelch(1.0, x, 0, dtype=F64)
    y = np.empty(4)
    assert ctx.lib.tsdr_welch_f64(ctx.h, x.ctypes.data_as(C.c_void_p), 1, x.size, 0, 0, y.ctypes.data_as(C.c_void_p)) == EINVAL
    assert ctx.lib.tsdr_waterfall_f64(ctx.h, x.ctypes.data_as(C.c_void_p), 1, x.size, 0, y.ctypes.data_as(C.c_void_p)) == EINVAL
    # type contract: float64 / complex128 only
    with pytest.raises(AssertionError):
        ctx.getWelch(1.0, x.astype(np.complex64), 16, dtype=F64)
    with pytest.raises(AssertionError):
        ctx.getWaterfall(1.0, x.real.astype(np.float32), 16, dtype=F64)
    # a misaligned ComplexF64 pointer to the _d forms
    d_in, d_out = ctx.dev_alloc(16 * 1024 + 16), ctx.dev_alloc(8 * 1024 * 2)
    try:
        assert ctx.lib.tsdr_welch_f64_d(ctx.h, C.c_void_p(d_in + 8), 1, 512, 256, 0, C.c_void_p(d_out)) == EINVAL
        assert ctx.lib.tsdr_waterfall_f64_d(ctx.h, C.c_void_p(d_in + 8), 1, 512, 256, C.c_void_p(d_out)) == EINVAL
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)


def test_device_forms_match_host_forms(ctx):
    x = _sig(20 * 1000 + 7, True)
    d_in = ctx.upload(x)
    d_y, d_m = ctx.dev_alloc(8 * 1000), ctx.dev_alloc(8 * 1000 * 20)
    try:
        assert ctx.lib.tsdr_welch_f64_d(ctx.h, C.c_void_p(d_in), 1, x.size, 1000, 1, C.c_void_p(d_y)) == 0
        assert ctx.lib.tsdr_waterfall_f64_d(ctx.h, C.c_void_p(d_in), 1, x.size, 1000, C.c_void_p(d_m)) == 0
        ctx.synchronize()
        y, m = ctx.download(d_y, (1000,), F64), ctx.download(d_m, (1000 * 20,), F64).reshape((1000, 20), order="F")
    finally:
        for p in (d_in, d_y, d_m):
            ctx.dev_free(p)
    assert np.array_equal(y, ctx.getWelch(1.0, x, 1000, lin=True, dtype=F64)[1])
    assert np.array_equal(m, ctx.getWaterfall(1.0, x, 1000, dtype=F64)[2])


# ---- resampler! in Float64 ---------------------------------------------------------------------------------------------
RESAMPLER_CASES = [(1024, 4), (1000, 4), (999, 3), (64, 2), (4096, 8), (100_000, 5), (625, 3), (10, 1), (4, 2), (250_000, 4),
                   (1_000_000, 4), (6, 1), (1218, 2), (3000, 7), (1021, 2)]


def _resampler_signal(bufferSize):
    if bufferSize == 1024:   # production/test_resampler.jl: Fs = 1e6, tones at 50 kHz and 20 kHz on a Float64 time range
        t = np.arange(bufferSize) / 1e6
        return np.cos(2 * np.pi * 50e3 * t) + 0.5 * np.sin(2 * np.pi * 20e3 * t)
    return rng.standard_normal(bufferSize)


@pytest.mark.parametrize("bufferSize,up", RESAMPLER_CASES)
def test_resampler_f64(ctx, bufferSize, up):
    r = ctx.init_resampler(np.float64, bufferSize, up)
    r32 = ctx.init_resampler(np.float32, bufferSize, up)
    N = bufferSize * up
    H = r.lpf64()
    assert np.array_equal(H.view(np.uint64), r32.lpf64().view(np.uint64))   # one filter: initLPF(Float64, ...)
    x = _resampler_signal(bufferSize)
    out = np.empty(N, F64)
    r(out, x)
    want = S.resampler(x, up, H)
    assert np.max(np.abs(out - want)) <= 1e-12 * max(1.0, np.log2(N)) * np.max(np.abs(want)), (bufferSize, up)
    with pytest.raises(AssertionError, match="should match size used during init"):
        r(out, x[:-1])
    with pytest.raises(AssertionError, match=r"should match type used during init \(Float64\)"):
        r(out.astype(np.float32), x.astype(np.float32))
    with pytest.raises(AssertionError):   # the Float32 closure keeps refusing float64 buffers
        r32(out, x)
    r.close()
    r32.close()


def test_resampler_handles_do_not_cross(ctx):
    r64, r32 = ctx.init_resampler(np.float64, 64, 2), ctx.init_resampler(np.float32, 64, 2)
    x64, o64 = np.zeros(64), np.zeros(128)
    x32, o32 = np.zeros(64, np.float32), np.zeros(128, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert ctx.lib.tsdr_resampler_run(C.c_void_p(r64.h), p(x32), 64, p(o32)) == EINVAL
    assert ctx.lib.tsdr_resampler_run_f64(C.c_void_p(r32.h), p(x64), 64, p(o64)) == EINVAL
    assert ctx.lib.tsdr_resampler_run_f64(C.c_void_p(r64.h), p(x64), 63, p(o64)) == EINVAL
    assert "should match size used during init" in ctx.lib.tsdr_last_error(ctx.h).decode()
    d_in, d_out = ctx.dev_alloc(64 * 8), ctx.dev_alloc(128 * 8)
    try:
        assert ctx.lib.tsdr_resampler_run_d(C.c_void_p(r64.h), C.c_void_p(d_in), 64, C.c_void_p(d_out)) == EINVAL
        assert ctx.lib.tsdr_resampler_run_f64_d(C.c_void_p(r32.h), C.c_void_p(d_in), 64, C.c_void_p(d_out)) == EINVAL
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)
    assert r64.lpf().dtype == np.complex64 and np.array_equal(r64.lpf(), r32.lpf())
    with pytest.raises(AssertionError):
        ctx.init_resampler(np.int32, 64, 2)
    r64.close()
    r32.close()


def test_f32_paths_unchanged_beside_f64_calls(ctx, tsdr):
    """f32 Welch / waterfall / resampler on the shared context with f64 calls in between equal a fresh context's bit for bit"""
    x32 = (rng.standard_normal(50 * 1024 + 5) + 1j * rng.standard_normal(50 * 1024 + 5)).astype(np.complex64)
    x64 = x32.astype(np.complex128)
    xr = rng.standard_normal(1000).astype(np.float32)

    def f32_run(c, interleave):
        outs = []
        r = c.init_resampler(np.float32, 1000, 4)
        r64 = c.init_resampler(np.float64, 1000, 4)
        for N in (1024, 1000, 17, 8192):
            if interleave:
                c.getWelch(1.0, x64, N, dtype=F64)
            outs.append(c.getWelch(1.0, x32, N)[1])
            if interleave:
                c.getWaterfall(1.0, x64, N, dtype=F64)
            outs.append(c.getWaterfall(1.0, x32, N)[2])
            if interleave:
                o = np.empty(4000)
                r64(o, xr.astype(F64))
            o32 = np.empty(4000, np.float32)
            r(o32, xr)
            outs.append(o32)
        r.close()
        r64.close()
        return outs

    fresh = tsdr.Context(0)
    try:
        want = f32_run(fresh, False)
    finally:
        fresh.close()
    got = f32_run(ctx, True)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes("F") == b.tobytes("F")


def test_module_level_wrappers_take_dtype(tsdr):
    import importlib
    api = importlib.import_module("tempestsdr_jl_amd.api")
    x = _sig(4 * 256, False)
    assert api.getWelch(1.0, x, 256, dtype=F64)[1].dtype == F64
    assert api.getWaterfall(1.0, x, 256, dtype=F64)[2].shape == (256, 4)
