"""Float64 / ComplexF64 per-function API on the MI355X (the `_f64` entry points): bit-exact against the numpy restatement
(f64_ref.py) where the contract says so, within the stated ulp / relative bars elsewhere, and, on f32-representable input,
float32(f64 result) bit-identical to the f32 oracle.  Plus: f32 callers see no change, and f32 / f64 sync states refuse
each other's entry points."""
import ctypes as C
import importlib

import numpy as np
import pytest

import f64_ref as R
import oracle_lib as O
from test_frame_path_gpu import RASTER_CASES

pytestmark = pytest.mark.gpu

rng = np.random.default_rng(6464)
F64 = np.float64


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return np.array_equal(np.asfortranarray(a).ravel(order="F").view(np.uint64), np.asfortranarray(b).ravel(order="F").view(np.uint64))


def _ulps(a, b):
    """largest distance in units in the last place between two float64 arrays (equal values, +-0 and NaN pairs count 0;
    values of opposite sign that are not equal count as far apart)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ia, ib = a.view(np.int64), b.view(np.int64)
    d = np.where((ia < 0) == (ib < 0), np.abs(ia - ib), np.int64(1) << 62)
    d = np.where((a == b) | np.isnan(a), 0, d)
    return int(np.max(d)) if d.size else 0


def _cplx(n, scale=1.0):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale


SPECIALS = [0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 1.0, -3.5, 1e300, -1e300, 1.7e308,
            np.inf, -np.inf, np.nan]


# ---- demodulation ----------------------------------------------------------------------------------------------------
def test_am_demod_f64_within_1ulp_of_hypot(ctx):
    z = _cplx(1_000_003)
    got = ctx.amDemod(z, dtype=F64)
    assert got.dtype == F64
    assert _ulps(got, np.hypot(z.real, z.imag)) <= 1


def test_am_demod_f64_specials(ctx):
    re, im = np.meshgrid(SPECIALS, SPECIALS)
    z = np.empty(re.size, np.complex128)
    z.real, z.imag = re.ravel(), im.ravel()
    got = ctx.amDemod(z, dtype=F64)
    want = np.hypot(z.real, z.imag)
    assert np.array_equal(np.isinf(got), np.isinf(want)), "hypot(+-Inf, NaN) = Inf, no overflow at 1e300"
    assert _ulps(got, want) <= 1
    assert got[(z.real == 1e-310) & (z.imag == 0)][0] == 1e-310   # no flush of denormals
    assert got[(z.real == 1e300) & (z.imag == 1e300)][0] == pytest.approx(1.4142135623730951e300, rel=1e-15)


def test_abs2_f64_bitexact(ctx):
    z = _cplx(777_777, 3.0)
    assert _same(ctx.abs2(z, dtype=F64), R.abs2(z))


def test_invert_am_f64_bitexact_vs_own_am(ctx):
    z = _cplx(300_001)
    a = ctx.amDemod(z, dtype=F64)
    assert _same(ctx.invert_amDemod(z, dtype=F64), 1.0 - a / a.max())
    z[1234] = complex(np.nan, 0.0)
    assert np.isnan(ctx.invert_amDemod(z, dtype=F64)).all()      # NaN propagates as through Julia's maximum
    with pytest.raises(AssertionError):
        ctx.invert_amDemod(np.zeros(0, np.complex128), dtype=F64)  # maximum of an empty collection


def test_fm_demod_f64_within_2ulp(ctx):
    z = _cplx(500_000)
    got = ctx.fmDemod(z, dtype=F64)
    re, im = R.fm_product(z)
    assert got[0] == 0.0
    assert _ulps(got[1:], np.arctan2(im, re)) <= 2


# ---- resize / raster -------------------------------------------------------------------------------------------------
def test_naive_resample_f64_bitexact(ctx):
    x = rng.standard_normal(1001)
    out = np.empty(x.size * 3, F64)
    ctx.naiveResampler(out, x, 3, dtype=F64)
    assert _same(out, R.naive_resample(x, 3))


@pytest.mark.parametrize("n_in,n_out", [(333, 41), (125, 500), (1000, 1000), (2, 7), (1_000_003, 777_777)])
def test_resize1d_f64(ctx, n_in, n_out):
    x = rng.random(n_in, dtype=np.float32)
    got = ctx.imresize1d(x.astype(F64), n_out, dtype=F64)
    assert _same(got, R.resize1d(x.astype(F64), n_out))
    assert np.array_equal(got.astype(np.float32).view(np.uint32), O.imresize1d(x, n_out).view(np.uint32))


S2I_CASES = list(RASTER_CASES) + [(333_333, 1125, 2576), (833_333, 2250, 4400), (1125 * 2576, 1125, 2576)]


@pytest.mark.parametrize("S,y_t,x_t", S2I_CASES)
def test_sig_to_image_f64(ctx, S, y_t, x_t):
    x = rng.random(S, dtype=np.float32)
    got = ctx.sig_to_image(x.astype(F64), y_t, x_t, dtype=F64)
    assert got.flags.f_contiguous and got.shape == (y_t, x_t)
    assert _same(got, R.sig_to_image(x.astype(F64), y_t, x_t))
    o = O.sig_to_image(x, y_t, x_t)
    assert np.array_equal(np.asfortranarray(got.astype(np.float32)).ravel(order="F").view(np.uint32), o.ravel(order="F").view(np.uint32))


@pytest.mark.parametrize("h,w,ho,wo", [(45, 64, 20, 30), (45, 64, 600, 800), (1125, 2576, 600, 800), (2250, 4400, 600, 800),
                                       (600, 800, 600, 800), (20, 30, 77, 131)])
def test_resize2d_and_downgrade_f64(ctx, h, w, ho, wo):
    img = np.asfortranarray(rng.random((h, w), dtype=np.float32))
    a = img.astype(F64, order="F")
    got = ctx.imresize2d(a, (ho, wo), dtype=F64)
    assert _same(got, R.resize2d(a, ho, wo))
    assert np.array_equal(got.astype(np.float32).ravel(order="F").view(np.uint32),
                          O.imresize2d(img, (ho, wo)).ravel(order="F").view(np.uint32))
    if (ho, wo) == (600, 800):
        assert _same(ctx.downgradeImage(a, dtype=F64), got)


def test_f64_entry_points_refuse_other_element_types(ctx):
    with pytest.raises(AssertionError):
        ctx.amDemod(np.zeros(8, np.complex64), dtype=F64)
    with pytest.raises(AssertionError):
        ctx.sig_to_image(np.zeros(1200, np.float32), 30, 40, dtype=F64)
    with pytest.raises(AssertionError):
        ctx.calculate_autocorrelation(np.zeros(100, np.float32), 1000.0, 0, 0.01, dtype=F64)
    with pytest.raises(AssertionError):
        ctx.amDemod(np.zeros(8, np.complex128), dtype=np.int32)


# ---- sync --------------------------------------------------------------------------------------------------------------
def _sync_images(y_t, x_t, k):
    out = []
    for f in range(k):
        img = rng.random((y_t, x_t)) + 1.0
        c0, r0 = (17 + 29 * f) % x_t, (5 + 11 * f) % y_t
        img[:, c0: c0 + max(3, x_t // 12)] *= 0.1
        img[r0: r0 + max(2, y_t // 20), :] *= 0.1
        out.append(np.asfortranarray(img))
    return out


@pytest.mark.parametrize("y_t,x_t", [(600, 800), (77, 131), (1125, 2576)])
def test_vsync_f64_bitexact(ctx, tsdr, y_t, x_t):
    s = tsdr.api.SyncXY(ctx, y_t, x_t, dtype=F64)
    r = R.SyncXY64(y_t, x_t)
    assert (s.wmin_y, s.wmax_y, s.wmin_x, s.wmax_x) == R.bounds(y_t, x_t)
    imgs = _sync_images(y_t, x_t, 3)
    for rnd in range(2):
        for f, img in enumerate(imgs):
            got, want = s.vsync(img), r.vsync(img)
            assert got == want, (rnd, f, got, want)
            bx, by = s.beta("x"), s.beta("y")
            assert bx.dtype == F64 and _same(bx, r.beta_x) and _same(by, r.beta_y)
            if f == 0:
                assert got[0] == 1                   # stale s_y of a fresh / reset state
            fl = np.sort(r.beta_x.ravel())[::-1]
            print(f"{y_t}x{x_t} frame {f}: beta_x top-2 margin {(fl[0] - fl[1]) / fl[0]:.3e}")
        s.reset()
        r.reset()
    s.close()


def test_fill_beta_f64_bitexact(ctx):
    for n, w_min, w_max in [(800, 40, 200), (131, 7, 32), (2576, 129, 644)]:
        cv = rng.random(n) * 100.0
        assert _same(ctx.fill_beta(cv, n, w_min, w_max, dtype=F64), R.fill_beta(cv, n, w_min, w_max))


def test_sync_types_refuse_each_other(ctx, tsdr):
    api = tsdr.api
    s64 = api.SyncXY(ctx, 600, 800, dtype=F64)
    a32, b32 = api.SyncXY(ctx, 600, 800), api.SyncXY(ctx, 600, 800)
    img1, img2 = _sync_images(600, 800, 2)
    first = a32.vsync(img1)
    b32.vsync(img1)
    sy, sx = C.c_int(0), C.c_int(0)
    f32img = np.asfortranarray(img1, np.float32)
    assert ctx.lib.tsdr_vsync(C.c_void_p(s64.h), f32img.ctypes.data_as(C.c_void_p), C.byref(sy), C.byref(sx)) == -1
    assert ctx.lib.tsdr_vsync_f64(C.c_void_p(a32.h), img1.ctypes.data_as(C.c_void_p), C.byref(sy), C.byref(sx)) == -1
    assert ctx.lib.tsdr_sync_beta(C.c_void_p(s64.h), 0, np.empty(1, np.float32).ctypes.data_as(C.c_void_p)) == -1
    assert ctx.lib.tsdr_sync_beta_f64(C.c_void_p(a32.h), 0, np.empty(1, F64).ctypes.data_as(C.c_void_p)) == -1
    d_iq, d_state = ctx.dev_alloc(8 * 4096), ctx.dev_alloc(4 * 600 * 800)
    try:
        n = C.c_int(0)
        for do_align in (1, 0):
            rc = ctx.lib.tsdr_frames_d(ctx.h, C.c_void_p(s64.h), C.c_void_p(d_iq), 4096, 1024, 32, 32, C.c_float(0.5), do_align,
                                       C.c_void_p(d_state), None, None, None, C.byref(n))
            assert rc == -1
        state = np.zeros((600, 800), np.float32, order="F")
        with pytest.raises(AssertionError):
            ctx.frames(s64, np.zeros(4096, np.complex64), 1024, 32, 32, 0.5, state)
    finally:
        ctx.dev_free(d_iq)
        ctx.dev_free(d_state)
    # the f32 state the refused calls sat between carries on exactly like an untouched twin
    assert first[0] == 1 and a32.vsync(img2) == b32.vsync(img2)
    s64.reset()
    assert s64.vsync(img2)[0] == 1
    for s in (s64, a32, b32):
        s.close()


# ---- autocorrelation / spectrum --------------------------------------------------------------------------------------
def _leak_power(synth, Fs, n):
    z = synth.synth_leak(Fs, 2576, 1125, 60.0, n).astype(np.complex128)
    return np.abs(z)


@pytest.mark.parametrize("Fs,maxDelay,length", [(20e6, 0.1, 5_000_000), (20e6, 0.1, 3_000_000), (1e6, 0.06, 100_003)])
def test_autocorr_f64(ctx, synth, Fs, maxDelay, length):
    x = _leak_power(synth, Fs, length)
    n = min(2 * int(round(maxDelay * Fs)), length)
    lin, _ = ctx.calculate_autocorrelation(x, Fs, 0, maxDelay, scale="lin", dtype=F64)
    want = R.autocorr(x, Fs, 0, maxDelay, log_scale=False)
    assert lin.dtype == F64 and lin.size == want.size
    err = np.max(np.abs(lin - want)) / np.max(want)
    print(f"autocorr_f64 n={n}: max |d abs2| / max(abs2) = {err:.2e}")
    assert err < 1e-11
    G, _ = ctx.calculate_autocorrelation(x, Fs, 0, maxDelay, dtype=F64)
    rates, Gz = ctx.zoom_autocorr(G, Fs, rate_min=50, rate_max=90)
    _, Wz = ctx.zoom_autocorr(10.0 * np.log10(want), Fs, rate_min=50, rate_max=90)
    top = np.sort(Wz)[::-1]
    print(f"zoom window findmax {int(np.argmax(Gz))}, top-2 margin {top[0] - top[1]:.3e} dB")
    assert int(np.argmax(Gz)) == int(np.argmax(Wz))


def test_autocorr_f64_bounds(ctx):
    with pytest.raises(IndexError):   # len < indexMax: the reference's BoundsError
        ctx.calculate_autocorrelation(rng.random(1000), 1e6, 0, 0.01, dtype=F64)


@pytest.mark.parametrize("cplx,N,length", [(False, 80_000, 100_000), (True, 80_000, 80_000), (True, 65_536, 65_536),
                                           (False, 80_021, 80_021), (True, 1000, 4000)])
def test_spectrum_f64(ctx, cplx, N, length):
    sig = _cplx(length) if cplx else rng.standard_normal(length)
    _, lin = ctx.getSpectrum(1.0, sig, N, lin=True, dtype=F64)
    want = R.spectrum(sig, N, log_scale=False)
    assert lin.dtype == F64 and np.max(np.abs(lin - want)) / np.max(want) < 1e-11
    _, db = ctx.getSpectrum(1.0, sig, N, dtype=F64)
    # the same power through the device's log10 (within a few ulp of numpy's)
    assert np.max(np.abs(db - 10.0 * np.log10(lin))) <= 1e-14 * np.max(np.abs(db))


# ---- no change for f32 callers ---------------------------------------------------------------------------------------
def test_default_dtype_keeps_the_f32_path(ctx):
    z = _cplx(4097).astype(np.complex128)
    got = ctx.amDemod(z)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), O.amDemod(z.astype(np.complex64)).view(np.uint32))
    x = rng.random(3333)
    assert ctx.sig_to_image(x, 70, 130).dtype == np.float32
    assert ctx.getSpectrum(1.0, z, 1000)[1].dtype == np.float32


def test_f32_frames_unchanged_by_f64_calls(ctx, tsdr, synth):
    api = tsdr.api
    S, y_t, x_t = 20_000, 125, 160
    iq = synth.synth_leak(2e6, x_t, y_t, 100.0, 4 * S)

    def run():
        ctx.set_option("sync_guard_ppb", 20000)
        ctx.set_option("sync_guard_auto", 1)
        s = api.SyncXY(ctx, 600, 800)
        state = np.zeros((600, 800), np.float32, order="F")
        r = ctx.frames(s, iq, S, y_t, x_t, 0.5, state, want_raster=True)
        s.close()
        return r, state

    r0, st0 = run()
    z = _cplx(1_000_000)
    ctx.amDemod(z, dtype=F64)
    ctx.invert_amDemod(z, dtype=F64)
    ctx.sig_to_image(rng.random(333_333), 1125, 2576, dtype=F64)
    ctx.calculate_autocorrelation(rng.random(200_000), 1e6, 0, 0.1, dtype=F64)
    ctx.getSpectrum(1.0, z, 80_021, dtype=F64)
    s64 = api.SyncXY(ctx, 600, 800, dtype=F64)
    s64.vsync(_sync_images(600, 800, 1)[0])
    s64.close()
    r1, st1 = run()
    assert np.array_equal(r0["sync_idx"], r1["sync_idx"])
    assert np.array_equal(st0.view(np.uint32), st1.view(np.uint32))
    for a, b in zip(r0["frames"] + r0["raster"], r1["frames"] + r1["raster"]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- end to end: a :double capture through the offline flow in Float64 ----------------------------------------------
def test_replay_double_capture_in_f64(ctx, tsdr, tmp_path):
    replay = importlib.import_module("tempestsdr_jl_amd.replay")
    dat = importlib.import_module("tempestsdr_jl_amd.dat_files")
    from test_replay import OracleBackend
    Fs, x_t, y_t, fv, n = 2.0e6, 1056, 628, 60.0, 600_000
    iq = synth_mod(tsdr).synth_leak(Fs, x_t, y_t, fv, n)
    path = str(tmp_path / "dumpIQ_0_double.dat")
    dat.writeComplexBinary(iq.astype(np.complex128), path, "double")
    g = replay.replay_file(ctx, path, Fs, fmt="double", dtype=np.complex128, offset=42_000)
    o = replay.replay_file(OracleBackend, path, Fs, fmt="double", offset=42_000)
    for k in ("fv", "y_t", "name", "sync", "tau", "sample_offset"):
        assert g[k] == o[k], (k, g[k], o[k])
    assert g["mode"].width == o["mode"].width and g["mode"].height == o["mode"].height
    assert g["image"].dtype == F64 and g["aligned"].dtype == F64 and g["G"].dtype == F64
    sig = ctx.amDemod(dat.readComplexBinary(path, "double"), dtype=F64)
    d = int(np.round(Fs / g["mode"].refresh))
    a0 = 42_000 + g["sample_offset"]
    assert _same(g["aligned"], R.sig_to_image(sig[a0: a0 + d], g["mode"].height, g["mode"].width))


def synth_mod(tsdr):
    return importlib.import_module("tempestsdr_jl_amd.synth")


def test_no_waits_given_up(ctx):
    assert ctx.wait_stats() == (0, 0)
