"""The device-pointer (`_d`) entry points at offsets inside larger buffers.

The host forms stage every array at the start of a workspace allocation; the `_d` forms exist for callers that pass
`base + k * sizeof(element)` -- a tensor slice, one frame of a capture.  Every case here calls a `_d` symbol with each array
inside a guarded arena (dptr_util.py) at a chosen pointer phase, input and output phases varied independently, and

  * compares with the reference and the bar the host form's own test uses (restated or imported below, with their origin);
    no tolerance is introduced here;
  * asserts after the call that nothing outside the documented output was written and that no input was;
  * where a phase exists to reach a fallback route, proves from the per-kernel profile that it did.

Pointers are always aligned to one element of what they point to.  The one exception are the refusal tests at the end, which
pass an under-aligned pointer to a library that checks on the host first: they assert TSDR_EINVAL, the error text, and that no
kernel was launched.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import f64_ref as R
import f64_spec_ref as S64
import oracle_lib as O
from dptr_util import Arenas
from test_fast_mode_gpu import RTOL, RTOL_TAPS                      # 6e-7: the FAST frame loop against the oracle
from test_fft_path_gpu import CORR_TOL, FFT_TOL, relmax             # 2e-5 / 5e-6, relative to the largest magnitude
from test_frame_path_gpu import assert_bitexact

pytestmark = pytest.mark.gpu

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
PH_F32 = (0, 4, 8, 12)     # float pointers: every phase mod 16
PH_C64 = (0, 8)            # ComplexF32: 0, 8 mod 16
PH_F64 = (0, 8)            # double
PH_C128 = (0, 16)          # ComplexF64: 0 and 16 mod 32
EINVAL = -1


def _rng(*key):
    return np.random.default_rng([20260, *[int(k) for k in key]])


def _crandn(rng, n, dtype=C64, scale=1.0):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(dtype)


def _pairs(a, b, full=True):
    """(input phase, output phase) combinations: the full product, or -- for large cases -- a walk that still visits every
    phase of both sides and never pairs equal indices only"""
    if full:
        return list(itertools.product(a, b))
    n = max(len(a), len(b))
    return [(a[i % len(a)], b[(i + 1) % len(b)]) for i in range(n)] + [(a[0], b[0])]


class profiled:
    """bracket calls with per-kernel profiling; .names() -> {kernel name: launches} of what ran inside"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.profile(True)
        self.ctx.profile_reset()
        return self

    def names(self):
        return {k: v["launches"] for k, v in self.ctx.profile_results().items()}

    def __exit__(self, *exc):
        self.ctx.profile(False)
        return False


def _same_bits(got, want, what):
    """bit equality of f64 arrays, NaN == NaN (payloads may differ)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F64, (what, got.shape, want.shape, got.dtype)
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}"


def _ulps(a, b):
    """test_f64_gpu.py:_ulps"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ia, ib = a.view(np.int64), b.view(np.int64)
    d = np.where((ia < 0) == (ib < 0), np.abs(ia - ib), np.int64(1) << 62)
    d = np.where((a == b) | np.isnan(a), 0, d)
    return int(np.max(d)) if d.size else 0


# ======================================================================================================== demodulation
# the `vals` table of test_frame_path_gpu.py:test_am_demod_extremes, and SPECIALS of test_f64_gpu.py
VALS32 = np.array([0.0, -0.0, 1e-45, 1e-38, 1e-20, 1.0, 3e38, -3e38, np.inf, -np.inf, np.nan, 1e19, 6e-8], F32)
VALS64 = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 1.0, -3.5, 1e300, -1e300, 1.7e308,
                   np.inf, -np.inf, np.nan])
# fmDemod's bar (1e-6 absolute on the angle, test_fm_demod_close) is a bar on atan2 of finite products: its table is the
# part of `vals` whose pairwise products stay finite and normal
VALS32_FM = np.array([0.0, -0.0, 1e-20, 1.0, 1e19, 6e-8], F32)
DEMOD_N = [1, 3, 4, 5, 1023, 100_003]


def _extremes_in_noise(n, vals, dtype, key):
    """random IQ with the vals x vals table (as many of its entries as fit, in shuffled order) spread through it"""
    rng = _rng(n, key)
    z = _crandn(rng, n, dtype, 5e-3)
    re, im = np.meshgrid(vals, vals)
    table = np.empty(re.size, dtype)
    table.real, table.imag = re.ravel(), im.ravel()
    table = table[rng.permutation(table.size)]
    k = min(n, table.size)
    z[np.linspace(0, n - 1, k).astype(np.int64)] = table[:k]
    return z


DEMOD32 = {
    "am": (lambda ctx, i, n, o: ctx.call("tsdr_am_demod_d", i, n, o), O.amDemod, ("am_demod", "am_demod1")),
    "abs2": (lambda ctx, i, n, o: ctx.call("tsdr_abs2_d", i, n, o), O.abs2, ("abs2", "abs2_1")),
    "invert": (lambda ctx, i, n, o: ctx.call("tsdr_invert_am_d", i, n, o), O.invert_amDemod, ("invert_am_abs", "invert_am_abs1")),
}


@pytest.mark.parametrize("n", DEMOD_N)
@pytest.mark.parametrize("fn", sorted(DEMOD32))
def test_demod_f32_bitexact_at_every_phase(ctx, fn, n):
    """amDemod / abs2 / invert_amDemod: bit-exact against the oracle (test_am_demod_bitexact, test_am_demod_extremes,
    test_abs2_bitexact, test_invert_am_bitexact) at IQ phases 0 / 8 and output phases 0 / 4 / 8 / 12 mod 16.  Both
    pointers 16-byte aligned: the kernel that moves 16-byte vectors; anything else: the one-sample-per-lane kernel."""
    run, ref, (k_vec, k_one) = DEMOD32[fn]
    inputs = [_extremes_in_noise(n, VALS32, C64, 1)]
    if fn == "invert":   # with NaN / Inf in the data the maximum makes every output NaN: also a finite table, whose values count
        inputs.append(_extremes_in_noise(n, VALS32[np.isfinite(VALS32) & (np.abs(VALS32) < 1e38)], C64, 2))
    for z in inputs:
        want = ref(z)
        for pi, po in _pairs(PH_C64, PH_F32):
            with Arenas(ctx) as A, profiled(ctx) as prof:
                i, o = A.input("iq", z, pi), A.output("out", 4 * n, po)
                run(ctx, i.ptr, n, o.ptr)
                A.check()
                assert_bitexact(o.get(F32), want, f"{fn} n={n} iq@{pi} out@{po}")
                names = prof.names()
                assert (k_vec in names) == (pi == 0 and po == 0) and (k_one in names) == (not (pi == 0 and po == 0)), (pi, po, names)


@pytest.mark.parametrize("n", DEMOD_N)
def test_fm_demod_f32_at_every_phase(ctx, n):
    """fmDemod has no vector requirement: 1e-6 on the angle (test_fm_demod_close) at both IQ phases and all four output phases"""
    z = _extremes_in_noise(n, VALS32_FM, C64, 3)
    want = O.fmDemod(z)
    for pi, po in _pairs(PH_C64, PH_F32):
        with Arenas(ctx) as A:
            i, o = A.input("iq", z, pi), A.output("out", 4 * n, po)
            ctx.call("tsdr_fm_demod_d", i.ptr, n, o.ptr)
            A.check()
            got = o.get(F32)
            assert got[0] == 0.0
            assert np.max(np.abs(got - want)) <= 1e-6, (n, pi, po, np.max(np.abs(got - want)))


@pytest.mark.parametrize("n", DEMOD_N)
def test_demod_f64_at_every_phase(ctx, n):
    """the `_f64_d` forms, bars of test_f64_gpu.py: am within 1 ulp of hypot (Inf where hypot is Inf), abs2 bit-exact
    against re*re + im*im, invert bit-exact against 1 - a / max(a) of the device's own a (a NaN among the samples: NaN
    everywhere, as through Julia's maximum), fm within 2 ulp of atan2 (on random data, as there)"""
    z = _extremes_in_noise(n, VALS64, C128, 4)
    zf = _crandn(_rng(n, 5), n, C128)
    re, im = R.fm_product(zf)
    for pi, po in _pairs(PH_C128, PH_F64):
        with Arenas(ctx) as A, np.errstate(all="ignore"):
            i, i2 = A.input("iq", z, pi), A.input("iq (random)", zf, pi)
            a, p, v, a2, f, v2 = (A.output(nm, 8 * n, q) for nm, q in (("am", po), ("abs2", 8 - po), ("invert", po), ("am (random)", po),
                                                                      ("fm", 8 - po), ("invert (random)", po)))
            ctx.call("tsdr_am_demod_f64_d", i.ptr, n, a.ptr)
            ctx.call("tsdr_abs2_f64_d", i.ptr, n, p.ptr)
            ctx.call("tsdr_invert_am_f64_d", i.ptr, n, v.ptr)
            ctx.call("tsdr_am_demod_f64_d", i2.ptr, n, a2.ptr)
            ctx.call("tsdr_fm_demod_f64_d", i2.ptr, n, f.ptr)
            ctx.call("tsdr_invert_am_f64_d", i2.ptr, n, v2.ptr)
            A.check()
            what = f"n={n} iq@{pi} out@{po}"
            got, want = a.get(F64), np.hypot(z.real, z.imag)
            assert np.array_equal(np.isinf(got), np.isinf(want)) and _ulps(got, want) <= 1, what
            _same_bits(p.get(F64), R.abs2(z), "abs2_f64 " + what)
            _same_bits(v.get(F64), 1.0 - got / got.max(), "invert_am_f64 (extremes) " + what)
            am = a2.get(F64)
            assert _ulps(am, np.hypot(zf.real, zf.imag)) <= 1, what
            _same_bits(v2.get(F64), 1.0 - am / am.max(), "invert_am_f64 " + what)
            gf = f.get(F64)
            assert gf[0] == 0.0 and (n == 1 or _ulps(gf[1:], np.arctan2(im, re)) <= 2), what


# ========================================================================================================== resampling
# shapes of test_imresize1d_bitexact: up, down, copy, strong up
@pytest.mark.parametrize("n_in,n_out", [(100, 873), (1000, 37), (64, 64), (333, 2898), (7, 7000)])
def test_resize1d_at_every_phase(ctx, n_in, n_out):
    x = _rng(n_in, n_out).random(n_in, dtype=F32)
    want, want64 = O.imresize1d(x, n_out), R.resize1d(x.astype(F64), n_out)
    for pi, po in _pairs(PH_F32, PH_F32):
        with Arenas(ctx) as A:
            i, o = A.input("sig", x, pi), A.output("out", 4 * n_out, po)
            ctx.call("tsdr_resize1d_d", i.ptr, n_in, n_out, o.ptr)
            A.check()
            assert_bitexact(o.get(F32), want, f"resize1d {n_in}->{n_out} sig@{pi} out@{po}")
    for pi, po in _pairs(PH_F64, PH_F64):
        with Arenas(ctx) as A:
            i, o = A.input("sig", x.astype(F64), pi), A.output("out", 8 * n_out, po)
            ctx.call("tsdr_resize1d_f64_d", i.ptr, n_in, n_out, o.ptr)
            A.check()
            _same_bits(o.get(F64), want64, f"resize1d_f64 {n_in}->{n_out} sig@{pi} out@{po}")


# shapes of RASTER_CASES (test_sig_to_image_bitexact): copy path, strong up-sampling, ragged tiles, down-sampling with an odd
# y_t * x_t (125 * 161), heavy down-sampling (the direct kernel), one C2 frame
@pytest.mark.parametrize("S,y_t,x_t", [(1200, 30, 40), (137, 30, 40), (3333, 70, 130), (26001, 125, 161), (800000, 100, 128),
                                       (333333, 1125, 2576)])
def test_sig_to_image_at_every_phase(ctx, S, y_t, x_t):
    P = y_t * x_t
    sig = _rng(S, P).random(S, dtype=F32)
    want = O.sig_to_image(sig, y_t, x_t)
    big = max(S, P) > 100_000
    for pi, po in _pairs(PH_F32, PH_F32, full=not big):
        with Arenas(ctx) as A:
            i, o = A.input("sig", sig, pi), A.output("img", 4 * P, po)
            ctx.call("tsdr_sig_to_image_d", i.ptr, S, y_t, x_t, o.ptr)
            A.check()
            assert_bitexact(o.get(F32, (y_t, x_t), "F"), want, f"sig_to_image S={S} {y_t}x{x_t} sig@{pi} img@{po}")
    if big:
        return
    want64 = R.sig_to_image(sig.astype(F64), y_t, x_t)
    for pi, po in _pairs(PH_F64, PH_F64):
        with Arenas(ctx) as A:
            i, o = A.input("sig", sig.astype(F64), pi), A.output("img", 8 * P, po)
            ctx.call("tsdr_sig_to_image_f64_d", i.ptr, S, y_t, x_t, o.ptr)
            A.check()
            _same_bits(o.get(F64, (y_t, x_t), "F"), want64, f"sig_to_image_f64 S={S} sig@{pi} img@{po}")


# shapes of test_imresize2d_bitexact: down, up, one axis unchanged, C2 -> 600x800
@pytest.mark.parametrize("shape,size", [((45, 64), (20, 30)), ((30, 40), (600, 800)), ((700, 800), (600, 800)), ((1125, 2576), (600, 800))])
def test_resize2d_and_downgrade_at_every_phase(ctx, shape, size):
    img = np.asfortranarray(_rng(*shape).random(shape, dtype=F32))
    want = O.imresize2d(img, size)
    flat = img.ravel(order="F")
    npx = size[0] * size[1]
    big = img.size > 100_000
    for pi, po in _pairs(PH_F32, PH_F32, full=not big):
        with Arenas(ctx) as A:
            i, o, o2 = A.input("img", flat, pi), A.output("out", 4 * npx, po), A.output("downgrade out", 4 * 480000, po)
            ctx.call("tsdr_resize2d_d", i.ptr, shape[0], shape[1], size[0], size[1], o.ptr)
            if size == (600, 800):
                ctx.call("tsdr_downgrade_d", i.ptr, shape[0], shape[1], o2.ptr)
            A.check()
            assert_bitexact(o.get(F32, size, "F"), want, f"resize2d {shape}->{size} img@{pi} out@{po}")
            if size == (600, 800):
                assert_bitexact(o2.get(F32, size, "F"), want, f"downgrade {shape} img@{pi} out@{po}")
    a64 = img.astype(F64, order="F")
    want64 = R.resize2d(a64, *size)
    for pi, po in _pairs(PH_F64, PH_F64, full=not big):
        with Arenas(ctx) as A:
            i, o, o2 = A.input("img", a64.ravel(order="F"), pi), A.output("out", 8 * npx, po), A.output("downgrade out", 8 * 480000, po)
            ctx.call("tsdr_resize2d_f64_d", i.ptr, shape[0], shape[1], size[0], size[1], o.ptr)
            if size == (600, 800):
                ctx.call("tsdr_downgrade_f64_d", i.ptr, shape[0], shape[1], o2.ptr)
            A.check()
            _same_bits(o.get(F64, size, "F"), want64, f"resize2d_f64 {shape}->{size} img@{pi} out@{po}")
            if size == (600, 800):
                _same_bits(o2.get(F64, size, "F"), want64, f"downgrade_f64 {shape} img@{pi} out@{po}")


@pytest.mark.parametrize("n,up", [(1000, 3), (1001, 3), (5, 1), (333, 7)])
def test_naive_resample_at_every_phase(ctx, n, up):
    x = _rng(n, up).random(n, dtype=F32)
    for pi, po in _pairs(PH_F32, PH_F32):
        with Arenas(ctx) as A:
            i, o = A.input("in", x, pi), A.output("out", 4 * n * up, po)
            ctx.call("tsdr_naive_resample_d", i.ptr, n, up, o.ptr)
            A.check()
            assert_bitexact(o.get(F32), O.naiveResampler(x, up), f"naiveResampler n={n} in@{pi} out@{po}")
    for pi, po in _pairs(PH_F64, PH_F64):
        with Arenas(ctx) as A:
            i, o = A.input("in", x.astype(F64), pi), A.output("out", 8 * n * up, po)
            ctx.call("tsdr_naive_resample_f64_d", i.ptr, n, up, o.ptr)
            A.check()
            _same_bits(o.get(F64), R.naive_resample(x.astype(F64), up), f"naive_resample_f64 n={n} in@{pi} out@{po}")


# ======================================================================================================= resampler!(out, in)
@pytest.mark.parametrize("bufferSize,up", [(1000, 4), (1024, 2), (64, 2), (10, 1), (512, 8), (3000, 2)])
def test_resampler_run_at_every_phase(ctx, tsdr, bufferSize, up):
    """resampler! through tsdr_resampler_run_d against O.Resampler at test_init_resampler's bar (4e-6 of the largest output).
    An even bufferSize takes the half-size route ("resampler_mid") only while `in` and `out` are both 8-byte aligned; a real
    pointer at an odd float takes the full-size transforms instead -- the route the host form only reaches with an odd
    bufferSize.  sizeFFT == 4096 is one workgroup whatever the pointers."""
    N = bufferSize * up
    r, o = ctx.init_resampler(F32, bufferSize, up), O.Resampler(bufferSize, up)
    x = _rng(bufferSize, up).standard_normal(bufferSize).astype(F32)
    want = np.empty(N, F32)
    o(want, x)
    for pi, po in _pairs((0, 4), (0, 4)):
        with Arenas(ctx) as A, profiled(ctx) as prof:
            i, out = A.input("in", x, pi), A.output("out", 4 * N, po)
            tsdr.api.check(ctx.h, ctx.lib.tsdr_resampler_run_d(C.c_void_p(r.h), i.ptr, bufferSize, out.ptr), "tsdr_resampler_run_d")
            A.check()
            e = relmax(out.get(F32), want)
            assert e < 4e-6, (bufferSize, up, pi, po, e)
            names = prof.names()
            if N == 4096:
                assert "resampler_4096" in names and "resampler_mid" not in names, names
            else:
                assert ("resampler_mid" in names) == (pi == 0 and po == 0), (pi, po, names)
    r.close()
    # Float64 closure: bar of test_resampler_f64
    r64 = ctx.init_resampler(F64, bufferSize, up)
    H = r64.lpf64()
    x64 = x.astype(F64)
    want64 = S64.resampler(x64, up, H)
    for pi, po in _pairs(PH_F64, PH_F64):
        with Arenas(ctx) as A:
            i, out = A.input("in", x64, pi), A.output("out", 8 * N, po)
            tsdr.api.check(ctx.h, ctx.lib.tsdr_resampler_run_f64_d(C.c_void_p(r64.h), i.ptr, bufferSize, out.ptr), "tsdr_resampler_run_f64_d")
            A.check()
            assert np.max(np.abs(out.get(F64) - want64)) <= 1e-12 * max(1.0, np.log2(N)) * np.max(np.abs(want64)), (bufferSize, up, pi, po)
    r64.close()


# ====================================================================================================== autocorrelation
def _search_signal(n, amp=3e-3, key=0):
    """the signal of test_autocorr_fused_middle_and_fused_findmax: noise with a period for the zoom window to find.  Its first
    and last sample carry 100 times the power of the rest: a loader that drops or misplaces either end of the buffer then moves
    every lag by far more than the bar, at any length (without them one sample in a million is below 2e-4 dB)"""
    z = _crandn(_rng(n, key), n, C64, amp)
    z *= (1.0 + 0.5 * np.cos(2 * np.pi * np.arange(n) / 977.0)).astype(F32)
    z[0] *= 10
    z[-1] *= 10
    return z


# one length per route of test_autocorr_fused_middle_and_fused_findmax: n = 2 * 2^a 3^b 5^c whose half takes two passes
# (100 000 = 50 * 2000) and three (196 608 = 64 * 48 * 64), a power of two, an odd length (zero-padded transform + fold)
AC_LENGTHS = [(200_000, 1e6), (393_216, 1e6), (8192, 4096.0), (100_003, 1e6)]


def test_autocorr_lengths_cover_the_routes(ctx):
    f = (C.c_uint * 8)()
    assert ctx.lib.tsdr_fft_plan(100_000, f, 8) == 2 and ctx.lib.tsdr_fft_plan(196_608, f, 8) == 3


@pytest.mark.parametrize("n,Fs", AC_LENGTHS)
def test_autocorr_real_at_every_phase(ctx, n, Fs):
    """tsdr_autocorr_d, real x at all four float phases, out at all four: 2e-4 dB against the oracle (the fused test's bar)"""
    x = O.abs2(_search_signal(n))
    maxd = (n // 2) / Fs
    want, _ = O.calculate_autocorrelation(x, Fs, 0, maxd)
    for pi, po in _pairs(PH_F32, PH_F32):
        with Arenas(ctx) as A:
            i, o = A.input("x", x, pi), A.output("lags", 4 * want.size, po)
            n_out = C.c_size_t(0)
            ctx.call("tsdr_autocorr_d", i.ptr, n, Fs, 0.0, maxd, 1, o.ptr, C.byref(n_out))
            A.check()
            assert n_out.value == want.size
            d = np.max(np.abs(o.get(F32) - want))
            assert d < 2e-4, (n, pi, po, d)


# shapes of test_autocorr_vs_oracle: a lag window that does not start at 0, and n/2 with a factor 7 (padded route)
@pytest.mark.parametrize("n,Fs,maxd,mind", [(3000, 30_000.0, 0.05, 0.0), (5000, 10_000.0, 0.1, 0.01), (14_000, 1000.0, 7.0, 0.5)])
def test_autocorr_real_lin_and_log_at_every_phase(ctx, n, Fs, maxd, mind):
    x = (_rng(n).random(n) ** 2).astype(F32) * 1e-5
    for log_scale, scale in ((0, "lin"), (1, "log")):
        want, _ = O.calculate_autocorrelation(x, Fs, mind, maxd, scale)
        for pi, po in _pairs(PH_F32, PH_F32):
            with Arenas(ctx) as A:
                i, o = A.input("x", x, pi), A.output("lags", 4 * want.size, po)
                n_out = C.c_size_t(0)
                ctx.call("tsdr_autocorr_d", i.ptr, n, Fs, mind, maxd, log_scale, o.ptr, C.byref(n_out))
                A.check()
                assert n_out.value == want.size
                g = o.get(F32)
                if log_scale:
                    assert np.max(np.abs(g - want)) < 2e-4, (n, pi, po, np.max(np.abs(g - want)))
                else:
                    assert relmax(g, want) < 2 * CORR_TOL, (n, pi, po, relmax(g, want))


@pytest.mark.parametrize("n,Fs", AC_LENGTHS)
def test_autocorr_iq_at_both_phases_takes_its_route(ctx, n, Fs):
    """tsdr_autocorr_iq_d: abs2 formed on the fly.  16-byte aligned IQ and n = 2 * smooth: the native transform whose first
    pass loads float4 pairs.  IQ at an ODD SAMPLE (8 mod 16): "ac_pack", the zero-padded power-of-two transform and "ac_fold" --
    the same 2e-4 dB, as "ac_mixed" = 0 holds that route to for real input."""
    z = _search_signal(n, key=1)
    maxd = (n // 2) / Fs
    want, _ = O.calculate_autocorrelation(O.abs2(z), Fs, 0, maxd)
    for pi, po in _pairs(PH_C64, PH_F32):
        with Arenas(ctx) as A, profiled(ctx) as prof:
            i, o = A.input("iq", z, pi), A.output("lags", 4 * want.size, po)
            n_out = C.c_size_t(0)
            ctx.call("tsdr_autocorr_iq_d", i.ptr, n, Fs, 0.0, maxd, 1, o.ptr, C.byref(n_out))
            A.check()
            d = np.max(np.abs(o.get(F32) - want))
            assert n_out.value == want.size and d < 2e-4, (n, pi, po, d)
            names = prof.names()
            if pi == 8:
                assert "ac_pack" in names and "ac_fold" in names, (n, pi, names)
            elif n % 2 == 0:
                assert "ac_pack" not in names and "ac_fold" not in names, (n, pi, names)
            else:   # odd n, aligned: padded transform straight from the samples
                assert "ac_pack" not in names and "ac_fold" in names, (n, pi, names)


def _search(ctx, A, z, Fs, pi, po, name=""):
    """tsdr_autocorr_search_d(is_iq = 1) on z at phase pi, lags at phase po -> (lags arena, idx, val, lo, hi)"""
    n = z.size
    maxd = (n // 2) / Fs
    cnt = n // 2
    lo, hi = 300, min(3000, cnt)      # zoom_autocorr bounds for rate_min = Fs / 3000, rate_max = Fs / 300, 1-based
    i, o = A.input("iq" + name, z, pi), A.output("lags" + name, 4 * cnt, po)
    n_out, idx, val = C.c_size_t(0), C.c_size_t(0), C.c_float(0)
    ctx.call("tsdr_autocorr_search_d", i.ptr, 1, n, Fs, 0.0, maxd, 1, o.ptr, C.byref(n_out), lo - 1, hi - lo + 1, C.byref(idx), C.byref(val))
    assert n_out.value == cnt
    return o, int(idx.value), float(val.value), lo, hi


@pytest.mark.parametrize("n,Fs", AC_LENGTHS + [(1_000_000, 5e6)])
def test_autocorr_search_iq_at_both_phases(ctx, n, Fs):
    """the search's findmax must equal numpy.argmax on the lags it returned -- fused into the last pass for aligned IQ at
    n = 2 * smooth, the separate "argmax" kernel for an odd-sample pointer -- and the lags hold the oracle's to 2e-4 dB"""
    z = _search_signal(n, key=2)
    want, _ = O.calculate_autocorrelation(O.abs2(z), Fs, 0, (n // 2) / Fs)
    smooth = n % 2 == 0 and ctx.lib.tsdr_fft_plan(n // 2, (C.c_uint * 8)(), 8) > 0 and (n // 2) & (n // 2 - 1) != 0
    for pi, po in _pairs(PH_C64, PH_F32, full=n < 500_000):
        with Arenas(ctx) as A, profiled(ctx) as prof:
            o, idx, val, lo, hi = _search(ctx, A, z, Fs, pi, po)
            A.check()
            G = o.get(F32)
            assert np.max(np.abs(G - want)) < 2e-4, (n, pi, po, np.max(np.abs(G - want)))
            win = G[lo - 1: hi]
            assert idx == int(np.argmax(win)) and val == win[idx], (n, pi, po, idx, int(np.argmax(win)))
            names = prof.names()
            if smooth:
                assert ("amax_publish" in names) == (pi == 0) and ("argmax" in names) == (pi == 8), (n, pi, names)
            else:
                assert "argmax" in names and "amax_publish" not in names, (n, pi, names)


def test_findmax_routes_interleaved_by_alignment_alone(ctx):
    """test_findmax_routes_interleaved_on_one_context's stale-key hazard, with the SAME lengths throughout: searches on aligned
    IQ (findmax fused into the last pass) and on odd-sample IQ (zero-padded route + the argmax kernel) alternate on one context,
    the larger maxima first, so a key left behind by an earlier search would win a later one's atomicMax."""
    Fs = 1e6
    order = [(200_000, 3e-1, 8), (200_000, 3e-2, 0), (180_000, 3e-3, 8), (80_000, 3e-1, 0), (200_000, 3e-2, 8), (180_000, 3e-4, 0),
             (80_000, 3e-4, 8), (80_000, 3e-5, 0), (200_000, 3e-6, 8)]
    for k, (n, amp, pi) in enumerate(order):
        z = _search_signal(n, amp, key=10 + k)
        with Arenas(ctx) as A:
            o, idx, val, lo, hi = _search(ctx, A, z, Fs, pi, (4 * k) % 16)
            A.check()
            win = o.get(F32)[lo - 1: hi]
            assert idx == int(np.argmax(win)) and val == win[idx], (k, n, amp, pi, idx, int(np.argmax(win)), val, float(win.max()))


def test_autocorr_partial_finish_argmax_at_offsets(ctx):
    """test_autocorr_partial_sums_to_whole with x, the partial sums, the reduced vector and the dB vector each at its own
    non-zero phase"""
    n, n_lags, G = 40_000, 20_000, 4
    x = (_rng(7).random(n) ** 2).astype(F32)
    X = np.fft.fft(x.astype(F64))
    ref = np.fft.ifft(X * np.conj(X)).real[:n_lags]
    for px, pp in ((4, 12), (12, 8), (8, 4), (0, 0)):
        parts = []
        with Arenas(ctx) as A:
            i = A.input("x", x, px)
            outs = [A.output(f"part {g}", 4 * n_lags, (pp + 4 * g) % 16) for g in range(G)]
            for g in range(G):
                ctx.call("tsdr_autocorr_partial_d", i.ptr, 0, n, g * n // G, n // G, n_lags, outs[g].ptr)
            A.check()
            parts = [p.get(F32) for p in outs]
        total = np.sum(np.stack(parts).astype(F64), axis=0)
        assert relmax(total, ref) < CORR_TOL, (px, pp, relmax(total, ref))
        with Arenas(ctx) as A:
            t, o = A.input("corr", total.astype(F32), pp), A.output("dB", 4 * n_lags, px)
            ctx.call("tsdr_autocorr_finish_d", t.ptr, 0, n_lags, 1, o.ptr)
            idx, val = C.c_size_t(0), C.c_float(0)
            ctx.call("tsdr_argmax_d", o.ptr, n_lags, C.byref(idx), C.byref(val))
            A.check()
            db = o.get(F32)
            assert np.max(np.abs(db - 20 * np.log10(np.abs(ref)))) < 2e-4
            assert idx.value == int(np.argmax(db)) and val.value == db[idx.value]
    # IQ input of the partial sums at an odd sample, a window that does not start at 0
    z = _crandn(_rng(8), n, C64)
    p2 = O.abs2(z).astype(F64)
    X = np.fft.fft(p2)
    with Arenas(ctx) as A:
        i, o = A.input("iq", z, 8), A.output("part", 4 * n_lags, 4)
        ctx.call("tsdr_autocorr_partial_d", i.ptr, 1, n, 0, n, n_lags, o.ptr)
        A.check()
        assert relmax(o.get(F32), np.fft.ifft(X * np.conj(X)).real[:n_lags]) < CORR_TOL


@pytest.mark.parametrize("n", [1, 3, 5, 1023, 2049, 100_003])
def test_argmax_at_offsets(ctx, n):
    """findmax (first maximum, NaN maximal) over a vector at every float phase: the maximum as first element, as last element,
    duplicated (the first wins), and a NaN at an n that is not a multiple of 4"""
    rng = _rng(n, 9)
    base = rng.standard_normal(n).astype(F32)
    cases = {}
    v = base.copy(); v[0] = 10.0; cases["first"] = (v, 0)
    v = base.copy(); v[-1] = 10.0; cases["last"] = (v, n - 1)
    if n >= 3:
        v = base.copy(); v[n // 3] = 10.0; v[n - 1] = 10.0; cases["duplicated"] = (v, n // 3)
        v = base.copy(); v[n // 2] = 10.0; v[n - 2] = np.nan; cases["NaN"] = (v, n - 2)
    v = -np.abs(base) - 1.0; cases["all negative"] = (v, int(np.argmax(v)))
    for what, (v, want) in cases.items():
        for ph in PH_F32:
            with Arenas(ctx) as A:
                i = A.input("v", v, ph)
                idx, val = C.c_size_t(0), C.c_float(0)
                ctx.call("tsdr_argmax_d", i.ptr, n, C.byref(idx), C.byref(val))
                A.check()
                assert idx.value == want, (what, n, ph, idx.value, want)
                assert (np.isnan(val.value) and np.isnan(v[want])) or val.value == v[want], (what, n, ph, val.value)


def test_autocorr_f64_at_offsets(ctx):
    """tsdr_autocorr_f64_d: 1e-11 of the largest value against the complex128 restatement (test_autocorr_f64)"""
    Fs, maxd, n = 1e6, 0.06, 100_003
    x = np.abs(_crandn(_rng(11), n, C128)) ** 2
    want = R.autocorr(x, Fs, 0, maxd, log_scale=False)
    for pi, po in _pairs(PH_F64, PH_F64):
        with Arenas(ctx) as A:
            i, o = A.input("x", x, pi), A.output("lags", 8 * want.size, po)
            n_out = C.c_size_t(0)
            ctx.call("tsdr_autocorr_f64_d", i.ptr, n, Fs, 0.0, maxd, 0, o.ptr, C.byref(n_out))
            A.check()
            assert n_out.value == want.size
            assert np.max(np.abs(o.get(F64) - want)) / np.max(want) < 1e-11, (pi, po)


# ================================================================================================================ spectra
# 1024: the wave-per-segment kernel; 3000 = 2^3 3 5^3 <= 4096; 2000: a three-step length; 997: Bluestein; 80 000: passes
SPEC_N = [1024, 3000, 2000, 997, 80_000]


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("N", SPEC_N)
def test_spectrum_at_every_phase(ctx, N, cplx):
    """bars of test_spectrum_vs_oracle: 2 * FFT_TOL on the magnitudes, 2e-2 dB where a bin is above the DC line's noise"""
    rng = _rng(N, cplx)
    sig = (_crandn(rng, N + 10) if cplx else rng.standard_normal(N + 10).astype(F32)) + F32(3.0)
    sig = sig.astype(C64 if cplx else F32)
    o, odb = O.getSpectrum(sig, N=N, lin=True), O.getSpectrum(sig, N=N)
    strong = o > 1e-4 * o.max()
    for pi, po in _pairs(PH_C64 if cplx else PH_F32, PH_F32):
        with Arenas(ctx) as A:
            i, y, ydb = A.input("sig", sig, pi), A.output("y", 4 * N, po), A.output("y dB", 4 * N, (po + 4) % 16)
            ctx.call("tsdr_spectrum_d", i.ptr, int(cplx), N, 1, y.ptr)
            ctx.call("tsdr_spectrum_d", i.ptr, int(cplx), N, 0, ydb.ptr)
            A.check()
            e = relmax(np.sqrt(y.get(F32)), np.sqrt(o))
            assert e < 2 * FFT_TOL, (N, cplx, pi, po, e)
            assert np.max(np.abs(ydb.get(F32)[strong] - odb[strong])) < 2e-2, (N, cplx, pi, po)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("N,nbs", [(1024, (1, 37)), (3000, (1, 37)), (2000, (1, 37)), (17, (1, 37)), (80_000, (1, 3))])
def test_welch_and_waterfall_at_every_phase(ctx, N, nbs, cplx):
    """bars of test_welch_and_waterfall: 4 * FFT_TOL; one segment and a ragged batch (the tail is dropped)"""
    for nb in nbs:
        L = N * nb + min(123, N - 1)
        rng = _rng(N, nb, cplx)
        sig = _crandn(rng, L) if cplx else rng.standard_normal(L).astype(F32)
        ow, om = O.getWelch(sig, sizeFFT=N, lin=True), O.getWaterfall(sig, sizeFFT=N)
        big = N * nb > 100_000
        for pi, po in _pairs(PH_C64 if cplx else PH_F32, PH_F32, full=not big):
            with Arenas(ctx) as A:
                i, y, m = A.input("sig", sig, pi), A.output("welch", 4 * N, po), A.output("waterfall", 8 * N * nb, po & 8)
                ctx.call("tsdr_welch_d", i.ptr, int(cplx), L, N, 1, y.ptr)
                ctx.call("tsdr_waterfall_d", i.ptr, int(cplx), L, N, m.ptr)
                A.check()
                e = relmax(y.get(F32), ow)
                assert e < 4 * FFT_TOL, ("welch", N, nb, cplx, pi, po, e)
                e = relmax(np.sqrt(m.get(F64, (N, nb), "F")), np.sqrt(om))
                assert e < 4 * FFT_TOL, ("waterfall", N, nb, cplx, pi, po, e)


@pytest.mark.parametrize("n,batch", [(1024, 1), (1024, 9), (3000, 1), (3000, 3), (2000, 1), (2000, 6), (997, 1), (997, 3), (80_000, 1),
                                     (80_000, 3)])
def test_fft_c2c_at_every_phase(ctx, n, batch):
    """tsdr_fft_c2c_d, both directions, input and output each at 0 and 8 mod 16: FFT_TOL (test_fft_pow2, test_fft_mixed_radix,
    test_fft_rows_one_launch, test_fft_mixed_radix_batched), 2 * FFT_TOL on the chirp-z route (test_fft_any_length)"""
    x = _crandn(_rng(n, batch), n * batch).reshape(batch, n)
    tol = 2 * FFT_TOL if n == 997 else FFT_TOL
    for dr, ref in ((-1, np.fft.fft(x.astype(C128), axis=1)), (1, np.fft.ifft(x.astype(C128), axis=1))):
        for pi, po in _pairs(PH_C64, PH_C64):
            with Arenas(ctx) as A:
                i, o = A.input("in", x, pi), A.output("out", 8 * n * batch, po)
                ctx.call("tsdr_fft_c2c_d", i.ptr, o.ptr, n, batch, dr)
                A.check()
                e = relmax(o.get(C64, (batch, n)), ref)
                assert e < tol, (n, batch, dr, pi, po, e)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("N", [1024, 1000, 17, 8192])
def test_spectra_f64_at_offsets(ctx, N, cplx):
    """tsdr_spectrum_f64_d (1e-11, test_spectrum_f64), tsdr_welch_f64_d / tsdr_waterfall_f64_d (1e-12, test_welch_waterfall_f64)"""
    nb = 5
    L = N * nb + N // 3 + 1
    rng = _rng(N, cplx, 64)
    sig = _crandn(rng, L, C128) if cplx else rng.standard_normal(L)
    ws, ww, wm = R.spectrum(sig, N, log_scale=False), S64.welch(sig, N, lin=True), S64.waterfall(sig, N)
    for pi, po in _pairs(PH_C128 if cplx else PH_F64, PH_F64):
        with Arenas(ctx) as A:
            i = A.input("sig", sig, pi)
            s, y, m = A.output("spectrum", 8 * N, po), A.output("welch", 8 * N, 8 - po), A.output("waterfall", 8 * N * nb, po)
            ctx.call("tsdr_spectrum_f64_d", i.ptr, int(cplx), N, 1, s.ptr)
            ctx.call("tsdr_welch_f64_d", i.ptr, int(cplx), L, N, 1, y.ptr)
            ctx.call("tsdr_waterfall_f64_d", i.ptr, int(cplx), L, N, m.ptr)
            A.check()
            assert np.max(np.abs(s.get(F64) - ws)) / np.max(ws) < 1e-11, (N, cplx, pi, po)
            assert np.max(np.abs(y.get(F64) - ww)) <= 1e-12 * np.max(ww), (N, cplx, pi, po)
            assert np.max(np.abs(m.get(F64, (N, nb), "F") - wm)) <= 1e-12 * np.max(wm), (N, cplx, pi, po)


# ================================================================================================================== vsync
def _band_image(rng, h, w, row_band, col_band, noise=0.02):
    """test_frame_path_gpu.py:band_image"""
    img = 0.3 + noise * rng.random((h, w), dtype=F32)
    img[np.arange(row_band[0], row_band[0] + row_band[1]) % h, :] = 1.0
    img[:, np.arange(col_band[0], col_band[0] + col_band[1]) % w] = 1.0
    return np.asfortranarray(img.astype(F32))


@pytest.mark.parametrize("h,w", [(120, 200), (77, 131), (600, 800)])
def test_vsync_at_every_phase(ctx, tsdr, h, w):
    """tsdr_vsync_d: the image at four float phases, the int[2] result inside an arena of its own; indices and both beta
    fields identical to the oracle's over a sequence of calls on one state (test_vsync_indices_and_stale_sy)"""
    rng = _rng(h, w)
    g, o = tsdr.SyncXY(ctx, h, w), O.SyncXY(h, w)
    imgs = [_band_image(rng, h, w, (h // 3, max(2, h // 20)), (w // 2, max(6, w // 8))),
            _band_image(rng, h, w, (h // 5, max(2, h // 25)), (w // 7, max(6, w // 9))),
            _band_image(rng, h, w, (2 * h // 3, max(2, h // 15)), (w - 5, max(6, w // 10))),
            _band_image(rng, h, w, (h // 2, max(2, h // 18)), (w // 3, max(6, w // 11)))]
    for k, (im, ph) in enumerate(zip(imgs, PH_F32)):
        with Arenas(ctx) as A:
            i, r = A.input("img", im.ravel(order="F"), ph), A.output("s_yx", 8, (ph + 4) % 16)
            tsdr.api.check(ctx.h, ctx.lib.tsdr_vsync_d(C.c_void_p(g.h), i.ptr, r.ptr), "tsdr_vsync_d")
            A.check()
            got, want = tuple(int(v) for v in r.get(np.int32)), o.vsync(im)
            assert got == want, f"call {k} img@{ph}: {got} vs oracle {want}"
            assert_bitexact(g.beta("x"), o.beta("x"), f"beta_x after call {k}")
            assert_bitexact(g.beta("y"), o.beta("y"), f"beta_y after call {k}")


def test_vsync_f64_at_offsets(ctx, tsdr):
    y_t, x_t = 77, 131
    s, r = tsdr.api.SyncXY(ctx, y_t, x_t, dtype=F64), R.SyncXY64(y_t, x_t)
    rng = _rng(64, 77)
    for k, ph in enumerate((8, 0, 8)):
        img = rng.random((y_t, x_t)) + 1.0
        img[:, (17 + 29 * k) % x_t: (17 + 29 * k) % x_t + 10] *= 0.1
        img[(5 + 11 * k) % y_t: (5 + 11 * k) % y_t + 3, :] *= 0.1
        img = np.asfortranarray(img)
        with Arenas(ctx) as A:
            i, out = A.input("img", img.ravel(order="F"), ph), A.output("s_yx", 8, 4 + 4 * k)
            tsdr.api.check(ctx.h, ctx.lib.tsdr_vsync_f64_d(C.c_void_p(s.h), i.ptr, out.ptr), "tsdr_vsync_f64_d")
            A.check()
            assert tuple(int(v) for v in out.get(np.int32)) == r.vsync(img), (k, ph)
            _same_bits(np.asarray(s.beta("x")).ravel(order="F"), r.beta_x.ravel(order="F"), f"beta_x after call {k}")
            _same_bits(np.asarray(s.beta("y")).ravel(order="F"), r.beta_y.ravel(order="F"), f"beta_y after call {k}")
    s.close()


# ============================================================================================================= frame loop
FRAME_CASE = dict(Fs=2.0e6, x_t=1056, y_t=628, fv=60.0, nfr=3)     # S = 33333: odd, so every second frame starts at an odd sample


def _frames_at_offsets(ctx, tsdr, synth, want_raster):
    """one buffer through tsdr_frames_d: IQ from an odd sample, state / frames / rasters / indices each inside an arena at a
    non-zero phase -> (dict like Context.frames, final state, oracle dict, oracle state)"""
    c = FRAME_CASE
    S, y_t, x_t, nfr = synth.samples_per_frame(c["Fs"], c["fv"]), c["y_t"], c["x_t"], c["nfr"]
    assert S % 2 == 1
    iq = synth.synth_leak(c["Fs"], x_t, y_t, c["fv"], S * nfr + 321)
    npx, P = 480000, y_t * x_t
    o_state = np.zeros((600, 800), F32, order="F")
    o = O.frames(O.SyncXY(600, 800), iq, S, y_t, x_t, F32(0.1), o_state, want_raster=want_raster)
    sync = tsdr.SyncXY(ctx, 600, 800)
    with Arenas(ctx) as A:
        i = A.input("iq", iq, 8)
        st = A.input("imageOut_state", np.zeros(npx, F32), 4)
        st.data = None     # in / out: only its surroundings are guarded
        fr, ix = A.output("frames_out", 4 * nfr * npx, 12), A.output("sync_idx", 8 * nfr, 4)
        ra = A.output("raster_out", 4 * nfr * P, 8) if want_raster else None
        n = C.c_int(0)
        ctx.call("tsdr_frames_d", C.c_void_p(sync.h), i.ptr, iq.size, S, y_t, x_t, C.c_float(0.1), 1, st.ptr, fr.ptr,
                 ra.ptr if ra else C.c_void_p(0), ix.ptr, C.byref(n))
        A.check()
        assert n.value == nfr == o["n_frames"]
        frames = fr.get(F32, (nfr, npx))
        g = {"sync_idx": ix.get(np.int32, (nfr, 2)), "frames": [frames[f].reshape((600, 800), order="F") for f in range(nfr)]}
        if ra:
            rast = ra.get(F32, (nfr, P))
            g["raster"] = [rast[f].reshape((y_t, x_t), order="F") for f in range(nfr)]
        g_state = st.get(F32, (600, 800), "F")
    return g, g_state, o, o_state


def test_frames_exact_at_offsets(ctx, tsdr, synth):
    """TSDR_EXACT: bit-identical to the oracle (test_frames_bitexact)"""
    ctx.set_precision("exact")
    try:
        g, gs, o, os_ = _frames_at_offsets(ctx, tsdr, synth, True)
    finally:
        ctx.set_precision("fast")
    assert np.array_equal(g["sync_idx"], o["sync_idx"]), (g["sync_idx"].tolist(), o["sync_idx"].tolist())
    for f in range(FRAME_CASE["nfr"]):
        assert_bitexact(g["raster"][f], o["raster"][f], f"raster frame {f}")
        assert_bitexact(g["frames"][f], o["frames"][f], f"imageOut after frame {f}")
    assert_bitexact(gs, os_, "imageOut state")


def _rel(a, b):
    """sync_margin.fast_vs_oracle's measure"""
    return float(np.max(np.abs(np.asarray(a, F64) - b) / np.maximum(np.abs(np.asarray(b, F64)), 1e-30)))


@pytest.mark.parametrize("want_raster,split", [(True, 0), (False, 0), (True, 1)])
def test_frames_fast_at_offsets(ctx, tsdr, synth, want_raster, split):
    """TSDR_FAST with and without rasters: identical sync indices, rasters / frames / state within RTOL of the oracle
    (test_frames_fast); "raster_split" 1: the sheared raster store, whose handling of a misaligned raster_out meets a guard
    region here, at RTOL_TAPS (test_frames_fast_sheared_raster_route)"""
    assert ctx.precision == "fast"
    ctx.set_option("raster_split", split)
    try:
        g, gs, o, os_ = _frames_at_offsets(ctx, tsdr, synth, want_raster)
    finally:
        ctx.set_option("raster_split", 0)
    tol = RTOL_TAPS if split else RTOL
    assert np.array_equal(g["sync_idx"], o["sync_idx"]), (g["sync_idx"].tolist(), o["sync_idx"].tolist())
    for f in range(FRAME_CASE["nfr"]):
        if want_raster:
            assert _rel(g["raster"][f], o["raster"][f]) < tol, (f, _rel(g["raster"][f], o["raster"][f]))
        assert _rel(g["frames"][f], o["frames"][f]) < tol, (f, _rel(g["frames"][f], o["frames"][f]))
    assert _rel(gs, os_) < tol


# ============================================================================================================= asynchrony
def test_three_calls_enqueued_without_synchronising(tsdr):
    """The host forms synchronise after every call, the `_d` forms do not: a small spectrum, an autocorrelation of IQ large
    enough to make a fresh context grow its FFT workspaces, and a Welch estimate are enqueued back to back, each on arenas of
    its own; one synchronisation; all three are checked."""
    c = tsdr.Context(0)
    try:
        rng = _rng(99)
        N, n, Fs, Nw, nbw = 3000, 393_216, 1e6, 1000, 37
        s1 = _crandn(rng, N)
        z = _search_signal(n, key=3)
        s3 = _crandn(rng, Nw * nbw + 5)
        maxd = (n // 2) / Fs
        with Arenas(c) as A:
            i1, o1 = A.input("spectrum in", s1, 8), A.output("spectrum out", 4 * N, 4)
            i2, o2 = A.input("iq", z, 8), A.output("lags", 4 * (n // 2), 12)
            i3, o3 = A.input("welch in", s3, 0), A.output("welch out", 4 * Nw, 8)
            n_out = C.c_size_t(0)
            c.call("tsdr_spectrum_d", i1.ptr, 1, N, 1, o1.ptr)
            c.call("tsdr_autocorr_iq_d", i2.ptr, n, Fs, 0.0, maxd, 1, o2.ptr, C.byref(n_out))
            c.call("tsdr_welch_d", i3.ptr, 1, s3.size, Nw, 1, o3.ptr)
            A.check()
            assert relmax(np.sqrt(o1.get(F32)), np.sqrt(O.getSpectrum(s1, N=N, lin=True))) < 2 * FFT_TOL
            want, _ = O.calculate_autocorrelation(O.abs2(z), Fs, 0, maxd)
            assert np.max(np.abs(o2.get(F32) - want)) < 2e-4
            assert relmax(o3.get(F32), O.getWelch(s3, sizeFFT=Nw, lin=True)) < 4 * FFT_TOL
    finally:
        c.close()


# ===================================================================================================== alignment contract
def _refused(ctx, fn, what):
    """fn() -> status of a call that passes an under-aligned pointer: TSDR_EINVAL with a text, and nothing was launched"""
    with profiled(ctx) as prof:
        rc = fn()
        assert rc == EINVAL, (what, rc)
        msg = ctx.lib.tsdr_last_error(ctx.h).decode()
        assert "not aligned to one element" in msg, (what, msg)
        names = prof.names()
        assert sum(names.values()) == 0, (what, names)
    return msg


def test_under_aligned_pointers_are_refused_before_anything_is_enqueued(ctx, tsdr):
    """A ComplexF32 pointer that is not 8-byte aligned, or a float pointer that is not 4-byte aligned, is TSDR_EINVAL from a host
    check in every f32 `_d` entry point: the status, the argument's name in tsdr_last_error, and an unchanged launch count.
    (No kernel ever runs on such a pointer here: the check sits in front of every launch, and a call that returned anything
    else would fail this test before a second one is made.)"""
    L = ctx.lib
    h = ctx.h
    n = 4096
    buf = ctx.dev_alloc(1 << 20)          # never written: every call below is refused
    out = ctx.dev_alloc(1 << 20)
    sync = tsdr.SyncXY(ctx, 600, 800)
    r = ctx.init_resampler(F32, 1000, 4)
    ctx.synchronize()
    P = C.c_void_p
    no, idx, val, nfr = C.c_size_t(0), C.c_size_t(0), C.c_float(0), C.c_int(0)
    try:
        c4, f2 = P(buf + 4), P(buf + 2)   # 4 mod 8: no ComplexF32; 2 mod 4: no float
        o2 = P(out + 2)
        cases = {
            "am_demod iq": lambda: L.tsdr_am_demod_d(h, c4, n, P(out)),
            "am_demod out": lambda: L.tsdr_am_demod_d(h, P(buf), n, o2),
            "abs2 iq": lambda: L.tsdr_abs2_d(h, c4, n, P(out)),
            "abs2 out": lambda: L.tsdr_abs2_d(h, P(buf), n, o2),
            "invert_am iq": lambda: L.tsdr_invert_am_d(h, c4, n, P(out)),
            "invert_am out": lambda: L.tsdr_invert_am_d(h, P(buf), n, o2),
            "fm_demod iq": lambda: L.tsdr_fm_demod_d(h, c4, n, P(out)),
            "fm_demod out": lambda: L.tsdr_fm_demod_d(h, P(buf), n, o2),
            "resize1d sig": lambda: L.tsdr_resize1d_d(h, f2, 100, 873, P(out)),
            "resize1d out": lambda: L.tsdr_resize1d_d(h, P(buf), 100, 873, o2),
            "sig_to_image sig": lambda: L.tsdr_sig_to_image_d(h, f2, 3333, 70, 130, P(out)),
            "sig_to_image img": lambda: L.tsdr_sig_to_image_d(h, P(buf), 3333, 70, 130, o2),
            "resize2d img": lambda: L.tsdr_resize2d_d(h, f2, 45, 64, 20, 30, P(out)),
            "resize2d out": lambda: L.tsdr_resize2d_d(h, P(buf), 45, 64, 20, 30, o2),
            "downgrade img": lambda: L.tsdr_downgrade_d(h, f2, 45, 64, P(out)),
            "downgrade out": lambda: L.tsdr_downgrade_d(h, P(buf), 45, 64, o2),
            "naive_resample in": lambda: L.tsdr_naive_resample_d(h, f2, 1000, 3, P(out)),
            "naive_resample out": lambda: L.tsdr_naive_resample_d(h, P(buf), 1000, 3, o2),
            "resampler in": lambda: L.tsdr_resampler_run_d(P(r.h), f2, 1000, P(out)),
            "resampler out": lambda: L.tsdr_resampler_run_d(P(r.h), P(buf), 1000, o2),
            "autocorr x": lambda: L.tsdr_autocorr_d(h, f2, n, 4096.0, 0.0, 0.5, 1, P(out), C.byref(no)),
            "autocorr out": lambda: L.tsdr_autocorr_d(h, P(buf), n, 4096.0, 0.0, 0.5, 1, o2, C.byref(no)),
            "autocorr_iq iq": lambda: L.tsdr_autocorr_iq_d(h, c4, n, 4096.0, 0.0, 0.5, 1, P(out), C.byref(no)),
            "autocorr_search iq": lambda: L.tsdr_autocorr_search_d(h, c4, 1, n, 4096.0, 0.0, 0.5, 1, P(out), C.byref(no), 10, 100,
                                                                   C.byref(idx), C.byref(val)),
            "autocorr_search x": lambda: L.tsdr_autocorr_search_d(h, f2, 0, n, 4096.0, 0.0, 0.5, 1, P(out), C.byref(no), 10, 100,
                                                                  C.byref(idx), C.byref(val)),
            "autocorr_partial iq": lambda: L.tsdr_autocorr_partial_d(h, c4, 1, n, 0, n, 100, P(out)),
            "autocorr_partial part": lambda: L.tsdr_autocorr_partial_d(h, P(buf), 0, n, 0, n, 100, o2),
            "autocorr_finish corr": lambda: L.tsdr_autocorr_finish_d(h, f2, 0, 100, 1, P(out)),
            "autocorr_finish out": lambda: L.tsdr_autocorr_finish_d(h, P(buf), 0, 100, 1, o2),
            "argmax v": lambda: L.tsdr_argmax_d(h, f2, 100, C.byref(idx), C.byref(val)),
            "spectrum complex sig": lambda: L.tsdr_spectrum_d(h, c4, 1, 1024, 1, P(out)),
            "spectrum real sig": lambda: L.tsdr_spectrum_d(h, f2, 0, 1024, 1, P(out)),
            "spectrum y": lambda: L.tsdr_spectrum_d(h, P(buf), 1, 1024, 1, o2),
            "welch complex sig": lambda: L.tsdr_welch_d(h, c4, 1, n, 1024, 1, P(out)),
            "welch real sig": lambda: L.tsdr_welch_d(h, f2, 0, n, 1024, 1, P(out)),
            "welch y": lambda: L.tsdr_welch_d(h, P(buf), 1, n, 1024, 1, o2),
            "waterfall complex sig": lambda: L.tsdr_waterfall_d(h, c4, 1, n, 1000, P(out)),
            "waterfall sMatrix": lambda: L.tsdr_waterfall_d(h, P(buf), 1, n, 1000, P(out + 4)),
            "fft_c2c in": lambda: L.tsdr_fft_c2c_d(h, c4, P(out), 1024, 3, -1),
            "fft_c2c out": lambda: L.tsdr_fft_c2c_d(h, P(buf), P(out + 4), 1024, 3, -1),
            "vsync img": lambda: L.tsdr_vsync_d(P(sync.h), f2, P(out)),
            "vsync s_yx": lambda: L.tsdr_vsync_d(P(sync.h), P(buf), o2),
            "frames iq": lambda: L.tsdr_frames_d(h, P(sync.h), c4, 4096, 1024, 32, 32, C.c_float(0.5), 1, P(out), None, None, None,
                                                 C.byref(nfr)),
            "frames state": lambda: L.tsdr_frames_d(h, P(sync.h), P(buf), 4096, 1024, 32, 32, C.c_float(0.5), 1, o2, None, None, None,
                                                    C.byref(nfr)),
            "frames_submit iq": lambda: L.tsdr_frames_submit_d(h, P(sync.h), c4, 4096, 1024, 32, 32, C.c_float(0.5), 1, P(out), None,
                                                               None, None, C.byref(nfr)),
        }
        for what, fn in cases.items():
            _refused(ctx, fn, what)
        # the message names the C argument
        assert "am_demod: iq is not aligned" in _refused(ctx, cases["am_demod iq"], "am_demod iq")
        assert "waterfall: sMatrix is not aligned" in _refused(ctx, cases["waterfall sMatrix"], "waterfall sMatrix")
    finally:
        r.close()
        ctx.dev_free(buf)
        ctx.dev_free(out)
