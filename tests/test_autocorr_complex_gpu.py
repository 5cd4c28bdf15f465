"""GPU tests of calculate_autocorrelation on COMPLEX input (include/tempest_hip_cplx.h): the coherent autocorrelation of the IQ
samples themselves, r[k] = sum_m z[(m+k) mod n] conj(z[m]), as ComplexF32, ComplexF64 and integer IQ.

Reference: numpy in complex128, ifft(F * conj(F)) with F = fft(z), then abs**2 / 10log10.  Bars (the real route's own, it has the
same structure -- two transforms plus squaring): lin max|got - ref| / max(ref) < 2 * CORR_TOL, dB max|got - ref| < 2e-4, f64 lin
< 1e-11.  Inputs:
  carrier  ((1 + 0.5j) + 0.3 u) exp(2 pi j 37 m / n) * 3e-3: every lag stays near r[0], so dB is well conditioned (asserted on the
           reference: min_{k < n/2} |r[k]| / r[0] >= 0.5)
  noise    3e-3 u: lags fall to 1e-6 r[0], compared in lin only (an exact-to-f32 implementation misses 2e-4 dB there)
with u complex standard normal from default_rng(n).  The integer formats are compared BIT FOR BIT with the ComplexF32 form on
host-expanded samples, at sample offsets inside guarded arenas (dptr_util)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import dptr_util as D

pytestmark = pytest.mark.gpu


def _mod(name):
    from tempest_loader import load_package
    load_package()
    return importlib.import_module("tempestsdr_jl_amd." + name)


API = _mod("api")
SEARCH = _mod("search")

CORR_TOL = 2e-5          # tests/test_fft_path_gpu.py
LIN_BAR = 2 * CORR_TOL
DB_BAR = 2e-4
F64_BAR = 1e-11          # tests/test_f64_gpu.py
FS = 1000.0

SIZES = [200, 1000, 1500, 3000, 4096, 4001, 14_000, 80_000, 100_003, 1_000_000]
BIG = 5_000_000


# ---- inputs and the numpy reference ---------------------------------------------------------------------------------------
def _u(n):
    rng = np.random.default_rng(n)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def carrier128(n):
    m = np.arange(n)
    return ((1 + 0.5j) + 0.3 * _u(n)) * np.exp(2j * np.pi * 37 * m / n) * 3e-3


@functools.lru_cache(maxsize=8)
def signal(kind, n):
    z = carrier128(n) if kind == "carrier" else 3e-3 * _u(n)
    z = z.astype(np.complex64)
    z.setflags(write=False)
    return z


def window(length, Fs, mind, maxd):
    """(n, k0, cnt) as autocorr_args forms them"""
    imin, imax = 1 + int(np.round(mind * Fs)), int(np.round(maxd * Fs))
    return min(2 * imax, length), imin - 1, max(imax - imin + 1, 0)


def ref_r(z, n):
    F = np.fft.fft(np.asarray(z[:n]).astype(np.complex128))
    return np.fft.ifft(F * np.conj(F))


@functools.lru_cache(maxsize=4)
def ref_full(kind, n):
    """the reference's complex lags of the whole n-sample signal (shared by the tests of that size; read-only)"""
    r = ref_r(signal(kind, n), n)
    r.setflags(write=False)
    return r


def lin_err(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref)) / np.max(ref))


def check_lags(tag, got_lin, got_db, r, k0, cnt, db=True):
    p = np.abs(r[k0:k0 + cnt]) ** 2
    assert got_lin.shape == p.shape and got_lin.dtype == np.float32
    e = lin_err(got_lin, p)
    print(f"{tag}: lin {e:.3e}", end="")
    assert e < LIN_BAR, (tag, e)
    if db:
        ed = float(np.max(np.abs(got_db.astype(np.float64) - 10.0 * np.log10(p))))
        print(f"  dB {ed:.3e}", end="")
        assert ed < DB_BAR, (tag, ed)
    print()


def full_delay(n):
    """maxDelay with indexMax = round(0.75 n) at FS: len = n < 2 indexMax, so the window is the whole signal"""
    return 0.75 * n / FS


# ---- 1. against numpy --------------------------------------------------------------------------------------------------------
def test_sizes_cover_every_pass_count(tsdr):
    lib = tsdr._lib.load()
    f = (C.c_uint * 8)()
    passes = {n: lib.tsdr_fft_plan(n, f, 8) for n in SIZES + [BIG]}
    print(passes)
    assert 0 in passes.values() and 1 in passes.values() and 2 in passes.values() and max(passes.values()) >= 3, passes
    assert passes[4001] == 0 and passes[100_003] == 0 and passes[200] == 1 and passes[80_000] >= 2 and passes[4096] >= 2


OPTS = [None, ("ac_mixed", 0), ("ac_fuse_mid", 0)]


@pytest.mark.parametrize("opt", OPTS, ids=lambda o: "default" if o is None else f"{o[0]}={o[1]}")
@pytest.mark.parametrize("kind", ["carrier", "noise"])
@pytest.mark.parametrize("n", SIZES)
def test_against_numpy(ctx, n, kind, opt):
    z, r = signal(kind, n), ref_full(kind, n)
    if kind == "carrier":
        assert np.abs(r[: n // 2]).min() / np.abs(r[0]) >= 0.5
    maxd = full_delay(n)
    nn, k0, cnt = window(n, FS, 0.0, maxd)
    assert nn == n and cnt == int(np.round(0.75 * n))
    if opt:
        ctx.set_option(*opt)
    try:
        lin, lags = ctx.calculate_autocorrelation(z, FS, 0.0, maxd, "lin")
        db = ctx.calculate_autocorrelation(z, FS, 0.0, maxd, "log")[0] if kind == "carrier" else None
    finally:
        if opt:
            ctx.set_option(opt[0], 1)
    assert lags.size == cnt and lags[1] == 1 / FS
    check_lags(f"n={n} {kind} {opt}", lin, db, r, k0, cnt, db=kind == "carrier")


def test_against_numpy_five_million(ctx):
    n = BIG
    z = carrier128(n).astype(np.complex64)
    r = ref_r(z, n)
    assert np.abs(r[: n // 2]).min() / np.abs(r[0]) >= 0.5
    maxd = full_delay(n)
    _, k0, cnt = window(n, FS, 0.0, maxd)
    lin, _ = ctx.calculate_autocorrelation(z, FS, 0.0, maxd, "lin")
    db, _ = ctx.calculate_autocorrelation(z, FS, 0.0, maxd, "log")
    check_lags(f"n={n} carrier", lin, db, r, k0, cnt)


@pytest.mark.parametrize("case", ["odd_k0_odd_cnt", "truncated", "odd_len"])
@pytest.mark.parametrize("n", [3000, 80_000])
def test_windows(ctx, n, case):
    """minDelay > 0 with odd k0 and odd cnt; len > 2 indexMax (the samples are truncated to n); indexMax < len < 2 indexMax with
    an odd len (the window is the whole, odd-length signal)"""
    if case == "odd_k0_odd_cnt":
        z, mind, maxd = signal("carrier", n), 0.101, full_delay(n)
    elif case == "truncated":
        z, mind, maxd = np.concatenate([signal("carrier", n), signal("noise", 777)]), 0.0, 0.5 * n / FS
    else:
        z, mind, maxd = signal("carrier", n)[: n - 1], 0.0, full_delay(n)
    nn, k0, cnt = window(z.size, FS, mind, maxd)
    if case == "odd_k0_odd_cnt":
        assert nn == n and k0 % 2 == 1 and cnt % 2 == 1
    elif case == "truncated":
        assert nn == n < z.size and cnt == n // 2
    else:
        assert nn == n - 1 and nn % 2 == 1
    r = ref_r(z, nn)
    assert np.abs(r[: nn // 2]).min() / np.abs(r[0]) >= 0.5
    for opt in OPTS:
        if opt:
            ctx.set_option(*opt)
        try:
            lin, _ = ctx.calculate_autocorrelation(z, FS, mind, maxd, "lin")
            db, _ = ctx.calculate_autocorrelation(z, FS, mind, maxd, "log")
        finally:
            if opt:
                ctx.set_option(opt[0], 1)
        check_lags(f"n={n} {case} {opt}", lin, db, r, k0, cnt)


# ---- 2. known answers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,f", [(4096, 5), (80_000, 1234)])
def test_pure_tone(ctx, n, f):
    A = 3e-3
    z = (A * np.exp(2j * np.pi * f * np.arange(n) / n)).astype(np.complex64)
    want = (n * A * A) ** 2
    lin, _ = ctx.calculate_autocorrelation(z, FS, 0.0, full_delay(n), "lin")
    db, _ = ctx.calculate_autocorrelation(z, FS, 0.0, full_delay(n), "log")
    e, ed = float(np.max(np.abs(lin - want)) / want), float(np.max(np.abs(db - 10 * np.log10(want))))
    print(f"tone n={n}: lin {e:.3e} dB {ed:.3e}")
    assert e < LIN_BAR and ed < DB_BAR


@pytest.mark.parametrize("n", [1000, 4001, 80_000])
def test_phase_invariance(ctx, n):
    z128 = carrier128(n)
    a, _ = ctx.calculate_autocorrelation(z128.astype(np.complex64), FS, 0.0, full_delay(n), "lin")
    b, _ = ctx.calculate_autocorrelation((z128 * np.exp(0.7j)).astype(np.complex64), FS, 0.0, full_delay(n), "lin")
    e = float(np.max(np.abs(a.astype(np.float64) - b)) / np.max(a))
    print(f"phase n={n}: {e:.3e}")
    assert e < LIN_BAR


@pytest.mark.parametrize("n,Fs,maxd,mind", [(3000, 30_000.0, 0.05, 0.0), (4096, 4096.0, 0.5, 0.0), (4001, 1000.0, 4.0, 0.0),
                                           (14_000, 1000.0, 7.0, 0.5)])
def test_zero_imaginary_part_is_the_real_route(ctx, n, Fs, maxd, mind):
    x = (np.random.default_rng(7).random(n) ** 2).astype(np.float32) * 1e-5   # power-like, as test_autocorr_vs_oracle
    real, _ = ctx.calculate_autocorrelation(x, Fs, mind, maxd, "lin")
    cplx, _ = ctx.calculate_autocorrelation(x.astype(np.complex64), Fs, mind, maxd, "lin")
    assert real.shape == cplx.shape
    e = float(np.max(np.abs(real.astype(np.float64) - cplx)) / np.max(real))
    print(f"(x, 0) n={n}: {e:.3e}")
    assert e < LIN_BAR


def test_periodic_known_answer(ctx):
    T, reps, Fs = 250, 16, 10_000.0
    base = _u(T).astype(np.complex64)
    G, lags = ctx.calculate_autocorrelation(np.tile(base, reps), Fs, 0, 0.2)   # indexMax = 2000, n = 4000
    assert G.size == 2000 and lags.size == 2000
    k = int(np.argmax(G[1:])) + 1
    assert k % T == 0, k
    for m in range(1, 8):
        assert abs(G[m * T] - G[0]) < 1e-3, m     # same energy at every full period (dB)
    off = np.delete(G, np.arange(0, 2000, T))
    assert off.max() < G[0] - 3.0


# ---- 3. Python dispatch ------------------------------------------------------------------------------------------------------
def test_dispatch_complex64_takes_the_complex_route(ctx):
    """before the complex route existed, complex input lost its imaginary part and got the autocorrelation of real(z)"""
    n = 3000
    z, r = signal("carrier", n), ref_full("carrier", n)
    _, k0, cnt = window(n, FS, 0.0, full_delay(n))
    lin, _ = ctx.calculate_autocorrelation(z, FS, 0.0, full_delay(n), "lin")
    db, _ = ctx.calculate_autocorrelation(z, FS, 0.0, full_delay(n))
    check_lags("dispatch", lin, db, r, k0, cnt)
    wrong = np.abs(ref_r(z.real.astype(np.complex64), n)[k0:k0 + cnt]) ** 2
    assert lin_err(lin, wrong) > 100 * LIN_BAR, "the answer of real(z) is far from the right one on this input"


@pytest.mark.parametrize("n", [100_000, 100_003])
def test_dispatch_complex128(ctx, n):
    z = carrier128(n)
    r = ref_r(z, n)
    _, k0, cnt = window(n, FS, 0.0, full_delay(n))
    lin, _ = ctx.calculate_autocorrelation(z, FS, 0.0, full_delay(n), "lin", dtype=np.float64)
    p = np.abs(r[k0:k0 + cnt]) ** 2
    assert lin.dtype == np.float64 and lin.shape == p.shape
    e = float(np.max(np.abs(lin - p)) / np.max(p))
    print(f"f64 n={n}: {e:.3e}")
    assert e < F64_BAR
    db, _ = ctx.calculate_autocorrelation(z, FS, 0.0, full_delay(n), dtype=np.float64)
    assert np.max(np.abs(db - 10 * np.log10(p))) < 1e-9


def test_dispatch_refuses_mixed_precisions_and_short_signals(ctx):
    z = carrier128(1000)
    with pytest.raises(AssertionError):
        ctx.calculate_autocorrelation(z, FS, 0.0, 0.5)                                            # complex128 without dtype
    with pytest.raises(AssertionError):
        ctx.calculate_autocorrelation(z.astype(np.complex64), FS, 0.0, 0.5, dtype=np.float64)     # complex64 with dtype
    with pytest.raises(AssertionError):
        ctx.calculate_autocorrelation(np.zeros(2000, np.int8), FS, 0.0, 0.5, iq_fmt="sc16")       # strict about the dtype
    with pytest.raises(IndexError):
        ctx.calculate_autocorrelation(z.astype(np.complex64), FS, 0.0, 1.5)                       # len < indexMax
    with pytest.raises(IndexError):
        ctx.calculate_autocorrelation(z, FS, 0.0, 1.5, dtype=np.float64)
    with pytest.raises(IndexError):
        ctx.calculate_autocorrelation(np.zeros(2000, np.int8), FS, 0.0, 1.5, iq_fmt="sc8")


# ---- 4. integer formats, bit for bit, at offsets in guarded arenas ---------------------------------------------------------------
DT = {"sc16": np.int16, "sc8": np.int8, "uc8": np.uint8}
CODE = {"cf32": 0, "sc16": 1, "sc8": 2, "uc8": 3}
SCALE = {"sc16": 3e-3 / 2048, "sc8": 3e-3 / 64, "uc8": 3e-3 / 64}
COMBOS = [(0, 0), (1, 4), (3, 8), (1, 12)]    # (input sample offset inside the larger buffer, output phase = float offset * 4)


def quantise(n, fmt):
    """integer components of a carrier-like signal (so dB stays finite) in the format's own dtype, 2 * n of them"""
    z = carrier128(n) / 3e-3
    amp = {"sc16": 2048.0, "sc8": 64.0, "uc8": 64.0}[fmt]
    q = np.empty(2 * n, np.float64)
    q[0::2], q[1::2] = z.real * amp * 0.5, z.imag * amp * 0.5
    q = np.round(q) + (128 if fmt == "uc8" else 0)
    info = np.iinfo(DT[fmt])
    return np.clip(q, info.min, info.max).astype(DT[fmt])


def search_d(ctx, ptr, code, scale, n, maxd, log, out_ptr, win_lo, win_cnt, mind=0.0):
    n_out, idx, val = C.c_size_t(0), C.c_size_t(0), C.c_float(0)
    ctx.call("tsdr_autocorr_cplx_search_iq_d", ptr, code, C.c_float(scale), n, FS, mind, maxd, log, out_ptr, C.byref(n_out), win_lo,
             win_cnt, C.byref(idx), C.byref(val))
    return n_out.value, idx.value, np.float32(val.value)


def host_iq(ctx, part, fmt, scale, n, maxd, log, cnt):
    host = np.empty(cnt, np.float32)
    n_out = C.c_size_t(0)
    part = np.ascontiguousarray(part)
    ctx.call("tsdr_autocorr_cplx_iq", C.c_void_p(part.ctypes.data), CODE[fmt], C.c_float(scale), n, FS, 0.0, maxd, log,
             C.c_void_p(host.ctypes.data), C.byref(n_out))
    assert n_out.value == cnt
    return host


@pytest.mark.parametrize("n", [200, 1000, 4001, 80_000])   # one pass (expanded first), two passes, Bluestein (expanded), two passes
@pytest.mark.parametrize("fmt", ["sc16", "sc8", "uc8"])
def test_integer_formats_bit_for_bit(ctx, fmt, n):
    raw = quantise(n + 8 + n % 2, fmt)   # (an arena holds whole 4-byte words)
    scale = np.float32(SCALE[fmt])
    bps = raw.itemsize * 2
    maxd = full_delay(n)
    _, k0, cnt = window(n, FS, 0.0, maxd)
    win_lo, win_cnt = cnt // 3, cnt // 2 + 1
    for log in (1, 0):
        for off, phase in COMBOS:
            part = raw[2 * off: 2 * (off + n)]
            z = API.expand_iq(part, fmt, scale)
            with D.Arenas(ctx) as A:
                # the ComplexF32 form on host-expanded samples, on fresh, aligned allocations
                zin, ref_out = A.input("z", z, 0), A.output("ref", 4 * cnt, 0)
                r_cnt, r_idx, r_val = search_d(ctx, zin.ptr, CODE["cf32"], 1.0, n, maxd, log, ref_out.ptr, win_lo, win_cnt)
                # the integer form: the raw buffer, the pointer `off` samples in, the output at a float offset
                qin, out = A.input("iq", raw, 0), A.output("out", 4 * cnt, phase)
                g_cnt, g_idx, g_val = search_d(ctx, C.c_void_p(qin.addr + off * bps), CODE[fmt], scale, n, maxd, log, out.ptr, win_lo, win_cnt)
                # win_cnt == 0: the plain device call
                out2 = A.output("out2", 4 * cnt, phase)
                search_d(ctx, C.c_void_p(qin.addr + off * bps), CODE[fmt], scale, n, maxd, log, out2.ptr, 0, 0)
                A.check()
                ref, got, got2 = ref_out.get(np.uint32), out.get(np.uint32), out2.get(np.uint32)
            assert r_cnt == g_cnt == cnt
            assert np.array_equal(got, ref), (fmt, n, off, phase, int(np.sum(got != ref)))
            assert np.array_equal(got2, ref)
            assert g_idx == r_idx and g_val.view(np.uint32) == r_val.view(np.uint32)
            win = ref.view(np.float32)[win_lo: win_lo + win_cnt]
            assert g_idx == int(np.argmax(win)) and g_val == win[g_idx]
            # the host form uploads the raw bytes
            assert np.array_equal(host_iq(ctx, part, fmt, scale, n, maxd, log, cnt).view(np.uint32), ref)
    # and through the Python keyword
    G, _ = ctx.calculate_autocorrelation(raw[: 2 * n], FS, 0.0, maxd, "lin", iq_fmt=fmt, iq_scale=float(scale))
    assert np.array_equal(G.view(np.uint32), host_iq(ctx, raw[: 2 * n], fmt, scale, n, maxd, 0, cnt).view(np.uint32))


@pytest.mark.parametrize("n", [200, 1000, 4001, 80_000])
def test_cf32_and_cf64_at_offsets(ctx, n):
    """tsdr_autocorr_cplx_d / tsdr_autocorr_cplx_f64_d at base + k samples of a larger buffer give the bits of the host form (which
    stages the samples at the start of a fresh workspace)"""
    maxd = full_delay(n)
    _, k0, cnt = window(n, FS, 0.0, maxd)
    big128 = carrier128(n + 8)
    for f64 in (False, True):
        big, obytes, odt = (big128, 8, np.float64) if f64 else (big128.astype(np.complex64), 4, np.float32)
        for off, phase in COMBOS:
            part = np.ascontiguousarray(big[off: off + n])
            want = np.empty(cnt, odt)
            n_out = C.c_size_t(0)
            ctx.call("tsdr_autocorr_cplx_f64" if f64 else "tsdr_autocorr_cplx", C.c_void_p(part.ctypes.data), n, FS, 0.0, maxd, 1,
                     C.c_void_p(want.ctypes.data), C.byref(n_out))
            assert n_out.value == cnt
            with D.Arenas(ctx) as A:
                zin = A.input("z", big, 0)
                out = A.output("out", obytes * cnt, (phase // 8) * 8 if f64 else phase)
                ctx.call("tsdr_autocorr_cplx_f64_d" if f64 else "tsdr_autocorr_cplx_d", C.c_void_p(zin.addr + off * big.itemsize), n, FS, 0.0,
                         maxd, 1, out.ptr, C.byref(n_out))
                A.check()
                got = out.get(odt)
            assert n_out.value == cnt and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (f64, off, phase)


def test_misaligned_pointers_and_unknown_formats_are_refused(ctx):
    n, maxd = 1000, full_delay(1000)
    _, _, cnt = window(n, FS, 0.0, maxd)
    raw = quantise(n + 8, "sc16")
    z = signal("carrier", n + 8)
    z128 = carrier128(n + 8)
    with D.Arenas(ctx) as A:
        qin, zin, z64, out = A.input("iq", raw, 0), A.input("z", z, 0), A.input("z64", z128, 0), A.output("out", 8 * cnt, 0)
        n_out = C.c_size_t(0)
        with pytest.raises(AssertionError, match=r"\biq is not aligned"):
            search_d(ctx, C.c_void_p(qin.addr + 2), 1, 1.0, n, maxd, 1, out.ptr, 0, 10)
        with pytest.raises(AssertionError, match=r"\biq is not aligned"):
            search_d(ctx, C.c_void_p(qin.addr + 1), 2, 1.0, n, maxd, 1, out.ptr, 0, 10)
        with pytest.raises(AssertionError, match=r"\biq is not aligned"):
            search_d(ctx, C.c_void_p(zin.addr + 4), 0, 1.0, n, maxd, 1, out.ptr, 0, 10)
        with pytest.raises(AssertionError, match=r"\bout is not aligned"):
            search_d(ctx, qin.ptr, 1, 1.0, n, maxd, 1, C.c_void_p(out.addr + 2), 0, 10)
        for bad in (7, -1, 4):
            with pytest.raises(AssertionError, match=rf"iq_fmt {bad} "):
                search_d(ctx, qin.ptr, bad, 1.0, n, maxd, 1, out.ptr, 0, 10)
            with pytest.raises(AssertionError, match=rf"iq_fmt {bad} "):
                ctx.call("tsdr_autocorr_cplx_iq", C.c_void_p(raw.ctypes.data), bad, C.c_float(1.0), n, FS, 0.0, maxd, 1, out.ptr, C.byref(n_out))
        with pytest.raises(AssertionError, match=r"\bz is not aligned"):
            ctx.call("tsdr_autocorr_cplx_d", C.c_void_p(zin.addr + 4), n, FS, 0.0, maxd, 1, out.ptr, C.byref(n_out))
        with pytest.raises(AssertionError, match=r"\bout is not aligned"):
            ctx.call("tsdr_autocorr_cplx_d", zin.ptr, n, FS, 0.0, maxd, 1, C.c_void_p(out.addr + 1), C.byref(n_out))
        with pytest.raises(AssertionError, match=r"\bz is not aligned"):
            ctx.call("tsdr_autocorr_cplx_f64_d", C.c_void_p(z64.addr + 8), n, FS, 0.0, maxd, 1, out.ptr, C.byref(n_out))
        with pytest.raises(AssertionError, match=r"\bout is not aligned"):
            ctx.call("tsdr_autocorr_cplx_f64_d", z64.ptr, n, FS, 0.0, maxd, 1, C.c_void_p(out.addr + 4), C.byref(n_out))
        A.check()   # nothing was written


# ---- 5. search ---------------------------------------------------------------------------------------------------------------
def to_sc8(z):
    sc = float(np.abs(np.concatenate([z.real, z.imag])).max()) / 127.0
    q = np.empty(2 * z.size, np.int8)
    q[0::2] = np.clip(np.round(z.real / sc), -127, 127)
    q[1::2] = np.clip(np.round(z.imag / sc), -127, 127)
    return q, sc


@functools.lru_cache(maxsize=1)
def small_leak():
    z = _mod("synth").synth_leak(1e6, 400, 250, 50.0, 200_000)
    z.setflags(write=False)
    return z


def zoom_window(cnt, Fs, rate_min, rate_max):
    pmin, pmax = min(int(np.round(Fs / rate_max)), cnt), min(int(np.round(Fs / rate_min)), cnt)
    return pmin - 1, pmax - pmin + 1


def test_search_small_capture(ctx):
    """synth_leak at 1 MS/s, 50 Hz frames: numpy finds the frame peak at window position 5715 (lag 20 000, labelled 49.9975 Hz by the
    reference's off-by-one), top-2 margin 0.13 dB"""
    z, Fs = small_leak(), 1e6
    r = ref_r(z, 200_000)
    lo, wc = zoom_window(100_000, Fs, 40, 70)
    want_db = 10 * np.log10(np.abs(r[:100_000]) ** 2)
    assert int(np.argmax(want_db[lo: lo + wc])) == 5715
    q, sc = to_sc8(z)
    for kw, sig in (({}, z), ({"iq_fmt": "sc8", "iq_scale": sc}, q)):
        G, pos, val = ctx.autocorr_search_complex(sig, Fs, 0, 0.1, rate_min=40, rate_max=70, **kw)
        win = G[lo: lo + wc]
        assert G.size == 100_000 and pos == int(np.argmax(win)) and np.float32(val) == win[pos]
        assert pos == 5715, pos
    G, _, _ = ctx.autocorr_search_complex(z, Fs, 0, 0.1, rate_min=40, rate_max=70)
    assert np.max(np.abs(G - want_db)) < DB_BAR
    # a device address
    d = ctx.upload(q)
    try:
        G2, pos2, _ = ctx.autocorr_search_complex(int(d), Fs, 0, 0.1, rate_min=40, rate_max=70, iq_fmt="sc8", iq_scale=sc, n_samples=z.size)
    finally:
        ctx.dev_free(d)
    assert pos2 == 5715
    search = SEARCH
    rates, Gz, fv, Gfull = search.extract_configuration(ctx, z, Fs, rate_min=40, rate_max=70, domain="complex")
    assert int(np.argmax(Gz)) == 5715 and abs(fv - 49.9975) < 1e-3 and np.array_equal(Gfull, G)
    rates, Gz, fv, _ = search.extract_configuration(ctx, q, Fs, rate_min=40, rate_max=70, iq_fmt="sc8", iq_scale=sc, domain="complex")
    assert int(np.argmax(Gz)) == 5715 and abs(fv - 49.9975) < 1e-3
    with pytest.raises(AssertionError):
        search.extract_configuration(ctx, z, Fs, domain="coherent")


def test_search_full_size(ctx, synth):
    """the workload's window: 4e6 samples at 20 MS/s, 60 Hz frames; numpy's position is 110 816 (60.053 Hz, the same
    line-off-by-one position the power route finds), its top-2 margin 1.4e-2 dB; min |r| / r0 = 0.70, so dB is well conditioned"""
    Fs = 20e6
    z = synth.synth_leak(Fs, 2576, 1125, 60.0, 4_000_000)
    r = ref_r(z, 4_000_000)
    want_db = 10 * np.log10(np.abs(r[:2_000_000]) ** 2)
    lo, wc = zoom_window(2_000_000, Fs, 50, 90)
    assert int(np.argmax(want_db[lo: lo + wc])) == 110_816
    G, pos, val = ctx.autocorr_search_complex(z, Fs, 0, 0.1, rate_min=50, rate_max=90)
    e = float(np.max(np.abs(G - want_db)))
    print(f"full size: dB {e:.3e}")
    assert e < DB_BAR
    win = G[lo: lo + wc]
    assert pos == int(np.argmax(win)) and np.float32(val) == win[pos]
    assert pos == 110_816, pos


def test_power_and_complex_searches_share_the_findmax_slots(ctx):
    z, Fs = small_leak(), 1e6
    lo, wc = zoom_window(100_000, Fs, 40, 70)
    first = None
    for _ in range(3):
        Gp, pp, vp = ctx.autocorr_search(z, Fs, 0, 0.1, rate_min=40, rate_max=70)
        Gc, pc, vc = ctx.autocorr_search_complex(z, Fs, 0, 0.1, rate_min=40, rate_max=70)
        assert pp == int(np.argmax(Gp[lo: lo + wc])) and np.float32(vp) == Gp[lo + pp]
        assert pc == int(np.argmax(Gc[lo: lo + wc])) == 5715 and np.float32(vc) == Gc[lo + pc]
        if first is None:
            first = (Gp, pp, Gc, pc)
        else:
            assert np.array_equal(Gp, first[0]) and pp == first[1] and np.array_equal(Gc, first[2])
    # a one-pass length in between takes the separate findmax kernel
    small = signal("carrier", 200)
    G, pos, val = ctx.autocorr_search_complex(small, FS, 0, 0.15, rate_min=10, rate_max=50)
    slo, swc = zoom_window(150, FS, 10, 50)
    assert pos == int(np.argmax(G[slo: slo + swc])) and np.float32(val) == G[slo + pos]
    Gc, pc, _ = ctx.autocorr_search_complex(z, Fs, 0, 0.1, rate_min=40, rate_max=70)
    assert pc == 5715 and np.array_equal(Gc, first[2])


# ---- 6. bounds ---------------------------------------------------------------------------------------------------------------
def test_bounds_in_every_form(ctx):
    n = 1000
    z, z128, raw = signal("carrier", n), carrier128(n), quantise(n, "sc8")
    n_out = C.c_size_t(7)
    out_h = np.full(16, -1.0, np.float64)
    with D.Arenas(ctx) as A:
        zin, z64, qin, out = A.input("z", z, 0), A.input("z64", z128, 0), A.input("iq", raw, 0), A.output("out", 8 * 16, 0)
        host_calls = [("tsdr_autocorr_cplx", (C.c_void_p(z.ctypes.data),)), ("tsdr_autocorr_cplx_f64", (C.c_void_p(z128.ctypes.data),)),
                      ("tsdr_autocorr_cplx_iq", (C.c_void_p(raw.ctypes.data), 2, C.c_float(1.0)))]
        for maxd, want in ((1.5, IndexError), (0.5, None)):     # len < indexMax; then cnt == 0 (minDelay = maxDelay)
            mind = 0.0 if want else 0.5
            for sym, head in host_calls:
                args = head + (n, FS, mind, maxd, 1, C.c_void_p(out_h.ctypes.data), C.byref(n_out))
                if want:
                    with pytest.raises(want):
                        ctx.call(sym, *args)
                else:
                    n_out.value = 7
                    ctx.call(sym, *args)
                    assert n_out.value == 0 and np.all(out_h == -1.0)
            dev_calls = [lambda: ctx.call("tsdr_autocorr_cplx_d", zin.ptr, n, FS, mind, maxd, 1, out.ptr, C.byref(n_out)),
                         lambda: ctx.call("tsdr_autocorr_cplx_f64_d", z64.ptr, n, FS, mind, maxd, 1, out.ptr, C.byref(n_out)),
                         lambda: ctx.call("tsdr_autocorr_cplx_search_iq_d", qin.ptr, 2, C.c_float(1.0), n, FS, mind, maxd, 1, out.ptr,
                                          C.byref(n_out), 0, 0, None, None)]
            for f in dev_calls:
                if want:
                    with pytest.raises(want):
                        f()
                else:
                    n_out.value = 7
                    f()
                    assert n_out.value == 0
        # a findmax window outside the lag vector
        with pytest.raises(IndexError):
            search_d(ctx, qin.ptr, 2, 1.0, n, 0.5, 1, out.ptr, 490, 20)
        A.check()   # nothing was written by any of them
