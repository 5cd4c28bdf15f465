"""GPU tests of getSpectrum / getWelch / getWaterfall on integer IQ (tsdr_spectrum_iq_d, tsdr_welch_iq_d, tsdr_waterfall_iq_d;
TSDR_IQ_SC16 / _SC8 / _UC8).  The samples go in as the SDR stored them and are converted by the transforms' own loaders.  The
bar is bit-identity, no tolerance anywhere: every output equals what the ComplexF32 `_d` entry point (is_complex = 1) writes for
the same samples expanded on the host with tests/iq8_ref.py's product -- on every transform route (the 1024-point
wavefront-per-segment kernel, the LDS segment transforms, the multi-pass engines, the expand-first lengths), at any sample offset
inside a larger buffer, and on a raw staging-ring slot."""
import ctypes as C
import functools
import importlib
import re

import numpy as np
import pytest

import dptr_util as D
import iq8_ref as R

pytestmark = pytest.mark.gpu

FMTS = ["sc16", "sc8", "uc8"]
EINVAL = -1


@functools.lru_cache(maxsize=None)
def _noise(n):
    """seeded noise over a few tones: every FFT bin carries power, none the same"""
    rng = np.random.default_rng(20250 + n % 97)
    t = np.arange(n, dtype=np.float64)
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    z += 3.0 * np.exp(2j * np.pi * 0.1234 * t) + 1.5 * np.exp(-2j * np.pi * 0.3111 * t)
    return z.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def _capture(fmt, n):
    """(integer components [2n], scale, the same samples expanded on the host [n complex64]) -- made once, never modified"""
    q, scale = R.quantise(_noise(n), fmt)
    cf = R.expand(q, fmt, scale)
    q.setflags(write=False)
    cf.setflags(write=False)
    return q, float(scale), cf


# the entry points under test and their ComplexF32 twins, called by name (status returned, nothing raised)
IQ_D = {"spectrum": lambda c, *a: c.lib.tsdr_spectrum_iq_d(c.h, *a), "welch": lambda c, *a: c.lib.tsdr_welch_iq_d(c.h, *a),
        "waterfall": lambda c, *a: c.lib.tsdr_waterfall_iq_d(c.h, *a)}
TWIN_D = {"spectrum": lambda c, *a: c.lib.tsdr_spectrum_d(c.h, *a), "welch": lambda c, *a: c.lib.tsdr_welch_d(c.h, *a),
          "waterfall": lambda c, *a: c.lib.tsdr_waterfall_d(c.h, *a)}


def _out_bytes(kind, n, size):
    return 4 * n if kind == "spectrum" else 4 * size if kind == "welch" else 8 * size * (n // size)


def _args(kind, n, size, lin):
    return (n, lin) if kind == "spectrum" else (n, size, lin) if kind == "welch" else (n, size)


_TWIN = {}


def _twin(ctx, kind, fmt, n, size=0, lin=0):
    """bits of the ComplexF32 `_d` entry point on the host-expanded samples; computed once per case and shared"""
    key = (kind, fmt, n, size, lin)
    if key not in _TWIN:
        _, _, cf = _capture(fmt, max(n, 1))
        nbytes = _out_bytes(kind, n, size)
        d_in = ctx.upload(cf[:max(n, 1)].view(np.float32))
        d_out = ctx.dev_alloc(max(nbytes, 8))
        try:
            assert TWIN_D[kind](ctx, C.c_void_p(d_in), 1, *_args(kind, n, size, lin), C.c_void_p(d_out)) == 0
            ctx.synchronize()
            got = ctx.download(d_out, (nbytes // (8 if kind == "waterfall" else 4),), np.uint64 if kind == "waterfall" else np.uint32)
        finally:
            ctx.dev_free(d_in)
            ctx.dev_free(d_out)
        got.setflags(write=False)
        _TWIN[key] = got
    return _TWIN[key]


def _raw_buffer(q, n, k, fill=77):
    """k samples of junk, then the n samples, padded to whole words: the call gets base + k samples"""
    buf = np.concatenate([np.full(2 * k, fill, q.dtype), q[:2 * n]])
    if buf.nbytes % 4:
        buf = np.concatenate([buf, np.full(2, fill, q.dtype)])
    return buf


def _iq(ctx, kind, fmt, n, size=0, lin=0, k=0, out_phase=0, code=None, in_byte_shift=0, out_byte_shift=0, expect=0):
    """The `_iq_d` entry point on the raw samples at base + k samples, every array in a guarded arena (tests/dptr_util.py): the
    guards around input and output are checked, the input must be unchanged.  The status must be `expect`.
    -> (output payload, whether the whole output arena still holds its sentinel, tsdr_last_error)"""
    q, scale, _ = _capture(fmt, max(n, 1))
    buf = _raw_buffer(q, n, k)
    nbytes = _out_bytes(kind, n, size)
    with D.Arenas(ctx) as A:
        x = A.input("iq", buf, 0)
        y = A.output("out", max(nbytes, 8) + (8 if out_byte_shift else 0), out_phase)
        rc = IQ_D[kind](ctx, C.c_void_p(x.addr + k * R.BYTES[fmt] + in_byte_shift), R.CODES[fmt] if code is None else code,
                        C.c_float(scale), *_args(kind, n, size, lin), C.c_void_p(y.addr + out_byte_shift))
        err = ctx.lib.tsdr_last_error(ctx.h).decode()
        assert rc == expect, (rc, err)
        A.check()
        pay = y.get(np.uint32)
        untouched = np.array_equal(pay, D.image(y.lead, y.payload)[y.lead // 4: (y.lead + y.payload) // 4])
        if kind == "waterfall":
            pay = pay.view(np.uint64)
    return pay[: nbytes // (8 if kind == "waterfall" else 4)], untouched, err


def _alive(bits, n_min=2):
    assert np.any(bits), "the output is all zero"
    if bits.size >= n_min:
        assert np.any(bits != bits[0]), "the output is all one value"


def _same(ctx, kind, fmt, n, size=0, lin=0, **kw):
    want = _twin(ctx, kind, fmt, n, size, lin)
    got, _, _ = _iq(ctx, kind, fmt, n, size, lin, **kw)
    assert got.dtype == want.dtype and np.array_equal(got, want), (kind, fmt, n, size, lin, kw)
    _alive(got)
    return got


def _nseg_big(ctx):
    return 12 * ctx.device_info()["cu_count"] + 28    # wavefronts walk several segments: the prefetch of segment s + 1 runs


# ---- Welch and waterfall ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("lin", [0, 1])
def test_welch_1024_one_segment_per_wavefront(ctx, fmt, lin):
    _same(ctx, "welch", fmt, 37 * 1024 + 500, 1024, lin)    # (the 500 leftover samples are dropped)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("lin", [0, 1])
def test_welch_1024_wavefronts_walk_segments(ctx, fmt, lin):
    _same(ctx, "welch", fmt, _nseg_big(ctx) * 1024, 1024, lin)


@pytest.mark.parametrize("fmt", FMTS)
def test_waterfall_1024_one_segment_per_wavefront(ctx, fmt):
    _same(ctx, "waterfall", fmt, 37 * 1024 + 500, 1024)


@pytest.mark.parametrize("fmt", FMTS)
def test_waterfall_1024_wavefronts_walk_segments(ctx, fmt):
    _same(ctx, "waterfall", fmt, _nseg_big(ctx) * 1024, 1024)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [64, 1000, 1536, 4096])
def test_lds_row_routes(ctx, fmt, size):
    n = 7 * size + 5
    _same(ctx, "welch", fmt, n, size, 0)
    _same(ctx, "welch", fmt, n, size, 1)
    _same(ctx, "waterfall", fmt, n, size)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [8192, 10000, 1031])    # two passes (2^13), two passes (mixed radix), prime: Bluestein
def test_generic_routes(ctx, fmt, size):
    n = 3 * size + 1
    _same(ctx, "welch", fmt, n, size, 0)
    _same(ctx, "welch", fmt, n, size, 1)
    _same(ctx, "waterfall", fmt, n, size)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [1024, 1000, 8192])
def test_fewer_samples_than_one_segment(ctx, fmt, size):
    """no segment: zeros / -Inf dB in y and an untouched sMatrix, as the ComplexF32 twin"""
    n = size - 1
    for lin in (0, 1):
        got, _, _ = _iq(ctx, "welch", fmt, n, size, lin)
        assert np.array_equal(got, _twin(ctx, "welch", fmt, n, size, lin))
        assert np.array_equal(got.view(np.float32), np.full(size, 0.0 if lin else -np.inf, np.float32))
    got, untouched, _ = _iq(ctx, "waterfall", fmt, n, size)
    assert got.size == 0 and untouched


# ---- spectrum --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("lin", [0, 1])
@pytest.mark.parametrize("N", [1, 1000, 1031, 4096, 65536, 80000])    # (80 000: production/investigate_data.jl:44)
def test_spectrum(ctx, fmt, lin, N):
    _same(ctx, "spectrum", fmt, N, 0, lin)


# ---- offsets inside a larger buffer ----------------------------------------------------------------------------------------------
ROUTES = [("welch", 37 * 1024 + 500, 1024), ("waterfall", 37 * 1024 + 500, 1024),      # wavefront per segment
          ("welch", 7 * 1000 + 5, 1000), ("waterfall", 7 * 1000 + 5, 1000),            # LDS rows (three-step kernel)
          ("welch", 7 * 1536 + 5, 1536), ("waterfall", 7 * 1536 + 5, 1536),            # LDS rows (generic stages) | batched passes
          ("welch", 7 * 64 + 5, 64), ("waterfall", 7 * 64 + 5, 64),                    # ... | one-pass rows (expanded first)
          ("welch", 3 * 8192 + 1, 8192), ("waterfall", 3 * 10000 + 1, 10000),          # batched multi-pass loaders
          ("welch", 3 * 1031 + 1, 1031),                                               # Bluestein (expanded first)
          ("spectrum", 4096, 0), ("spectrum", 80000, 0), ("spectrum", 1000, 0), ("spectrum", 1031, 0), ("spectrum", 1, 0)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: f"{r[0]}-{r[1]}-{r[2]}")
def test_input_at_a_sample_offset(ctx, fmt, route):
    """base + k samples (8-bit: byte offsets 2, 6, 14) gives the bits of k = 0, with the guards around input and output intact;
    the output sits at an odd float / an odd double of its arena"""
    kind, n, size = route
    base = _same(ctx, kind, fmt, n, size, 0)
    for k in (1, 3, 7):
        got, _, _ = _iq(ctx, kind, fmt, n, size, 0, k=k, out_phase=8 * k if kind == "waterfall" else 4 * k)
        assert np.array_equal(got, base), (route, fmt, k)


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def _named(err, arg):
    return re.search(rf"\b{arg}\b", err) is not None


@pytest.mark.parametrize("kind", ["spectrum", "welch", "waterfall"])
@pytest.mark.parametrize("code", [-1, 4])
def test_unknown_format_is_einval(ctx, kind, code):
    _, untouched, err = _iq(ctx, kind, "sc8", 4096, 1024, 0, code=code, expect=EINVAL)
    assert untouched and _named(err, "iq_fmt"), err


@pytest.mark.parametrize("kind", ["spectrum", "welch", "waterfall"])
@pytest.mark.parametrize("fmt", FMTS)
def test_pointer_at_half_a_sample_is_einval(ctx, kind, fmt):
    """an odd byte for the 8-bit formats, 2 mod 4 for sc16"""
    _, untouched, err = _iq(ctx, kind, fmt, 4096, 1024, 0, in_byte_shift=R.BYTES[fmt] // 2, expect=EINVAL)
    assert untouched and _named(err, "iq"), err


@pytest.mark.parametrize("kind,arg", [("spectrum", "y"), ("welch", "y"), ("waterfall", "sMatrix")])
def test_misaligned_output_is_einval(ctx, kind, arg):
    _, untouched, err = _iq(ctx, kind, "sc16", 4096, 1024, 0, out_byte_shift=2 if kind != "waterfall" else 4, expect=EINVAL)
    assert untouched and _named(err, arg), err


@pytest.mark.parametrize("kind,n,size", [("spectrum", 4096, 0), ("welch", 5 * 1024, 1024), ("waterfall", 5 * 1024, 1024),
                                         ("welch", 5 * 1000, 1000)])
def test_cf32_code_is_the_twin(ctx, kind, n, size):
    """TSDR_IQ_CF32: the `_d` entry point with is_complex = 1, the scale ignored"""
    _, _, cf = _capture("sc16", n)
    nbytes = _out_bytes(kind, n, size)
    want = _twin(ctx, kind, "sc16", n, size, 0)
    with D.Arenas(ctx) as A:
        x = A.input("iq", cf[:n].view(np.float32), 8)
        y = A.output("out", nbytes, 8)
        assert IQ_D[kind](ctx, x.ptr, R.CODES["cf32"], C.c_float(123.0), *_args(kind, n, size, 0), y.ptr) == 0
        A.check()
        got = y.get(want.dtype)
    assert np.array_equal(got, want)


# ---- a raw ring slot ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["sc8", "uc8", "sc16"])    # tsdr_ring_create fmt 4, 6, 2
def test_raw_ring_slot_to_welch(ctx, tsdr, fmt):
    api = importlib.import_module("tempestsdr_jl_amd.api")
    n = 8192
    q, scale, _ = _capture(fmt, n)
    ring = tsdr.StagingRing(ctx, n, depth=2, fmt=fmt + "raw", scale=scale)
    d_y = ctx.dev_alloc(4 * 1024)
    try:
        assert ring.iq_fmt == fmt
        ring.put(q[:2 * n])
        slot = ring.take_d(timeout_ms=10000)
        api.welch_iq_d(ctx, slot, ring.iq_fmt, ring.scale, n, 1024, False, d_y)
        ctx.synchronize()
        got = ctx.download(d_y, (1024,), np.uint32)
    finally:
        ring.close()
        ctx.dev_free(d_y)
    assert np.array_equal(got, _twin(ctx, "welch", fmt, n, 1024, 0))
    _alive(got)


# ---- host-pointer forms and the Context keywords -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_context_keywords_upload_raw_samples(ctx, fmt):
    """Context.getSpectrum / getWelch / getWaterfall / amDemod / invert_amDemod / fmDemod / abs2 with iq_fmt= (tsdr_*_iq host forms and
    the demodulators' device forms behind an upload of the raw bytes) equal the same calls on the expanded samples"""
    n = 5 * 1024 + 3
    q, scale, cf = _capture(fmt, n)
    kw = dict(iq_fmt=fmt, iq_scale=scale)
    f0, y0 = ctx.getSpectrum(2.0e6, cf, N=4096)
    f1, y1 = ctx.getSpectrum(2.0e6, q, N=4096, **kw)
    assert np.array_equal(f0, f1) and np.array_equal(y0.view(np.uint32), y1.view(np.uint32))
    for size in (1024, 1000):
        f0, y0 = ctx.getWelch(2.0e6, cf, sizeFFT=size)
        f1, y1 = ctx.getWelch(2.0e6, q, sizeFFT=size, **kw)
        assert np.array_equal(f0, f1) and np.array_equal(y0.view(np.uint32), y1.view(np.uint32)), size
        t0, f0, m0 = ctx.getWaterfall(2.0e6, cf, sizeFFT=size)
        t1, f1, m1 = ctx.getWaterfall(2.0e6, q, sizeFFT=size, **kw)
        assert np.array_equal(t0, t1) and np.array_equal(f0, f1) and m1.shape == m0.shape == (size, n // size)
        assert np.array_equal(m0.view(np.uint64), m1.view(np.uint64)), size
        _alive(m1.view(np.uint64).ravel())
    for name in ("amDemod", "invert_amDemod", "fmDemod", "abs2"):
        a, b = getattr(ctx, name)(cf), getattr(ctx, name)(q, **kw)
        assert b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    with pytest.raises(AssertionError):
        ctx.getWelch(2.0e6, q.view(np.uint8) if fmt != "uc8" else q.view(np.int8), **kw)    # strict about the dtype
    with pytest.raises(IndexError):
        ctx.getSpectrum(2.0e6, q, N=n + 1, **kw)
