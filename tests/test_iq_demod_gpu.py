"""GPU tests of the demodulators on integer IQ (tsdr_am_demod_iq_d, tsdr_abs2_iq_d, tsdr_invert_am_iq_d, tsdr_fm_demod_iq_d) and of
the public expansion tsdr_iq_expand_d.  Bit-identity, no tolerance: every output equals what the ComplexF32 `_d` entry point
writes for the same samples expanded on the host (tests/iq8_ref.py) -- invert_am's device-reduced maximum included --, on the
16-byte vector kernels and on the one-sample-per-lane ones that every other pair of pointers takes."""
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
KINDS = {"am": "tsdr_am_demod", "abs2": "tsdr_abs2", "invert_am": "tsdr_invert_am", "fm": "tsdr_fm_demod"}
IQ_D = {"am": lambda c, *a: c.lib.tsdr_am_demod_iq_d(c.h, *a), "abs2": lambda c, *a: c.lib.tsdr_abs2_iq_d(c.h, *a),
        "invert_am": lambda c, *a: c.lib.tsdr_invert_am_iq_d(c.h, *a), "fm": lambda c, *a: c.lib.tsdr_fm_demod_iq_d(c.h, *a),
        "expand": lambda c, *a: c.lib.tsdr_iq_expand_d(c.h, *a)}
TWIN_D = {"am": lambda c, *a: c.lib.tsdr_am_demod_d(c.h, *a), "abs2": lambda c, *a: c.lib.tsdr_abs2_d(c.h, *a),
          "invert_am": lambda c, *a: c.lib.tsdr_invert_am_d(c.h, *a), "fm": lambda c, *a: c.lib.tsdr_fm_demod_d(c.h, *a)}
SIZES = [1, 63, 1000, 4099]    # below one vector; vector body + tail (4099 = 1024 x 4 + 3 = 512 x 8 + 3)


@functools.lru_cache(maxsize=None)
def _capture(fmt, n, peak_at=None):
    """seeded noise at a tenth of full scale as integer components; peak_at: that sample alone at full scale (the maximum)"""
    rng = np.random.default_rng(777 + n)
    z = (0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    z = np.clip(z.real, -0.45, 0.45) + 1j * np.clip(z.imag, -0.45, 0.45)
    z = z.astype(np.complex64)
    ref = np.concatenate([z, np.array([1.0 + 1.0j], np.complex64)])    # fixes the scale: full scale = 1.0
    q, scale = R.quantise(ref, fmt)
    q = q[:2 * n].copy()
    if peak_at is not None:
        q[2 * peak_at: 2 * peak_at + 2] = R.quantise(np.array([1.0 + 1.0j], np.complex64), fmt)[0]
    cf = R.expand(q, fmt, scale)
    q.setflags(write=False)
    cf.setflags(write=False)
    return q, float(scale), cf


_TWIN = {}


def _twin(ctx, kind, fmt, n, peak_at=None):
    key = (kind, fmt, n, peak_at)
    if key not in _TWIN:
        _, _, cf = _capture(fmt, n, peak_at)
        d_in, d_out = ctx.upload(cf.view(np.float32)), ctx.dev_alloc(4 * n)
        try:
            assert TWIN_D[kind](ctx, C.c_void_p(d_in), n, C.c_void_p(d_out)) == 0
            ctx.synchronize()
            got = ctx.download(d_out, (n,), np.uint32)
        finally:
            ctx.dev_free(d_in)
            ctx.dev_free(d_out)
        got.setflags(write=False)
        _TWIN[key] = got
    return _TWIN[key]


def _raw_buffer(q, k, fill=55):
    buf = np.concatenate([np.full(2 * k, fill, q.dtype), q])
    if buf.nbytes % 4:
        buf = np.concatenate([buf, np.full(2, fill, q.dtype)])
    return buf


def _iq(ctx, kind, fmt, n, k=0, out_floats=0, peak_at=None):
    """the `_iq_d` entry point on base + k samples, output at base + out_floats floats, both in guarded arenas"""
    api = importlib.import_module("tempestsdr_jl_amd.api")
    q, scale, _ = _capture(fmt, n, peak_at)
    with D.Arenas(ctx) as A:
        x = A.input("iq", _raw_buffer(q, k), 0)
        y = A.output("out", 4 * n, 4 * out_floats)
        api.demod_iq_d(kind, ctx, x.addr + k * R.BYTES[fmt], fmt, scale, n, y.addr)
        A.check()
        return y.get(np.uint32)


def _alive(kind, bits):
    if bits.size > 1 or kind in ("am", "abs2"):    # (fmDemod's first output is 0, and so is invert_amDemod of one sample)
        assert np.any(bits), "the output is all zero"
    if bits.size > 2:
        assert np.any(bits[1:] != bits[1]), "the output is all one value"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", SIZES)
def test_demod_equals_cf32_twin(ctx, kind, fmt, n):
    want = _twin(ctx, kind, fmt, n)
    for k, of in ((0, 0), (1, 0), (3, 0), (0, 1), (0, 3), (1, 3), (3, 1)):    # (0, 0): the 16-byte vector kernels
        got = _iq(ctx, kind, fmt, n, k=k, out_floats=of)
        assert np.array_equal(got, want), (kind, fmt, n, k, of)
    _alive(kind, want)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("where", ["first", "last", "tail"])
def test_invert_am_maximum_position(ctx, fmt, where):
    """the device-reduced maximum, wherever it sits: first sample, last sample, the tail behind the vector body"""
    n = 4099
    peak = {"first": 0, "last": n - 1, "tail": n - 3}[where]
    want = _twin(ctx, "invert_am", fmt, n, peak)
    assert want.view(np.float32)[peak] == 0.0 and np.count_nonzero(want.view(np.float32) == 0.0) == 1    # 1 - max / max, there alone
    for k, of in ((0, 0), (1, 0), (0, 1)):
        assert np.array_equal(_iq(ctx, "invert_am", fmt, n, k=k, out_floats=of, peak_at=peak), want), (fmt, where, k, of)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_no_samples_is_what_the_twin_returns(ctx, kind, fmt):
    q, scale, cf = _capture(fmt, 8)
    d_in, d_cf, d_out = ctx.upload(q), ctx.upload(cf.view(np.float32)), ctx.dev_alloc(64)
    try:
        rc_twin = TWIN_D[kind](ctx, C.c_void_p(d_cf), 0, C.c_void_p(d_out))
        rc = IQ_D[kind](ctx, C.c_void_p(d_in), R.CODES[fmt], C.c_float(scale), 0, C.c_void_p(d_out))
        assert rc == rc_twin == (-1 if kind == "invert_am" else 0)
    finally:
        for p in (d_in, d_cf, d_out):
            ctx.dev_free(p)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n", SIZES)
def test_expand_equals_host_expansion(ctx, fmt, n):
    api = importlib.import_module("tempestsdr_jl_amd.api")
    q, scale, cf = _capture(fmt, n)
    want = cf.view(np.uint32)
    for k, oc in ((0, 0), (1, 0), (3, 0), (0, 1), (1, 3)):    # input at base + k samples, output at base + oc ComplexF32
        with D.Arenas(ctx) as A:
            x = A.input("iq", _raw_buffer(q, k), 0)
            y = A.output("cf32_out", 8 * n, 8 * oc)
            api.expand_iq_d(ctx, x.addr + k * R.BYTES[fmt], fmt, scale, n, y.addr)
            A.check()
            assert np.array_equal(y.get(np.uint32), want), (fmt, n, k, oc)
    assert np.any(want)


@pytest.mark.parametrize("kind", list(KINDS) + ["expand"])
def test_bad_arguments_are_einval(ctx, kind):
    q, scale, _ = _capture("sc8", 64)
    out_name = "cf32_out" if kind == "expand" else "out"
    for code, in_shift, out_shift, arg in ((-1, 0, 0, "iq_fmt"), (4, 0, 0, "iq_fmt"), (R.CODES["sc8"], 1, 0, "iq"), (R.CODES["sc16"], 2, 0, "iq"),
                                           (R.CODES["sc8"], 0, 2, out_name)):
        with D.Arenas(ctx) as A:
            x = A.input("iq", q, 0)
            y = A.output("out", 8 * 64 + 8, 0)
            rc = IQ_D[kind](ctx, C.c_void_p(x.addr + in_shift), code, C.c_float(scale), 32, C.c_void_p(y.addr + out_shift))
            err = ctx.lib.tsdr_last_error(ctx.h).decode()
            assert rc == -1 and re.search(rf"\b{arg}\b", err), (kind, code, in_shift, out_shift, err)
            A.check()
            assert np.array_equal(y.get(np.uint32), D.image(y.lead, y.payload)[y.lead // 4: (y.lead + y.payload) // 4]), "output written"
