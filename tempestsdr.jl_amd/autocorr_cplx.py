"""calculate_autocorrelation (Autocorrelations.jl:23-37) of COMPLEX input -- the coherent autocorrelation of the IQ samples
themselves, no abs2 before the correlation -- through the entry points of include/tempest_hip_cplx.h.  Every call of their `_d`
symbols is here; api.Context.calculate_autocorrelation (complex input), Context.autocorr_search_complex and
search.extract_configuration(domain="complex") delegate to this module."""
import ctypes as C

import numpy as np


def _window(Fs, minDelay, maxDelay):
    index_min = 1 + int(np.round(minDelay * Fs))
    index_max = int(np.round(maxDelay * Fs))
    return index_min, index_max, max(index_max - index_min + 1, 0)


def _lags(Fs, index_min, index_max):
    return np.arange(0, index_max - index_min + 1, dtype=np.float64) * (1.0 / Fs)


def calculate(ctx, x, Fs, minDelay, maxDelay, scale="log", *, dtype=None, iq_fmt=None, iq_scale=1.0):
    """-> (G, lags) like Context.calculate_autocorrelation, host arrays in and out.
    x: complex64 (tsdr_autocorr_cplx); complex128 with dtype=np.float64 (tsdr_autocorr_cplx_f64, Float64 out) -- any other
    complex / dtype mix is an AssertionError, the MethodError analogue; or, with iq_fmt "sc16" / "sc8" / "uc8", an int16 / int8 /
    uint8 array of 2*n interleaved components (strict about the dtype), uploaded as it is (tsdr_autocorr_cplx_iq)."""
    from . import api   # at call time: api.py imports this module
    log = 1 if scale == "log" else 0
    index_min, index_max, cnt = _window(Fs, minDelay, maxDelay)
    n_out = C.c_size_t(0)
    tail = (float(Fs), float(minDelay), float(maxDelay), log)
    if iq_fmt is not None:
        if dtype is not None:
            raise AssertionError("calculate_autocorrelation: iq_fmt is a Float32 path (dtype must be None)")
        a, code, n = api._int_iq(x, iq_fmt, "calculate_autocorrelation")
        out = np.empty(max(cnt, 1), np.float32)
        ctx.call("tsdr_autocorr_cplx_iq", api._ptr(a), code, C.c_float(iq_scale), n, *tail, api._ptr(out), C.byref(n_out))
    elif api._is64(dtype):
        a = api._c128(x, "calculate_autocorrelation")
        out = np.empty(max(cnt, 1), np.float64)
        ctx.call("tsdr_autocorr_cplx_f64", api._ptr(a), a.size, *tail, api._ptr(out), C.byref(n_out))
    else:
        a = np.ascontiguousarray(api._need(x, np.complex64, "calculate_autocorrelation"))
        out = np.empty(max(cnt, 1), np.float32)
        ctx.call("tsdr_autocorr_cplx", api._ptr(a), a.size, *tail, api._ptr(out), C.byref(n_out))
    return out[: n_out.value], _lags(Fs, index_min, index_max)


def autocorr_cplx_d(ctx, z, n, Fs, minDelay, maxDelay, log_scale, out, *, f64=False):
    """device pointers: the lags of n ComplexF32 (f64: ComplexF64) samples at z -> out (float32 / float64 on the device); returns
    the number of lags written.  Enqueues on the context's stream and returns -- tsdr_autocorr_cplx_d / tsdr_autocorr_cplx_f64_d"""
    from . import api
    n_out = C.c_size_t(0)
    ctx.call("tsdr_autocorr_cplx_f64_d" if f64 else "tsdr_autocorr_cplx_d", api._ptr(z), int(n), float(Fs), float(minDelay),
             float(maxDelay), int(bool(log_scale)), api._ptr(out), C.byref(n_out))
    return n_out.value


def search_iq_d(ctx, iq, fmt, scale, n, Fs, minDelay, maxDelay, log_scale, out, win_lo=0, win_cnt=0):
    """device pointers: the lags of n samples of `fmt` ("cf32", "sc16", "sc8", "uc8": a raw StagingRing slot, a tensor slice at any
    sample) -> out, and findmax over out[win_lo .. win_lo + win_cnt) -> (lags written, idx, val); win_cnt == 0 is the plain
    device call (idx, val = None) -- tsdr_autocorr_cplx_search_iq_d"""
    from . import api
    n_out, idx, val = C.c_size_t(0), C.c_size_t(0), C.c_float(0)
    ctx.call("tsdr_autocorr_cplx_search_iq_d", api._ptr(iq), api.iq_fmt_code(fmt), C.c_float(scale), int(n), float(Fs), float(minDelay),
             float(maxDelay), int(bool(log_scale)), api._ptr(out), C.byref(n_out), int(win_lo), int(win_cnt), C.byref(idx), C.byref(val))
    if not win_cnt:
        return n_out.value, None, None
    return n_out.value, int(idx.value), float(val.value)


def search(ctx, sig, Fs, minDelay, maxDelay, rate_min=50, rate_max=90, scale="log", *, iq_fmt=None, iq_scale=1.0, n_samples=None):
    """calculate_autocorrelation of the complex samples + zoom_autocorr + findmax as ONE library call (GUI.jl:73-81 on the raw IQ).
    sig: a complex array (ComplexF32), or with iq_fmt "sc16" / "sc8" / "uc8" an integer array of 2*n interleaved components, or
    the integer address of a device buffer of iq_fmt samples ("cf32" allowed there) with n_samples = n.
    -> (G, pos, val): the lag vector, the 0-based findmax position inside the zoom window, its value."""
    from . import api
    d_in, own = None, True
    if isinstance(sig, (int, np.integer)) and not isinstance(sig, bool):
        if iq_fmt is None or n_samples is None or int(n_samples) <= 0:
            raise AssertionError("a device address needs iq_fmt and n_samples")
        d_in, own, n, code = int(sig), False, int(n_samples), api.iq_fmt_code(iq_fmt)
    elif iq_fmt is None:
        a = np.ascontiguousarray(sig)
        if not np.iscomplexobj(a):
            raise AssertionError("autocorr_search_complex: expected a complex vector (real samples: autocorr_search)")
        a, code = a.astype(np.complex64, copy=False), 0
        n = a.size
    else:
        a, code, n = api._int_iq(sig, iq_fmt, "autocorr_search_complex")
    _, _, cnt = _window(Fs, minDelay, maxDelay)
    pmin, pmax = C.c_size_t(0), C.c_size_t(0)
    api.check(ctx.h, ctx.lib.tsdr_zoom_bounds(cnt, float(Fs), float(rate_min), float(rate_max), C.byref(pmin), C.byref(pmax)),
              "tsdr_zoom_bounds")
    if d_in is None:
        d_in = ctx.upload(a)
    d_out = None
    try:
        d_out = ctx.dev_alloc(max(cnt, 1) * 4)
        n_out, idx, val = search_iq_d(ctx, d_in, code, iq_scale, n, Fs, minDelay, maxDelay, scale == "log", d_out,
                                      int(pmin.value - 1), int(pmax.value - pmin.value + 1))
        G = ctx.download(d_out, (n_out,), np.float32)
    finally:
        if own:
            ctx.dev_free(d_in)
        if d_out is not None:
            ctx.dev_free(d_out)
    return G, idx, val
