"""Device-pointer forms of GetSpectrum.jl's and Demodulation.jl's functions on integer IQ as the SDR stored it, and the staging
ring's expansion as a call: thin wrappers of the entry points of include/tempest_hip_iq.h.  api.py re-exports them
(api.spectrum_iq_d ...), next to frames_iq_d."""
import ctypes as C


def _head(iq, fmt, scale):
    """the `iq, iq_fmt, scale` arguments, and api._ptr for the outputs"""
    from . import api   # at call time: api.py imports this module
    return api._ptr, (api._ptr(iq), api.iq_fmt_code(fmt), C.c_float(scale))


# Device-pointer forms of the spectra and demodulators on a buffer of `fmt` samples ("cf32", "sc16", "sc8", "uc8" -- a raw
# StagingRing slot, a tensor slice at any sample): they enqueue on the context's stream and return without synchronising.
def spectrum_iq_d(ctx, iq, fmt, scale, N, lin, y):
    """getSpectrum of the first N samples -> y (N float32 on the device) -- tsdr_spectrum_iq_d"""
    ptr, head = _head(iq, fmt, scale)
    ctx.call("tsdr_spectrum_iq_d", *head, int(N), int(bool(lin)), ptr(y))


def welch_iq_d(ctx, iq, fmt, scale, n, sizeFFT, lin, y):
    """getWelch of n samples -> y (sizeFFT float32 on the device) -- tsdr_welch_iq_d"""
    ptr, head = _head(iq, fmt, scale)
    ctx.call("tsdr_welch_iq_d", *head, int(n), int(sizeFFT), int(bool(lin)), ptr(y))


def waterfall_iq_d(ctx, iq, fmt, scale, n, sizeFFT, sMatrix):
    """getWaterfall of n samples -> sMatrix (sizeFFT x n // sizeFFT float64, column-major, on the device) -- tsdr_waterfall_iq_d"""
    ptr, head = _head(iq, fmt, scale)
    ctx.call("tsdr_waterfall_iq_d", *head, int(n), int(sizeFFT), ptr(sMatrix))


DEMOD_IQ = {"am": "tsdr_am_demod_iq_d", "abs2": "tsdr_abs2_iq_d", "invert_am": "tsdr_invert_am_iq_d", "fm": "tsdr_fm_demod_iq_d"}


def demod_iq_d(kind, ctx, iq, fmt, scale, n, out):
    """kind "am" / "abs2" / "invert_am" / "fm": amDemod, abs2, invert_amDemod or fmDemod of n samples -> out (n float32)"""
    if kind not in DEMOD_IQ:
        raise AssertionError(f"unknown demodulator {kind!r} (am, abs2, invert_am, fm)")
    ptr, head = _head(iq, fmt, scale)
    ctx.call(DEMOD_IQ[kind], *head, int(n), ptr(out))


def expand_iq_d(ctx, iq, fmt, scale, n, cf32_out):
    """the staging ring's expansion as a call: n samples of `fmt` -> n ComplexF32 at cf32_out (8-byte aligned) -- tsdr_iq_expand_d"""
    ptr, head = _head(iq, fmt, scale)
    ctx.call("tsdr_iq_expand_d", *head, int(n), ptr(cf32_out))
