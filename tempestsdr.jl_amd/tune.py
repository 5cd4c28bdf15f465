"""The tuner -- frequency shift by a 64-bit phase accumulator, real FIR low-pass and decimation of an IQ stream, chained across calls
-- through the entry points of include/tempest_hip_tune.h.  Every call of their symbols is here; api.Context.tune / tune_d / tuner
delegate to this module.

A wideband capture holds the harmonic the user wants and much beside it.  The loop: getWelch / getWaterfall show where the leak is;
nu = freq_fix(-f_leak, Fs) brings it to DC; design_lowpass(L, D) rejects what lies beside it; a Tuner turns every buffer of the ring
into Fs / D ComplexF32 samples that every other entry point takes -- a fold at T / D with its origin moved by the filter's group
delay (tuned_t0)."""
import ctypes as C
import math

import numpy as np

from . import _lib
from .fold import _host_iq, _iq_args

TAPS_MAX, DECIM_MAX = _lib.TUNE_TAPS_MAX, _lib.TUNE_DECIM_MAX
_MASK = (1 << 64) - 1


def freq_fix(f_hz, Fs):
    """nu_fix (turns * 2^64 per sample, wrapped to uint64) of a shift BY f_hz at sample rate Fs: bringing a carrier at +f to DC needs
    freq_fix(-f, Fs).  Exact rational arithmetic on the two floats, rounded once to the nearest integer"""
    from fractions import Fraction
    if not (math.isfinite(f_hz) and math.isfinite(Fs) and Fs > 0.0):
        raise AssertionError(f"freq_fix: f_hz must be finite and Fs positive (got {f_hz}, {Fs})")
    turns = Fraction(float(f_hz)) / Fraction(float(Fs))
    return int(round(turns * (1 << 64))) & _MASK


def phase_fix(turns):
    """phi_fix of a start phase in turns"""
    from fractions import Fraction
    return int(round(Fraction(float(turns)) * (1 << 64))) & _MASK


def _window(name, L):
    k = np.arange(L, dtype=np.float64)
    if L == 1:
        return np.ones(1)
    x = 2.0 * np.pi * k / (L - 1)
    if name == "blackman":
        return 0.42 - 0.5 * np.cos(x) + 0.08 * np.cos(2.0 * x)
    if name == "hamming":
        return 0.54 - 0.46 * np.cos(x)
    if name == "hann":
        return 0.5 - 0.5 * np.cos(x)
    if name in ("rect", "boxcar"):
        return np.ones(L)
    raise AssertionError(f"design_lowpass: unknown window {name!r} (blackman, hamming, hann, rect)")


def design_lowpass(L, D, width=0.9, window="blackman"):
    """L real taps of a windowed sinc with cut-off width / (2 D) cycles per input sample (width = 1: the output's Nyquist frequency):
    sinc(width * (i - (L - 1) / 2) / D) * window, normalised to unit DC gain in f64, then rounded to f32.  Symmetric: the group delay
    is (L - 1) / 2 input samples"""
    L, D = int(L), int(D)
    if not (1 <= L <= TAPS_MAX and 1 <= D <= DECIM_MAX and 0.0 < float(width) <= 1.0):
        raise AssertionError(f"design_lowpass: 1 <= L <= {TAPS_MAX}, 1 <= D <= {DECIM_MAX}, 0 < width <= 1 (got {L}, {D}, {width})")
    i = np.arange(L, dtype=np.float64) - (L - 1) / 2.0
    h = np.sinc(float(width) * i / D) * _window(window, L)
    return (h / h.sum()).astype(np.float32)


def tune_plan(m0, n, L, D, j0, n_hist, Fs=None):
    """-> (n_out, next): the outputs a call with these arguments writes (include/tempest_hip_tune.h, 4.: j0 .. floor((m0 + n - L) / D))
    and the arguments of the call that follows it: next = {"m0", "j0", "n_hist"} carried forward, "decim" = D, "delay" = (L - 1) / 2
    input samples (the group delay of symmetric taps) and, when Fs is given, "Fs_out" = Fs / D.  AssertionError for what the library
    refuses: a window that starts before the history"""
    m0, n, L, D, j0, n_hist = int(m0), int(n), int(L), int(D), int(j0), int(n_hist)
    if not (1 <= L <= TAPS_MAX and 1 <= D <= DECIM_MAX and 0 <= n < (1 << 31) and 0 <= n_hist <= min(L - 1, m0) and m0 >= 0 and j0 >= 0):
        raise AssertionError(f"tune_plan: arguments out of range (m0 {m0}, n {n}, L {L}, D {D}, j0 {j0}, n_hist {n_hist})")
    if m0 + n > _MASK:
        raise AssertionError("tune_plan: m0 + n must be below 2^64")
    if j0 * D < m0 - n_hist:
        raise AssertionError(f"tune_plan: the window of j0 = {j0} starts at {j0 * D}, before the history ({m0} - {n_hist})")
    end = m0 + n
    n_out = max((end - L) // D - j0 + 1, 0) if end >= L else 0
    nxt = {"m0": end, "j0": j0 + n_out, "n_hist": min(L - 1, n_hist + n), "decim": D, "delay": (L - 1) / 2.0}
    if Fs is not None:
        nxt["Fs_out"] = float(Fs) / D
    return n_out, nxt


def tuned_t0(t_in, L, D):
    """where input position t_in (samples of the stream, absolute) lies in the tuned stream: (t_in - (L - 1) / 2) / D output samples
    -- frame f of period T begins at tuned_t0(f * T, L, D); fold the tuned stream at period T / D"""
    return (float(t_in) - (int(L) - 1) / 2.0) / int(D)


def tune_tile(L, D):
    """outputs per workgroup of the kernel for these L and D (tsdr_tune_tile)"""
    r = _lib.load().tsdr_tune_tile(int(L), int(D))
    if r <= 0:
        raise AssertionError(f"tune_tile: 1 <= L <= {TAPS_MAX}, 1 <= D <= {DECIM_MAX} (got {L}, {D})")
    return r


def tune_d(ctx, iq, fmt, scale, n, m0, nu_fix, phi_fix, taps, n_taps, decim, j0, hist, n_hist, out, out_cap):
    """device pointers: out[0 .. n_out) (ComplexF32) <- y[j0 ..] of the n samples of format `fmt` at iq (iq[0] = x[m0]); hist (L - 1
    ComplexF32, or None with n_hist == 0) carried forward.  Enqueues on the context's stream and returns n_out -- tsdr_tune_iq_d"""
    from . import api
    code, sc, n = _iq_args(fmt, scale, n)
    n_out = C.c_size_t(0)
    ctx.call("tsdr_tune_iq_d", api._ptr(iq), code, sc, n, int(m0) & _MASK, int(nu_fix) & _MASK, int(phi_fix) & _MASK, api._ptr(taps),
             int(n_taps), int(decim), int(j0), api._ptr(hist), int(n_hist), api._ptr(out), int(out_cap), C.byref(n_out))
    return n_out.value


def tune(ctx, iq, nu_fix, taps, decim, m0=0, phi_fix=0, j0=None, hist=None, n_hist=0, fmt="cf32", scale=1.0):
    """host arrays -> (y complex64[n_out], hist complex64[L - 1], next): one call of tsdr_tune_iq on `iq` (complex64, or integer IQ of
    format `fmt`).  j0 None: the first window that starts at or after m0 - n_hist.  hist / n_hist: what the previous call returned
    (next["n_hist"]); next: tune_plan's"""
    from . import api
    a, code, n = _host_iq(iq, fmt)
    h = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    L, D = h.size, int(decim)
    if j0 is None:
        j0 = -((-(int(m0) - int(n_hist))) // D)
    cap, nxt = tune_plan(m0, n, L, D, j0, n_hist)
    hs = np.zeros(max(L - 1, 1), np.complex64)
    if hist is not None:
        hs[:L - 1] = np.asarray(hist, np.complex64).reshape(-1)[:L - 1]
    out = np.zeros(max(cap, 1), np.complex64)
    n_out = C.c_size_t(0)
    ctx.call("tsdr_tune_iq", api._ptr(a if n else np.zeros(1, np.complex64)), code, C.c_float(scale), n, int(m0) & _MASK, int(nu_fix) & _MASK,
             int(phi_fix) & _MASK, api._ptr(h), L, D, int(j0), api._ptr(hs), int(n_hist), api._ptr(out), cap, C.byref(n_out))
    assert n_out.value == cap, (n_out.value, cap)
    return out[:cap], hs[:L - 1], nxt


class Tuner:
    """A tuner on the device for a ring's consumer: owns the device taps and the history, carries the plan from buffer to buffer.
        t = ctx.tuner(freq_fix(-f_leak, Fs), design_lowpass(63, 4), 4)
        n_out = t.push_d(d_iq, "sc16", scale, n, d_out)        # enqueues; d_out holds n_out ComplexF32 at Fs / 4
    m0 / j0 / n_hist: the next call's (tune_plan).  delay: (L - 1) / 2 input samples; close() frees the device memory."""

    def __init__(self, ctx, nu_fix, taps, decim, phi_fix=0, m0=0):
        h = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.ctx, self.L, self.D = ctx, int(h.size), int(decim)
        if not (1 <= self.L <= TAPS_MAX and 1 <= self.D <= DECIM_MAX):
            raise AssertionError(f"Tuner: 1 <= taps <= {TAPS_MAX}, 1 <= decim <= {DECIM_MAX} (got {self.L}, {self.D})")
        self.nu_fix, self.phi_fix = int(nu_fix) & _MASK, int(phi_fix) & _MASK
        self.taps = h
        self.d_taps = ctx.upload(h)
        self.d_hist = ctx.dev_alloc(8 * max(self.L - 1, 1))
        self.delay = (self.L - 1) / 2.0
        self.reset(m0)

    def reset(self, m0=0):
        """start a new stream at absolute sample m0 with no history"""
        self.m0, self.n_hist = int(m0), 0
        self.j0 = -((-self.m0) // self.D)

    def plan(self, n):
        """(n_out, next) of the next push of n samples"""
        return tune_plan(self.m0, n, self.L, self.D, self.j0, self.n_hist)

    def push_d(self, iq, fmt, scale, n, out, out_cap=None):
        """the next n samples of the stream (device pointer, format `fmt`) -> out (device pointer, room for out_cap ComplexF32; None:
        what plan(n) says).  Enqueues and returns n_out"""
        cap, nxt = self.plan(n)
        n_out = tune_d(self.ctx, iq, fmt, scale, n, self.m0, self.nu_fix, self.phi_fix, self.d_taps, self.L, self.D, self.j0, self.d_hist,
                       self.n_hist, out, cap if out_cap is None else out_cap)
        assert n_out == cap, (n_out, cap)
        self.m0, self.j0, self.n_hist = nxt["m0"], nxt["j0"], nxt["n_hist"]
        return n_out

    def close(self):
        if getattr(self, "d_taps", None):
            self.ctx.synchronize()
            self.ctx.dev_free(self.d_taps)
            self.ctx.dev_free(self.d_hist)
            self.d_taps = self.d_hist = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
