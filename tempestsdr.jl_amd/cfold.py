"""Phase-coherent frame folding with carrier de-rotation -- the frames a buffer holds, sampled at t0 + f*T as complex samples, frame f
turned by -f*kappa turns, summed, the magnitude taken once and IIR-averaged into a y_t x x_t state; and the carrier scan that scores the
energy of the pictures folded at trial kappas -- through the entry points of include/tempest_hip_cfold.h.  Every call of their
symbols is here; api.Context.cfold* / cfold_scan* / refine_carrier delegate to this module.  The loop a viewer runs at low SNR:
refine_period (or the joint search of INTEGRATION.md) -> refine_carrier once; per buffer F, t0_next = fold_plan(n, t0, T) and
cfold_d(..., t0, T, kappa, F, ...) with the carried t0."""
import ctypes as C

import numpy as np

from .fold import _host_iq, _host_state, _iq_args, first_max


def cfold_d(ctx, iq, fmt, scale, n, t0, T, kappa, n_frames, y_t, x_t, alpha, state):
    """device pointers: iq = n samples of format `fmt`; state (y_t * x_t float32, column-major (y_t, x_t)) <- alpha * state +
    (1 - alpha) * |the mean of n_frames complex frames of period T starting at t0, frame f turned by -f * kappa turns| (alpha == 0:
    state is overwritten, not read).  Enqueues on the context's stream and returns -- tsdr_cfold_iq_d"""
    from . import api
    code, sc, n = _iq_args(fmt, scale, n)
    ctx.call("tsdr_cfold_iq_d", api._ptr(iq), code, sc, n, C.c_double(t0), C.c_double(T), C.c_double(kappa), int(n_frames), int(y_t),
             int(x_t), C.c_float(alpha), api._ptr(state))


def cfold(ctx, iq, t0, T, kappa, n_frames, y_t, x_t, alpha=0.0, state=None, fmt="cf32", scale=1.0):
    """host arrays -> the (y_t, x_t) Fortran-order float32 picture: the coherent fold of `iq` (complex64, or integer IQ of format
    `fmt`), averaged into `state` (left untouched; required when alpha != 0) -- tsdr_cfold_iq"""
    from . import api
    a, code, n = _host_iq(iq, fmt)
    out = _host_state("cfold", state, alpha, y_t, x_t)
    ctx.call("tsdr_cfold_iq", api._ptr(a), code, C.c_float(scale), n, C.c_double(t0), C.c_double(T), C.c_double(kappa), int(n_frames),
             int(y_t), int(x_t), C.c_float(alpha), api._ptr(out))
    return out.reshape((int(y_t), int(x_t)), order="F")


def cfold_scan_d(ctx, iq, fmt, scale, n, t0, T, kappa0, dkappa, n_trials, n_frames, y_t, x_t, score):
    """device pointers: score[k] (float64) <- the energy of the complex picture folded at kappa0 + k * dkappa, k < n_trials, all at
    the one period T.  Enqueues and returns -- tsdr_cfold_scan_iq_d"""
    from . import api
    code, sc, n = _iq_args(fmt, scale, n)
    ctx.call("tsdr_cfold_scan_iq_d", api._ptr(iq), code, sc, n, C.c_double(t0), C.c_double(T), C.c_double(kappa0), C.c_double(dkappa),
             int(n_trials), int(n_frames), int(y_t), int(x_t), api._ptr(score))


def cfold_scan(ctx, iq, t0, T, kappa0, dkappa, n_trials, n_frames, y_t, x_t, fmt="cf32", scale=1.0):
    """host arrays -> (scores float64[n_trials], best): best = the first maximum, -1 when every score is NaN -- tsdr_cfold_scan_iq"""
    from . import api
    a, code, n = _host_iq(iq, fmt)
    score = np.zeros(max(int(n_trials), 1), np.float64)
    best = C.c_int(-1)
    ctx.call("tsdr_cfold_scan_iq", api._ptr(a), code, C.c_float(scale), n, C.c_double(t0), C.c_double(T), C.c_double(kappa0),
             C.c_double(dkappa), int(n_trials), int(n_frames), int(y_t), int(x_t), api._ptr(score), C.byref(best))
    return score[:int(n_trials)], best.value


def refine_carrier(ctx, iq_d, fmt, scale, n, t0, T, n_frames, y_t, x_t, oversample=4, half=8, levels=2, shrink=4):
    """The carrier's advance per frame, kappa = frac(nu * T) turns, from nothing: level 0 scans oversample * n_frames trials over
    [0, 1) at dkappa = 1 / (oversample * n_frames) (the periodogram's own resolution is 1 / n_frames); each further level scans
    2 * half + 1 trials around the first maximum at dkappa / shrink.  iq_d: device pointer to n samples of format `fmt`.
    Synchronises once per level.  -> (kappa_hat mod 1, last_dkappa, scores): scores = one float64 array per level"""
    F = int(n_frames)
    if F < 1 or int(oversample) < 1 or int(levels) < 1:
        raise AssertionError("refine_carrier: n_frames, oversample and levels must be positive")
    nt0, nt = int(oversample) * F, 2 * int(half) + 1
    step = 1.0 / nt0
    kappa0, count, last, scores = 0.0, nt0, step, []
    d_score = ctx.dev_alloc(max(nt0, nt) * 8)
    try:
        for _ in range(int(levels)):
            cfold_scan_d(ctx, iq_d, fmt, scale, n, t0, T, kappa0, step, count, F, y_t, x_t, d_score)
            ctx.synchronize()
            s = ctx.download(d_score, (count,), np.float64)
            scores.append(s)
            b = first_max(s)
            if b < 0:
                raise AssertionError("refine_carrier: every score is NaN")
            kappa_hat, last = kappa0 + b * step, step
            step = step / shrink
            kappa0, count = kappa_hat - half * step, nt
    finally:
        ctx.dev_free(d_score)
    return kappa_hat % 1.0, last, scores
