"""Coherent frame folding at a fractional frame period -- the mean of the frames a buffer holds when they are sampled at t0 + f*T,
IIR-averaged into a y_t x x_t state, and the period scan that scores the pictures folded at trial periods -- through the entry points
of include/tempest_hip_fold.h.  Every call of their symbols is here; api.Context.fold* / fold_scan* / refine_period delegate to this
module.  The loop a viewer runs: search -> refine_period once; per buffer F, t0_next = fold_plan(n, t0, T) and fold_d(..., t0, T, F, ...)
with the carried t0; once, downgrade + vsync on the folded picture for the origin; display_u8_d."""
import ctypes as C
import math

import numpy as np


def fold_plan(n, t0, T):
    """(F, next_t0) of a buffer of n samples whose first whole frame starts at t0: F = floor((n - t0) / T) frames fit; the frame
    that straddles the end is skipped and the phase kept, next_t0 = t0 + (F + 1) * T - n in (0, T] -- all in f64.  (t0 >= n: no frame
    starts in this buffer, (0, t0 - n).)"""
    n, t0, T = float(n), float(t0), float(T)
    if not (T > 0.0 and t0 >= 0.0 and math.isfinite(T) and math.isfinite(t0)):
        raise AssertionError(f"fold_plan: T must be positive and t0 not negative (got {T}, {t0})")
    if t0 >= n:
        return 0, t0 - n
    F = max(int(math.floor((n - t0) / T)), 0)
    while F > 0 and t0 + F * T > n:      # the quotient's rounding must not promise a frame the buffer does not hold
        F -= 1
    while t0 + (F + 1) * T <= n:
        F += 1
    return F, t0 + (F + 1) * T - n


def _iq_args(fmt, scale, n):
    from . import api
    return api.iq_fmt_code(fmt), C.c_float(scale), int(n)


def fold_d(ctx, iq, fmt, scale, n, t0, T, n_frames, y_t, x_t, alpha, state):
    """device pointers: iq = n samples of format `fmt`; state (y_t * x_t float32, column-major (y_t, x_t)) <- alpha * state +
    (1 - alpha) * the mean of n_frames frames of period T starting at t0 (alpha == 0: state is overwritten, not read).  Enqueues on
    the context's stream and returns -- tsdr_fold_iq_d"""
    from . import api
    code, sc, n = _iq_args(fmt, scale, n)
    ctx.call("tsdr_fold_iq_d", api._ptr(iq), code, sc, n, C.c_double(t0), C.c_double(T), int(n_frames), int(y_t), int(x_t), C.c_float(alpha),
             api._ptr(state))


def _host_iq(iq, fmt):
    """(contiguous array, TSDR_IQ_* code, samples) of a host buffer: complex64 for "cf32", else the format's integer dtype"""
    from . import api
    code = api.iq_fmt_code(fmt)
    if code == 0:
        a = api._c64(iq)
        return a, code, a.size
    return api._int_iq(iq, fmt, "fold")


def _host_state(who, state, alpha, y_t, x_t):
    """the y_t * x_t float32 vector a host fold works on: a column-major copy of `state` (required when alpha != 0), else zeros"""
    if alpha != 0.0 and state is None:
        raise AssertionError(f"{who}: alpha != 0 needs a state")
    out = np.zeros(int(y_t) * int(x_t), np.float32) if state is None else np.asarray(state, np.float32).reshape(-1, order="F").copy()
    if out.size != int(y_t) * int(x_t):
        raise AssertionError(f"{who}: state has {out.size} pixels, expected {int(y_t) * int(x_t)}")
    return out


def fold(ctx, iq, t0, T, n_frames, y_t, x_t, alpha=0.0, state=None, fmt="cf32", scale=1.0):
    """host arrays -> the (y_t, x_t) Fortran-order float32 picture: the fold of `iq` (complex64, or integer IQ of format `fmt`),
    averaged into `state` (left untouched; required when alpha != 0) -- tsdr_fold_iq"""
    from . import api
    a, code, n = _host_iq(iq, fmt)
    out = _host_state("fold", state, alpha, y_t, x_t)
    ctx.call("tsdr_fold_iq", api._ptr(a), code, C.c_float(scale), n, C.c_double(t0), C.c_double(T), int(n_frames), int(y_t), int(x_t),
             C.c_float(alpha), api._ptr(out))
    return out.reshape((int(y_t), int(x_t)), order="F")


def fold_scan_d(ctx, iq, fmt, scale, n, t0, T0, dT, n_trials, n_frames, y_t, x_t, score):
    """device pointers: score[k] (float64) <- the variance times y_t * x_t of the picture folded at T0 + k * dT, k < n_trials.
    Enqueues and returns -- tsdr_fold_scan_iq_d"""
    from . import api
    code, sc, n = _iq_args(fmt, scale, n)
    ctx.call("tsdr_fold_scan_iq_d", api._ptr(iq), code, sc, n, C.c_double(t0), C.c_double(T0), C.c_double(dT), int(n_trials), int(n_frames),
             int(y_t), int(x_t), api._ptr(score))


def fold_scan(ctx, iq, t0, T0, dT, n_trials, n_frames, y_t, x_t, fmt="cf32", scale=1.0):
    """host arrays -> (scores float64[n_trials], best): best = the first maximum, -1 when every score is NaN -- tsdr_fold_scan_iq"""
    from . import api
    a, code, n = _host_iq(iq, fmt)
    score = np.zeros(max(int(n_trials), 1), np.float64)
    best = C.c_int(-1)
    ctx.call("tsdr_fold_scan_iq", api._ptr(a), code, C.c_float(scale), n, C.c_double(t0), C.c_double(T0), C.c_double(dT), int(n_trials),
             int(n_frames), int(y_t), int(x_t), api._ptr(score), C.byref(best))
    return score[:int(n_trials)], best.value


def first_max(scores):
    """index of the first maximum; a NaN never wins; -1 when every score is NaN"""
    best = -1
    for k, s in enumerate(scores):
        if s == s and (best < 0 or s > scores[best]):
            best = k
    return best


def refine_period(ctx, iq_d, fmt, scale, n, T_guess, n_frames, y_t, x_t, dT=0.125, half=8, levels=2, shrink=4, t0=0.0):
    """The frame period to a fraction of a sample, from a guess good to half a sample (the autocorrelation peak's lag): a scan of
    2 * half + 1 trials spaced dT around the guess, recentred on the first maximum, `levels` times with dT /= shrink per level.
    iq_d: device pointer to n samples of format `fmt`; n_frames frames must fit at the largest trial.  Synchronises once per level.
    -> (T_hat, last_dT, scores): scores = one float64 array per level"""
    nt = 2 * int(half) + 1
    T_hat, step, last, scores = float(T_guess), float(dT), float(dT), []
    d_score = ctx.dev_alloc(nt * 8)
    try:
        for _ in range(int(levels)):
            T0 = T_hat - half * step
            fold_scan_d(ctx, iq_d, fmt, scale, n, t0, T0, step, nt, n_frames, y_t, x_t, d_score)
            ctx.synchronize()
            s = ctx.download(d_score, (nt,), np.float64)
            scores.append(s)
            b = first_max(s)
            if b < 0:
                raise AssertionError("refine_period: every score is NaN")
            T_hat, last, step = T0 + b * step, step, step / shrink
    finally:
        ctx.dev_free(d_score)
    return T_hat, last, scores
