"""Coherent stacking across buffers -- the phase-coherent fold of a buffer kept COMPLEX, turned onto a complex y_t x x_t state and
blended into it, the magnitude taken once of the blended state -- through the entry points of include/tempest_hip_cstack.h.  Every
call of their symbols is here; api.Context.cstack / cstack_d / cstack_plan delegate to this module.  The loop a viewer runs on a weak
target: refine_period and refine_carrier once; per buffer F, t0_next, phi_next = cstack_plan(n, t0, T, kappa, phi) and
cstack_d(..., t0, T, kappa, phi, F, ..., alpha, mode, zstate, mag, info) with the carried t0 and phi.  mode "given" trusts the carried
phi; "lock" measures the turn between the buffer's picture and the state and survives a dropped buffer or a carrier phase step
(a retune by whole turns per frame also changes the phase along each frame: ctrack.py)."""
import ctypes as C
import math

import numpy as np

from ._lib import CSTACK_GIVEN, CSTACK_INFO, CSTACK_LOCK
from .fold import _host_iq, _iq_args, fold_plan

MODES = {"given": CSTACK_GIVEN, "lock": CSTACK_LOCK}


def mode_code(mode):
    """"given" / "lock" (or the TSDR_CSTACK_* integer) -> the integer; AssertionError for anything else"""
    if isinstance(mode, str) and mode in MODES:
        return MODES[mode]
    if isinstance(mode, (int, np.integer)) and not isinstance(mode, bool) and int(mode) in (CSTACK_GIVEN, CSTACK_LOCK):
        return int(mode)
    raise AssertionError(f"unknown stacking mode {mode!r} (given, lock)")


def cstack_plan(n, t0, T, kappa, phi, theta=0.0):
    """(F, next_t0, next_phi) of a buffer of n samples whose first whole frame starts at t0 with carrier phase phi (turns):
    F, next_t0 = fold_plan(n, t0, T); the frame that straddles the end is skipped but advances the carrier too, so
    next_phi = frac(phi + theta + (F + 1) * kappa) -- theta: a measured residual (info[4] of a call) to fold into the carried phase.
    (t0 >= n: no frame starts in this buffer, (0, t0 - n, phi).)"""
    F, nt0 = fold_plan(n, t0, T)
    if float(t0) >= float(n):
        return 0, nt0, float(phi)
    x = float(phi) + float(theta) + (F + 1) * float(kappa)
    return F, nt0, x - math.floor(x)


def cstack_d(ctx, iq, fmt, scale, n, t0, T, kappa, phi, n_frames, y_t, x_t, alpha, mode, zstate, mag=None, info=None):
    """device pointers: iq = n samples of format `fmt`; zstate (y_t * x_t complex64, column-major (y_t, x_t)) <- alpha * zstate +
    (1 - alpha) * conj(q) * Z, Z the mean of n_frames complex frames of period T from t0, frame f turned by -(phi + f * kappa) turns;
    q = 1 (mode "given") or the measured turn of Z against zstate ("lock"); alpha == 0: zstate is overwritten, not read.
    mag (y_t * x_t float32) <- |zstate|, info (8 float64) <- Re rho, Im rho, E_z, E_s, theta, gamma, q; either may be None.
    Enqueues on the context's stream and returns -- tsdr_cstack_iq_d"""
    from . import api
    code, sc, n = _iq_args(fmt, scale, n)
    ctx.call("tsdr_cstack_iq_d", api._ptr(iq), code, sc, n, C.c_double(t0), C.c_double(T), C.c_double(kappa), C.c_double(phi), int(n_frames),
             int(y_t), int(x_t), C.c_float(alpha), mode_code(mode), api._ptr(zstate), api._ptr(mag), api._ptr(info))


def cstack(ctx, iq, t0, T, kappa, phi, n_frames, y_t, x_t, alpha=0.0, mode="given", zstate=None, fmt="cf32", scale=1.0):
    """host arrays -> (zstate complex64 (y_t, x_t) Fortran-order, mag float32 (y_t, x_t) Fortran-order, info float64[8]): one
    stacking step of `iq` (complex64, or integer IQ of format `fmt`) onto `zstate` (left untouched; required when alpha != 0) --
    tsdr_cstack_iq"""
    from . import api
    a, code, n = _host_iq(iq, fmt)
    P = int(y_t) * int(x_t)
    if alpha != 0.0 and zstate is None:
        raise AssertionError("cstack: alpha != 0 needs a zstate")
    z = np.zeros(P, np.complex64) if zstate is None else np.asarray(zstate, np.complex64).reshape(-1, order="F").copy()
    if z.size != P:
        raise AssertionError(f"cstack: zstate has {z.size} pixels, expected {P}")
    mag = np.zeros(P, np.float32)
    info = np.zeros(CSTACK_INFO, np.float64)
    ctx.call("tsdr_cstack_iq", api._ptr(a), code, C.c_float(scale), n, C.c_double(t0), C.c_double(T), C.c_double(kappa), C.c_double(phi),
             int(n_frames), int(y_t), int(x_t), C.c_float(alpha), mode_code(mode), api._ptr(z), api._ptr(mag), api._ptr(info))
    shape = (int(y_t), int(x_t))
    return z.reshape(shape, order="F"), mag.reshape(shape, order="F"), info
