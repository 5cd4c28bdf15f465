"""Carrier tracking -- the weight of a sample as a function of frame and raster line, given as data -- through the entry points of
include/tempest_hip_ctrack.h.  Every call of their symbols is here; api.Context.ctrack_* / constant_track / fit_track / refine_track
delegate to this module.

A track is a float64 array of shape (F, 2): (a_f, b_f) in turns, the phase of frame f at its start and its advance over the frame.
ctrack_stack is coherent stacking (cstack.py) along a track; ctrack_probe measures every frame's phase against a picture.  The loop
that repairs a carrier drifting inside a buffer: refine_track = a constant-kappa stack, then probe against it, fit_track (a weighted
polynomial through the frames' phases), stack along the fitted track, twice.  The retune between buffers: constant_track with a
slope, F, kappa + slope whole turns per frame."""
import ctypes as C
import math

import numpy as np

from ._lib import CSTACK_INFO
from .cstack import mode_code
from .fold import _host_iq, _iq_args


def as_track(track, n_frames):
    """the (F, 2) float64 C-order array the library reads as 2F doubles; AssertionError on any other size"""
    t = np.ascontiguousarray(track, dtype=np.float64)
    if t.size != 2 * int(n_frames):
        raise AssertionError(f"ctrack: the track has {t.size} doubles, expected 2 * {int(n_frames)}")
    return t.reshape(int(n_frames), 2)


def constant_track(n_frames, kappa, phi=0.0, slope=0.0):
    """a_f = fl64(fl64(f * kappa) + phi), b_f = slope: the weights of cstack(kappa, phi) when slope == 0 (bit for bit), and with
    slope = the whole turns per frame of a retune the track that keeps a new buffer on the old state"""
    t = np.empty((int(n_frames), 2), np.float64)
    t[:, 0] = np.arange(int(n_frames), dtype=np.float64) * np.float64(kappa) + np.float64(phi)
    t[:, 1] = np.float64(slope)
    return t


def unwrap_turns(r, keep):
    """r (turns, any branch) with every kept entry moved by whole turns to lie nearest to the kept entry before it; an entry that is
    not kept takes its predecessor's value"""
    out = np.array(r, np.float64)
    last = None
    for f in range(out.size):
        if not keep[f]:
            out[f] = 0.0 if last is None else last
            continue
        if last is not None:
            out[f] += round(last - out[f])
        last = out[f]
    return out


def fit_track(rho, track, degree=2):
    """rho: complex[F], the probe's rho_f measured along `track`.  r_f = arg(rho_f) / 2 pi, unwrapped sequentially; p = the least-squares
    polynomial of `degree` in f with weights |rho_f| (a frame with rho_f == 0 has no say; the degree is lowered to what the frames
    with weight determine); the frame's phase is measured at its middle, so a_f += p(f) - p'(f) / 2 and b_f += p'(f).
    -> (the new track, p as numpy.poly1d)"""
    rho = np.asarray(rho, np.complex128).reshape(-1)
    F = rho.size
    t = as_track(track, F).copy()
    w = np.abs(rho)
    keep = (w > 0) & np.isfinite(w)
    if not keep.any():
        return t, np.poly1d([0.0])
    r = unwrap_turns(np.angle(rho) / (2.0 * math.pi), keep)
    f = np.arange(F, dtype=np.float64)
    deg = max(0, min(int(degree), int(np.count_nonzero(keep)) - 1))
    p = np.poly1d(np.polyfit(f[keep], r[keep], deg, w=np.sqrt(w[keep])))   # polyfit weighs the residuals: sqrt for the squares
    dp = p.deriv()
    t[:, 0] += p(f) - 0.5 * dp(f)
    t[:, 1] += dp(f)
    return t, p


def probe_record(out, n_frames):
    """the probe's 4F + 1 doubles -> (rho complex128[F], E_f float64[F], gamma float64[F], E_s)"""
    F = int(n_frames)
    o = np.asarray(out, np.float64)
    rec = o[:4 * F].reshape(F, 4)
    return rec[:, 0] + 1j * rec[:, 1], rec[:, 2].copy(), rec[:, 3].copy(), float(o[4 * F])


def ctrack_stack_d(ctx, iq, fmt, scale, n, t0, T, track, n_frames, y_t, x_t, alpha, mode, zstate, mag=None, info=None):
    """device pointers: cstack_d with `track` (2 * n_frames float64 on the device) in place of kappa and phi: frame f on line l is
    turned by -(a_f + b_f * (l + 1/2) / y_t) turns.  Enqueues on the context's stream and returns -- tsdr_ctrack_stack_iq_d"""
    from . import api
    code, sc, n = _iq_args(fmt, scale, n)
    ctx.call("tsdr_ctrack_stack_iq_d", api._ptr(iq), code, sc, n, C.c_double(t0), C.c_double(T), api._ptr(track), int(n_frames), int(y_t),
             int(x_t), C.c_float(alpha), mode_code(mode), api._ptr(zstate), api._ptr(mag), api._ptr(info))


def ctrack_stack(ctx, iq, t0, T, track, n_frames, y_t, x_t, alpha=0.0, mode="given", zstate=None, fmt="cf32", scale=1.0):
    """host arrays -> (zstate complex64 (y_t, x_t) Fortran-order, mag float32 (y_t, x_t) Fortran-order, info float64[8]): one
    stacking step of `iq` along `track` onto `zstate` (left untouched; required when alpha != 0) -- tsdr_ctrack_stack_iq"""
    from . import api
    a, code, n = _host_iq(iq, fmt)
    P = int(y_t) * int(x_t)
    t = as_track(track, n_frames)
    if alpha != 0.0 and zstate is None:
        raise AssertionError("ctrack_stack: alpha != 0 needs a zstate")
    z = np.zeros(P, np.complex64) if zstate is None else np.asarray(zstate, np.complex64).reshape(-1, order="F").copy()
    if z.size != P:
        raise AssertionError(f"ctrack_stack: zstate has {z.size} pixels, expected {P}")
    mag = np.zeros(P, np.float32)
    info = np.zeros(CSTACK_INFO, np.float64)
    ctx.call("tsdr_ctrack_stack_iq", api._ptr(a), code, C.c_float(scale), n, C.c_double(t0), C.c_double(T), api._ptr(t), int(n_frames),
             int(y_t), int(x_t), C.c_float(alpha), mode_code(mode), api._ptr(z), api._ptr(mag), api._ptr(info))
    shape = (int(y_t), int(x_t))
    return z.reshape(shape, order="F"), mag.reshape(shape, order="F"), info


def ctrack_probe_d(ctx, iq, fmt, scale, n, t0, T, track, n_frames, y_t, x_t, zref, out):
    """device pointers: out (4 * n_frames + 1 float64) <- per frame Re rho_f, Im rho_f, E_f, gamma_f, then E_s, of the frames of
    `iq` turned along `track` (None: the zero track) against the picture zref (y_t * x_t complex64 in state order).  Enqueues on the
    context's stream and returns -- tsdr_ctrack_probe_iq_d"""
    from . import api
    code, sc, n = _iq_args(fmt, scale, n)
    ctx.call("tsdr_ctrack_probe_iq_d", api._ptr(iq), code, sc, n, C.c_double(t0), C.c_double(T), api._ptr(track), int(n_frames), int(y_t),
             int(x_t), api._ptr(zref), api._ptr(out))


def ctrack_probe(ctx, iq, t0, T, track, n_frames, y_t, x_t, zref, fmt="cf32", scale=1.0):
    """host arrays -> (rho complex128[F], E_f float64[F], gamma float64[F], E_s) -- tsdr_ctrack_probe_iq.  track: (F, 2) or None"""
    from . import api
    a, code, n = _host_iq(iq, fmt)
    P, F = int(y_t) * int(x_t), int(n_frames)
    t = None if track is None else as_track(track, F)
    z = np.ascontiguousarray(np.asarray(zref, np.complex64).reshape(-1, order="F"))
    if z.size != P:
        raise AssertionError(f"ctrack_probe: zref has {z.size} pixels, expected {P}")
    out = np.zeros(4 * F + 1, np.float64)
    ctx.call("tsdr_ctrack_probe_iq", api._ptr(a), code, C.c_float(scale), n, C.c_double(t0), C.c_double(T), api._ptr(t), F, int(y_t),
             int(x_t), api._ptr(z), api._ptr(out))
    return probe_record(out, F)


def refine_track(ctx, iq_d, fmt, scale, n, t0, T, n_frames, y_t, x_t, kappa, iterations=2, degree=2, zstate=None, mag=None):
    """The carrier's phase track of one buffer from a start kappa (refine_carrier's): a stack along constant_track(F, kappa) with
    alpha = 0; then `iterations` times: probe the frames against that picture, fit_track, stack again along the new track.
    iq_d: device pointer to n samples of format `fmt`; zstate (complex64) / mag (float32): optional device pointers to y_t * x_t
    elements that hold the last stack on return.  Synchronises once per iteration.
    -> (track (F, 2), [p per iteration], [gamma float64[F] per iteration])"""
    F, P = int(n_frames), int(y_t) * int(x_t)
    if F < 1 or int(iterations) < 0:
        raise AssertionError("refine_track: n_frames must be positive and iterations not negative")
    track = constant_track(F, kappa)
    own = ctx.dev_alloc(8 * P) if zstate is None else None
    d_z = own if zstate is None else zstate
    d_track, d_out = ctx.dev_alloc(16 * F), ctx.dev_alloc(8 * (4 * F + 1))
    polys, gammas = [], []

    def stack():
        ctx.call("tsdr_upload", C.c_void_p(d_track), C.c_void_p(track.ctypes.data), track.nbytes)
        ctrack_stack_d(ctx, iq_d, fmt, scale, n, t0, T, d_track, F, y_t, x_t, 0.0, "given", d_z, mag, None)

    try:
        stack()
        for _ in range(int(iterations)):
            ctrack_probe_d(ctx, iq_d, fmt, scale, n, t0, T, d_track, F, y_t, x_t, d_z, d_out)
            ctx.synchronize()
            rho, _, gamma, _ = probe_record(ctx.download(d_out, (4 * F + 1,), np.float64), F)
            track, p = fit_track(rho, track, degree)
            polys.append(p)
            gammas.append(gamma)
            stack()
        ctx.synchronize()
    finally:
        for d in (own, d_track, d_out):
            if d:
                ctx.dev_free(d)
    return track, polys, gammas
