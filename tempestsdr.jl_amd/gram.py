"""The frame Gram matrix -- G[f][g] = sum_m v_f(m) conj(v_g(m)), every pair of frames' inner product along a track -- through the
entry points of include/tempest_hip_gram.h (their names: _lib.GRAM_IQ_D, _lib.GRAM_IQ).  Every call of those symbols is here;
api.Context.ctrack_gram* / gram_* / track_slopes / blind_track / coherent_period_scan delegate to this module.

G is F x F complex numbers, each with the processing gain of all P pixels.  From G alone, on the host, with no further pass over the
IQ: gram_energy, the energy of the coherent fold for any per-frame turns; gram_carrier, the maximum of the whole kappa periodogram
(what cfold.refine_carrier finds with two scans); gram_phases, every frame's carrier phase against the stack of all the others, with
no reference picture and no model of the drift.  blind_track is the loop around them that needs no start kappa;
coherent_period_scan is the joint (T, kappa) search at one launch per trial period."""
import ctypes as C
import math

import numpy as np

from . import _lib
from .ctrack import as_track, ctrack_stack_d
from .fold import _host_iq, _iq_args, fold_plan

MAX_FRAMES = _lib.GRAM_MAX_FRAMES


def ctrack_gram_d(ctx, iq, fmt, scale, n, t0, T, track, n_frames, y_t, x_t, gram):
    """device pointers: gram (2 * n_frames^2 float64, row-major (re, im) pairs) <- the Gram matrix of the frames of `iq` turned along
    `track` (2 * n_frames float64 on the device; None: the zero track).  Enqueues on the context's stream and returns"""
    from . import api
    code, sc, n = _iq_args(fmt, scale, n)
    ctx.call(_lib.GRAM_IQ_D, api._ptr(iq), code, sc, n, C.c_double(t0), C.c_double(T), api._ptr(track), int(n_frames), int(y_t), int(x_t),
             api._ptr(gram))


def ctrack_gram(ctx, iq, t0, T, track, n_frames, y_t, x_t, fmt="cf32", scale=1.0):
    """host arrays -> G complex128 (F, F).  track: (F, 2) or None"""
    from . import api
    a, code, n = _host_iq(iq, fmt)
    F = int(n_frames)
    t = None if track is None else as_track(track, F)
    out = np.zeros(2 * F * F, np.float64)
    ctx.call(_lib.GRAM_IQ, api._ptr(a), code, C.c_float(scale), n, C.c_double(t0), C.c_double(T), api._ptr(t), F, int(y_t), int(x_t),
             api._ptr(out if F else np.zeros(2)))
    return gram_matrix(out, F)


def gram_matrix(out, n_frames):
    """the 2 F^2 doubles of the library -> complex128 (F, F)"""
    F = int(n_frames)
    o = np.asarray(out, np.float64).reshape(F, F, 2)
    return o[:, :, 0] + 1j * o[:, :, 1]


def _square(G):
    G = np.asarray(G, np.complex128)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise AssertionError(f"gram: G must be square (got {G.shape})")
    return G


def gram_energy(G, turns):
    """the energy sum_m |Z(m)|^2 of the coherent fold Z = (1/F) sum_f exp(-2 pi i a_f) v_f for per-frame turns a_f = turns[f]:
    (1/F^2) sum_fg w_f conj(w_g) G[f][g].  At a_f = f * kappa it is the carrier scan's score; for a track with b = 0 the stack's E_z"""
    G = _square(G)
    a = np.asarray(turns, np.float64).reshape(-1)
    if a.size != G.shape[0]:
        raise AssertionError(f"gram_energy: {a.size} turns for {G.shape[0]} frames")
    w = np.exp(-2j * np.pi * (a - np.floor(a)))
    return float(np.real(w @ G @ np.conj(w))) / float(a.size) ** 2


def lag_sums(G):
    """R(d) = sum_f G[f + d][f], d = 0 .. F-1: the energy at a_f = f * kappa is (R(0) + 2 Re sum_{d >= 1} exp(-2 pi i d kappa) R(d)) / F^2"""
    G = _square(G)
    return np.array([np.trace(G, offset=-d) for d in range(G.shape[0])], np.complex128)


def gram_carrier(G, oversample=16, steps=4):
    """-> (kappa mod 1, energy): the maximum of the kappa periodogram of G.  The lag sums R(d); the energy on a grid of
    oversample * F points over [0, 1); its first maximum; then `steps` Newton steps on the energy's derivative, each kept inside one
    grid step (a step is taken only where the second derivative is negative)"""
    R = lag_sums(G)
    F = R.size
    d = np.arange(1, F, dtype=np.float64)

    def energy(k, order=0):
        c = (-2j * np.pi * d) ** order * np.exp(-2j * np.pi * d * k) * R[1:]
        return ((R[0].real if order == 0 else 0.0) + 2.0 * float(np.sum(c).real)) / float(F) ** 2

    if F == 1:
        return 0.0, energy(0.0)
    n = int(oversample) * F
    h = 1.0 / n
    grid = 2.0 * np.real(np.exp(-2j * np.pi * h * np.outer(np.arange(n), d)) @ R[1:])   # (the constant R(0) moves no maximum)
    k = float(np.argmax(grid)) * h
    for _ in range(int(steps)):
        e1, e2 = energy(k, 1), energy(k, 2)
        if not e2 < 0.0:
            break
        k += min(max(-e1 / e2, -h), h)
    return k % 1.0, energy(k)


def gram_phases(G, iters=50):
    """-> (v, rho): v_f of unit modulus, the carrier phase of frame f with v_0 = 1; rho = G0 v, what the probe would measure for frame
    f against the stack of all other frames.  G0 = G with a zero diagonal; v starts as the eigenvector of G0's largest eigenvalue
    scaled entrywise to unit modulus (a zero entry becomes 1), then r = G0 v, v <- r / |r| (v_f kept where r_f == 0) until
    max |dv| <= 1e-12 or `iters` iterations"""
    G0 = _square(G).copy()
    F = G0.shape[0]
    np.fill_diagonal(G0, 0.0)
    if F == 1:
        return np.ones(1, np.complex128), np.zeros(1, np.complex128)
    v = np.linalg.eigh(0.5 * (G0 + G0.conj().T))[1][:, -1]
    m = np.abs(v)
    v = np.where(m > 0, v / np.where(m > 0, m, 1.0), 1.0 + 0j)
    for _ in range(int(iters)):
        r = G0 @ v
        m = np.abs(r)
        nv = np.where(m > 0, r / np.where(m > 0, m, 1.0), v)
        done = float(np.max(np.abs(nv - v))) <= 1e-12
        v = nv
        if done:
            break
    v = v * np.conj(v[0])
    v[0] = 1.0
    return v, G0 @ v


def gram_track(G, track=None, v=None):
    """-> track (F, 2): `track` (None: zeros), the track G was measured along, with a_f += arg(v_f) / 2 pi; v: gram_phases(G)[0]
    when the caller has it already"""
    G = _square(G)
    F = G.shape[0]
    t = np.zeros((F, 2)) if track is None else as_track(track, F).copy()
    if v is None:
        v = gram_phases(G)[0]
    t[:, 0] += np.angle(v) / (2.0 * math.pi)
    return t


def track_slopes(track):
    """-> the track with its advance per frame taken from the phase differences: d_f = a_{f+1} - a_f, d_0 moved into [-1/2, 1/2), every
    later d_f moved by whole turns to lie nearest its predecessor; b_f = the mean of d_{f-1} and d_f (one-sided at the ends);
    a_f <- a_f - b_f / 2 (a measured phase belongs to the frame's middle, a_f to its start)"""
    t = np.array(track, np.float64)
    t = t.reshape(t.size // 2, 2).copy()
    F = t.shape[0]
    if F < 2:
        t[:, 1] = 0.0
        return t
    d = np.diff(t[:, 0])
    d[0] -= math.floor(d[0] + 0.5)
    for f in range(1, F - 1):
        d[f] += round(d[f - 1] - d[f])
    b = np.empty(F)
    b[0], b[-1] = d[0], d[-1]
    b[1:-1] = 0.5 * (d[:-1] + d[1:])
    t[:, 1] = b
    t[:, 0] -= 0.5 * b
    return t


def _gram_of(ctx, iq_d, fmt, scale, n, t0, T, track, F, y_t, x_t, d_track, d_gram):
    """one Gram on device buffers the caller owns -> complex128 (F, F); synchronises"""
    if track is not None:
        ctx.call("tsdr_upload", C.c_void_p(d_track), C.c_void_p(track.ctypes.data), track.nbytes)
    ctrack_gram_d(ctx, iq_d, fmt, scale, n, t0, T, None if track is None else d_track, F, y_t, x_t, d_gram)
    ctx.synchronize()
    return gram_matrix(ctx.download(d_gram, (2 * F * F,), np.float64), F)


def blind_track(ctx, iq_d, fmt, scale, n, t0, T, n_frames, y_t, x_t, passes=2, zstate=None, mag=None):
    """The carrier's phase track of one buffer with no start kappa and no reference picture.  Pass 1: the Gram matrix with no track,
    gram_phases, track_slopes.  Every further pass: the Gram matrix along the slope-only track (0, b_f); the track becomes
    (arg v_f / 2 pi, b_f).  Then one stack along the track with alpha = 0 (GIVEN).  iq_d: device pointer to n samples of format
    `fmt`; zstate (complex64) / mag (float32): optional device pointers to y_t * x_t elements that hold the stack on return.
    Synchronises once per pass.  -> (track (F, 2), |rho| float64[F] of the last pass)"""
    F, P = int(n_frames), int(y_t) * int(x_t)
    if F < 1 or F > MAX_FRAMES or int(passes) < 1:
        raise AssertionError(f"blind_track: n_frames must be in [1, {MAX_FRAMES}] and passes positive")
    own = ctx.dev_alloc(8 * P) if zstate is None else None
    d_track, d_gram = ctx.dev_alloc(16 * F), ctx.dev_alloc(16 * F * F)
    try:
        G = _gram_of(ctx, iq_d, fmt, scale, n, t0, T, None, F, y_t, x_t, d_track, d_gram)
        v, rho = gram_phases(G)
        track = track_slopes(gram_track(G, None, v))
        for k in range(1, int(passes)):
            if k > 1:   # the slopes again, from the phases at the frames' middles
                track = track_slopes(np.stack([track[:, 0] + 0.5 * track[:, 1], np.zeros(F)], axis=1))
            slopes = np.ascontiguousarray(np.stack([np.zeros(F), track[:, 1]], axis=1))
            G = _gram_of(ctx, iq_d, fmt, scale, n, t0, T, slopes, F, y_t, x_t, d_track, d_gram)
            v, rho = gram_phases(G)
            track = gram_track(G, slopes, v)
        track = np.ascontiguousarray(track)
        ctx.call("tsdr_upload", C.c_void_p(d_track), C.c_void_p(track.ctypes.data), track.nbytes)
        ctrack_stack_d(ctx, iq_d, fmt, scale, n, t0, T, d_track, F, y_t, x_t, 0.0, "given", own if zstate is None else zstate, mag, None)
        ctx.synchronize()
    finally:
        for d in (own, d_track, d_gram):
            if d:
                ctx.dev_free(d)
    return track, np.abs(rho)


def coherent_period_scan(ctx, iq_d, fmt, scale, n, t0, y_t, x_t, periods):
    """The joint (T, kappa) search at one launch per trial period: for every T of `periods`, the Gram matrix (no track) of the
    F = min(fold_plan(n, t0, T), MAX_FRAMES) frames the buffer holds at that T, then gram_carrier.
    -> (energies float64[K], kappas float64[K], best): best = the index of the first maximum of the energies"""
    Ts = [float(T) for T in periods]
    if not Ts:
        raise AssertionError("coherent_period_scan: no trial period")
    Fs = [min(fold_plan(int(n), t0, T)[0], MAX_FRAMES) for T in Ts]
    if min(Fs) < 1:
        raise AssertionError("coherent_period_scan: a trial period leaves no whole frame in the buffer")
    d_gram = ctx.dev_alloc(16 * max(Fs) ** 2)
    energies, kappas = np.zeros(len(Ts)), np.zeros(len(Ts))
    try:
        for k, (T, F) in enumerate(zip(Ts, Fs)):
            kappas[k], energies[k] = gram_carrier(_gram_of(ctx, iq_d, fmt, scale, n, t0, T, None, F, y_t, x_t, None, d_gram))
    finally:
        ctx.dev_free(d_gram)
    return energies, kappas, int(np.argmax(energies))
