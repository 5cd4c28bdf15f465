"""numpy f64 reference of carrier tracking, written from the contract in include/tempest_hip_ctrack.h (TRACK, SAMPLING, RESULT,
ACCURACY), not from the kernels, on top of cfold_ref / cstack_ref: the samples of one frame, the weight of a frame on a line, the
picture Z folded along a track, the stack, the probe's record, the error bounds the GPU tests assert, constant_track and fit_track.
Everything is float64 / complex128; the weights are exact (not rounded to f32): the bounds budget that rounding.  A track is a
float64 array of shape (F, 2): (a_f, b_f) in turns."""
import math

import numpy as np

import cstack_ref as CS
from cfold_ref import ULP, samples, to_state  # noqa: F401  (shared helpers, same definitions)

GIVEN, LOCK = CS.GIVEN, CS.LOCK
TERM = 12   # eps_t = sqrt(2) * TERM * 2^-24 * amax: the F-independent part of cfold_ref.eps_z


def frame_samples(z, t0, T, f, y_t, x_t):
    """z_f(m), m = l * x_t + p, complex128[P]: z sampled at u_f(m) = (t0 + f T) + ((m + 1/2)(T/P) - 1/2), clamped to the buffer,
    linearly interpolated (SAMPLING: cfold_ref.zfold_mean's frame f)"""
    z = np.asarray(z, np.complex128)
    n, P = z.size, y_t * x_t
    u = np.clip((t0 + f * T) + ((np.arange(P, dtype=np.float64) + 0.5) * (T / P) - 0.5), 0.0, n - 1.0)
    k = np.minimum(np.floor(u), n - 2.0).astype(np.int64)
    return z[k] + (u - k) * (z[k + 1] - z[k])


def line_turns(track, f, y_t):
    """x of TRACK for every line of frame f, float64[y_t]: b_f * (l + 1/2) / y_t + a_f"""
    a, b = float(track[f][0]), float(track[f][1])
    return b * ((np.arange(y_t, dtype=np.float64) + 0.5) / y_t) + a


def line_weights(track, f, y_t):
    """w_f(l) = exp(-2 pi i r), r = x - floor(x), complex128[y_t]"""
    x = line_turns(track, f, y_t)
    return np.exp(-2j * np.pi * (x - np.floor(x)))


def turned_frame(z, t0, T, track, f, y_t, x_t):
    """v_f(m) = w_f(l) z_f(m) in raster order, complex128[P]; track None: the zero track"""
    zf = frame_samples(z, t0, T, f, y_t, x_t)
    if track is None:
        return zf
    return (line_weights(track, f, y_t)[:, None] * zf.reshape(y_t, x_t)).reshape(-1)


def zmean(z, t0, T, track, F, y_t, x_t):
    """Z in STATE order (pixel (l, p) at p * y_t + l), complex128[P]: the mean over f < F of w_f(l) z_f(m)"""
    acc = np.zeros(y_t * x_t, np.complex128)
    for f in range(F):
        acc += turned_frame(z, t0, T, track, f, y_t, x_t)
    return to_state(acc / F, y_t, x_t)


def ctrack(z, t0, T, track, F, y_t, x_t, alpha=0.0, mode=GIVEN, S=None):
    """the stack itself on samples z: -> (S', |S'|, info): cstack_ref.step on the tracked Z"""
    out, info = CS.step(zmean(z, t0, T, track, F, y_t, x_t), alpha, mode, S)
    return out, np.abs(out), info


def probe(z, t0, T, track, F, y_t, x_t, S):
    """the probe's record: -> (rho complex128[F], E_f float64[F], gamma float64[F], E_s); S in state order"""
    S = np.asarray(S, np.complex128)
    E_s = float(np.sum(np.abs(S) ** 2))
    rho, E_f, gamma = np.zeros(F, np.complex128), np.zeros(F), np.zeros(F)
    for f in range(F):
        v = to_state(turned_frame(z, t0, T, track, f, y_t, x_t), y_t, x_t)
        rho[f] = np.sum(v * np.conj(S))
        E_f[f] = float(np.sum(np.abs(v) ** 2))
        den = E_f[f] * E_s
        gamma[f] = abs(rho[f]) / math.sqrt(den) if den > 0.0 else 0.0
    return rho, E_f, gamma, E_s


# ---------------------------------------------------------------- the bounds of ACCURACY (the probe; the stack's are cstack_ref's)
def eps_t(amax):
    """|v - ref| <= sqrt(2) * 12 * 2^-24 * amax"""
    return math.sqrt(2.0) * TERM * ULP * float(amax)


def eps_rho(amax, P, E_f, E_s):
    """|rho_f - ref| <= eps_t * sqrt(P * E_s) + 2^-36 * sqrt(E_f * E_s)"""
    return eps_t(amax) * math.sqrt(P * E_s) + 2.0 ** -36 * math.sqrt(E_f * E_s)


def eps_ef(amax, P, E_f):
    """|E_f - ref| <= 2 eps_t sqrt(P ref) + P eps_t^2 + 2^-36 ref"""
    e = eps_t(amax)
    return 2.0 * e * math.sqrt(P * E_f) + P * e * e + 2.0 ** -36 * E_f


def eps_es(E_s):
    return 2.0 ** -36 * E_s


# ---------------------------------------------------------------- tracks
def constant_track(F, kappa, phi=0.0, slope=0.0):
    """a_f = fl64(fl64(f * kappa) + phi), b_f = slope"""
    t = np.empty((F, 2), np.float64)
    for f in range(F):
        x = float(f) * float(kappa)
        t[f, 0] = x + float(phi)
        t[f, 1] = float(slope)
    return t


def fit_track(rho, track, degree=2):
    """-> (new track, p): r_f = arg(rho_f) / 2 pi unwrapped so that each lies nearest to its predecessor (frames with rho_f == 0 are
    passed over), p = the polynomial of `degree` in f that minimises sum |rho_f| (r_f - p(f))^2, a_f += p(f) - p'(f) / 2, b_f += p'(f)"""
    rho = np.asarray(rho, np.complex128)
    F = rho.size
    w = np.abs(rho)
    idx = [f for f in range(F) if w[f] > 0.0]
    t = np.array(track, np.float64).reshape(F, 2).copy()
    if not idx:
        return t, np.poly1d([0.0])
    r, last = [], None
    for f in idx:
        x = math.atan2(rho[f].imag, rho[f].real) / (2.0 * math.pi)
        if last is not None:
            x += round(last - x)
        r.append(x)
        last = x
    fi = np.array(idx, np.float64)
    deg = max(0, min(degree, len(idx) - 1))
    # the normal equations of the weighted problem, solved by least squares on the scaled Vandermonde matrix
    V = np.vander(fi, deg + 1) * np.sqrt(w[idx])[:, None]
    coef = np.linalg.lstsq(V, np.array(r) * np.sqrt(w[idx]), rcond=None)[0]
    p = np.poly1d(coef)
    dp = p.deriv()
    f_all = np.arange(F, dtype=np.float64)
    t[:, 0] += p(f_all) - 0.5 * dp(f_all)
    t[:, 1] += dp(f_all)
    return t, p


def refine_track(z, t0, T, F, y_t, x_t, kappa, iterations=2, degree=2):
    """ctrack.refine_track on the reference: -> (track, [Z in state order after the constant stack and after every iteration])"""
    track = constant_track(F, kappa)
    Z = [zmean(z, t0, T, track, F, y_t, x_t)]
    for _ in range(iterations):
        rho = probe(z, t0, T, track, F, y_t, x_t, Z[-1])[0]
        track, _ = fit_track(rho, track, degree)
        Z.append(zmean(z, t0, T, track, F, y_t, x_t))
    return track, Z
