"""numpy f64 reference of coherent frame folding, written from the contract in include/tempest_hip_fold.h (SAMPLING, ACCURACY, SCORE),
not from the kernels: the fold, the score of a folded picture, the error bounds the GPU tests assert, and the period ladder of
fold.refine_period.  Everything is float64 except `a`, which is what the contract says the samples are: f32 |IQ| of the converted
samples, computed in f64 and rounded once."""
import math

import numpy as np

ULP = 2.0 ** -24


def amplitudes(iq):
    """a[k] = |IQ[k]| as f32: f64 square root of the exact f64 squares, rounded once"""
    z = np.asarray(iq, np.complex64)
    return np.sqrt(z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2).astype(np.float32)


def fold_mean(a, t0, T, F, y_t, x_t):
    """mean(m), m = l * x_t + p, float64[P]: the mean over f < F of a sampled at u_f(m) = (t0 + f T) + ((m + 1/2)(T/P) - 1/2),
    clamped to the buffer, linearly interpolated"""
    a = np.asarray(a, np.float64)
    n, P = a.size, y_t * x_t
    w = (np.arange(P, dtype=np.float64) + 0.5) * (T / P) - 0.5
    acc = np.zeros(P, np.float64)
    for f in range(F):
        u = np.clip((t0 + f * T) + w, 0.0, n - 1.0)
        k = np.minimum(np.floor(u), n - 2.0).astype(np.int64)
        d = u - k
        acc += a[k] + d * (a[k + 1] - a[k])
    return acc / F


def to_state(mean, y_t, x_t):
    """mean(m) in the order of the state: element (line l, pixel p) at p * y_t + l"""
    return np.asarray(mean).reshape(y_t, x_t).reshape(-1, order="F")


def fold(a, t0, T, F, y_t, x_t, alpha=0.0, state=None):
    """the state after the call, float64[P] in state order; alpha == 0: the state is not read"""
    m = to_state(fold_mean(a, t0, T, F, y_t, x_t), y_t, x_t)
    if alpha == 0:
        return m
    al = float(np.float32(alpha))
    return al * np.asarray(state, np.float64) + (1.0 - al) * m


def eps(F, amax, state_max=0.0):
    """|state - ref| <= (F + 8) * 2^-24 * max(amax, max |state_in|)"""
    return (F + 8) * ULP * max(float(amax), float(state_max))


def score_of(mean):
    x = np.asarray(mean, np.float64)
    return float(np.sum(x * x) - np.sum(x) ** 2 / x.size)


def score_bound(e, P, ref):
    """|score - ref| <= 2 eps sqrt(P ref) + P eps^2"""
    return 2.0 * e * math.sqrt(P * max(ref, 0.0)) + P * e * e


def scan(a, t0, T0, dT, n_trials, F, y_t, x_t):
    """score of the picture folded at T0 + k dT, k < n_trials"""
    return np.array([score_of(fold_mean(a, t0, T0 + k * dT, F, y_t, x_t)) for k in range(n_trials)])


def first_max(s):
    best = -1
    for k, v in enumerate(s):
        if v == v and (best < 0 or v > s[best]):
            best = k
    return best


def top2_margin(s):
    """(best - second best) / best of a score vector"""
    o = np.sort(np.asarray(s, np.float64))
    return float((o[-1] - o[-2]) / o[-1])


def ladder(a, T_guess, F, y_t, x_t, dT=0.125, half=8, levels=2, shrink=4, t0=0.0):
    """fold.refine_period on the reference's scores -> (T_hat, last_dT, [scores per level])"""
    T_hat, step, last, out = float(T_guess), float(dT), float(dT), []
    for _ in range(levels):
        T0 = T_hat - half * step
        s = scan(a, t0, T0, step, 2 * half + 1, F, y_t, x_t)
        out.append(s)
        T_hat, last, step = T0 + first_max(s) * step, step, step / shrink
    return T_hat, last, out


def sig_to_image_1d(a, y_t, x_t):
    """sig_to_image restated with np.interp: pixel m of P samples the S-sample signal at (m + 1/2) S / P - 1/2, clamped to
    [0, S - 1] -- float64[P] in line-major order"""
    a = np.asarray(a, np.float64)
    S, P = a.size, y_t * x_t
    x = np.clip((np.arange(P, dtype=np.float64) + 0.5) * (S / P) - 0.5, 0.0, S - 1.0)
    return np.interp(x, np.arange(S, dtype=np.float64), a)
