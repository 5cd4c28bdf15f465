"""numpy f64 reference of phase-coherent frame folding, written from the contract in include/tempest_hip_cfold.h (SAMPLING, WEIGHT,
RESULT, ACCURACY, SCORE), not from the kernels: the complex fold, the state after the IIR, the energy score, the error bounds the GPU
tests assert, and the carrier ladder of cfold.refine_carrier.  Everything is float64 / complex128 except the samples, which are what
the contract says they are: the converted complex f32 pairs.  Weights are exact (not rounded to f32): the bound budgets that rounding."""
import math

import numpy as np

from fold_ref import ULP, first_max, score_bound, to_state, top2_margin  # noqa: F401  (shared helpers, same definitions)


def samples(iq):
    """z[k]: the complex64 samples, widened exactly to complex128"""
    return np.asarray(iq, np.complex64).astype(np.complex128)


def zfold_mean(z, t0, T, kappa, F, y_t, x_t):
    """Z(m), m = l * x_t + p, complex128[P]: the mean over f < F of exp(-2 pi i r_f) * z sampled at
    u_f(m) = (t0 + f T) + ((m + 1/2)(T/P) - 1/2), clamped to the buffer, linearly interpolated; r_f = frac(f * kappa)"""
    z = np.asarray(z, np.complex128)
    n, P = z.size, y_t * x_t
    w = (np.arange(P, dtype=np.float64) + 0.5) * (T / P) - 0.5
    acc = np.zeros(P, np.complex128)
    for f in range(F):
        u = np.clip((t0 + f * T) + w, 0.0, n - 1.0)
        k = np.minimum(np.floor(u), n - 2.0).astype(np.int64)
        d = u - k
        x = float(f) * float(kappa)
        r = x - math.floor(x)
        acc += complex(math.cos(2.0 * math.pi * r), -math.sin(2.0 * math.pi * r)) * (z[k] + d * (z[k + 1] - z[k]))
    return acc / F


def cfold(z, t0, T, kappa, F, y_t, x_t, alpha=0.0, state=None):
    """the state after the call, float64[P] in state order; alpha == 0: the state is not read"""
    c = to_state(np.abs(zfold_mean(z, t0, T, kappa, F, y_t, x_t)), y_t, x_t)
    if alpha == 0:
        return c
    al = float(np.float32(alpha))
    return al * np.asarray(state, np.float64) + (1.0 - al) * c


def eps_z(F, amax):
    """|Z - Zref| <= sqrt(2) * (F + 12) * 2^-24 * amax"""
    return math.sqrt(2.0) * (F + 12) * ULP * float(amax)


def eps_c(F, amax, state_max=0.0):
    """|state - ref| <= 1.5 * (F + 16) * 2^-24 * max(amax, max |state_in|)"""
    return 1.5 * (F + 16) * ULP * max(float(amax), float(state_max))


def energy(Z):
    """score of a complex picture: sum_m Re^2 + Im^2"""
    Z = np.asarray(Z, np.complex128)
    return float(np.sum(Z.real * Z.real + Z.imag * Z.imag))


def scan(z, t0, T, kappa0, dkappa, n_trials, F, y_t, x_t):
    """energy of the picture folded at kappa0 + k dkappa, k < n_trials, all at the one period T"""
    return np.array([energy(zfold_mean(z, t0, T, kappa0 + k * dkappa, F, y_t, x_t)) for k in range(n_trials)])


def ladder(z, t0, T, F, y_t, x_t, oversample=4, half=8, levels=2, shrink=4):
    """cfold.refine_carrier on the reference's scores -> (kappa_hat mod 1, last_dkappa, [scores per level])"""
    nt0, nt = oversample * F, 2 * half + 1
    step = 1.0 / nt0
    kappa0, count, last, out, kappa_hat = 0.0, nt0, step, [], 0.0
    for _ in range(levels):
        s = scan(z, t0, T, kappa0, step, count, F, y_t, x_t)
        out.append(s)
        kappa_hat, last = kappa0 + first_max(s) * step, step
        step = step / shrink
        kappa0, count = kappa_hat - half * step, nt
    return kappa_hat % 1.0, last, out
