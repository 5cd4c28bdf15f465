"""numpy f64 reference of coherent stacking across buffers, written from the contract in include/tempest_hip_cstack.h (WEIGHT, RESULT,
LOCK, INFO, ACCURACY), not from the kernels, on top of cfold_ref.zfold_mean: the complex picture Z with a start phase, the sums
rho, E_z, E_s, the rotation q, the blended complex state, the info record, the error bounds the GPU tests assert, and cstack_plan.
Everything is float64 / complex128; weights and q are exact (not rounded to f32): the bounds budget those roundings."""
import math

import numpy as np

from cfold_ref import ULP, eps_z, samples, to_state, zfold_mean  # noqa: F401  (shared helpers, same definitions)

GIVEN, LOCK = 0, 1


def frac(x):
    return x - math.floor(x)


def weight(f, kappa, phi):
    """w_f = exp(-2 pi i r_f), r_f = frac(f * kappa + phi)"""
    r = frac(float(f) * float(kappa) + float(phi))
    return complex(math.cos(2.0 * math.pi * r), -math.sin(2.0 * math.pi * r))


def zmean(z, t0, T, kappa, phi, F, y_t, x_t):
    """Z in STATE order (pixel (l, p) at p * y_t + l), complex128[P]: every weight of the coherent fold carries the one factor
    exp(-2 pi i phi), so Z = exp(-2 pi i frac(phi)) * zfold_mean"""
    return to_state(weight(0, 0.0, phi) * zfold_mean(z, t0, T, kappa, F, y_t, x_t), y_t, x_t)


def sums(Z, S):
    """(rho, E_z, E_s): rho = sum Z conj(S)"""
    Z, S = np.asarray(Z, np.complex128), np.asarray(S, np.complex128)
    return complex(np.sum(Z * np.conj(S))), float(np.sum(np.abs(Z) ** 2)), float(np.sum(np.abs(S) ** 2))


def rotation(rho, mode):
    """q: (1, 0) in GIVEN mode; rho / |rho| in LOCK mode when |rho| is finite and > 0, else (1, 0)"""
    a = math.hypot(rho.real, rho.imag)
    if mode == LOCK and math.isfinite(a) and a > 0.0:
        return complex(rho.real / a, rho.imag / a)
    return 1.0 + 0.0j


def info_record(rho, E_z, E_s, q):
    """the eight doubles of INFO"""
    a = math.hypot(rho.real, rho.imag)
    theta = 0.0 if rho == 0 else math.atan2(rho.imag, rho.real) / (2.0 * math.pi)
    den = E_z * E_s
    gamma = a / math.sqrt(den) if den > 0.0 else 0.0
    return np.array([rho.real, rho.imag, E_z, E_s, theta, gamma, q.real, q.imag])


def step(Z, alpha, mode, S=None):
    """one call on a picture Z (state order): -> (S' complex128[P], info float64[8]); alpha == 0: S is not read (S = 0 in the sums)"""
    Z = np.asarray(Z, np.complex128)
    al = float(np.float32(alpha))
    S = np.zeros_like(Z) if al == 0.0 else np.asarray(S, np.complex128)
    rho, E_z, E_s = sums(Z, S)
    q = rotation(rho, mode)
    Zq = np.conj(q) * Z
    out = Zq if al == 0.0 else al * S + (1.0 - al) * Zq
    return out, info_record(rho, E_z, E_s, q)


def cstack(z, t0, T, kappa, phi, F, y_t, x_t, alpha=0.0, mode=GIVEN, S=None):
    """the call itself on samples z: -> (S', |S'|, info)"""
    out, info = step(zmean(z, t0, T, kappa, phi, F, y_t, x_t), alpha, mode, S)
    return out, np.abs(out), info


# ---------------------------------------------------------------- the bounds of ACCURACY
def eps_s(F, amax, state_max=0.0):
    """GIVEN: |S' - ref| <= sqrt(2) * (F + 16) * 2^-24 * max(amax, max |S|)"""
    return math.sqrt(2.0) * (F + 16) * ULP * max(float(amax), float(state_max))


def eps_mag(F, amax, state_max=0.0):
    """GIVEN: |mag - |ref|| <= sqrt(2) * (F + 18) * 2^-24 * max(amax, max |S|)"""
    return math.sqrt(2.0) * (F + 18) * ULP * max(float(amax), float(state_max))


def eps_rho(F, amax, P, E_z, E_s):
    """|rho - ref| <= eps_z * sqrt(P * E_s) + 2^-36 * sqrt(E_z * E_s)"""
    return eps_z(F, amax) * math.sqrt(P * E_s) + 2.0 ** -36 * math.sqrt(E_z * E_s)


def eps_ez(F, amax, P, E_z):
    """|E_z - ref| <= 2 eps_z sqrt(P ref) + P eps_z^2 + 2^-36 ref"""
    e = eps_z(F, amax)
    return 2.0 * e * math.sqrt(P * E_z) + P * e * e + 2.0 ** -36 * E_z


def eps_es(E_s):
    return 2.0 ** -36 * E_s


def eps_theta(e_rho, rho_abs):
    """|theta - ref| <= eps_rho / (4 |rho_ref|) + 2^-40 turns (mod 1)"""
    return e_rho / (4.0 * rho_abs) + 2.0 ** -40


def angle_term(amax, e_rho, rho_abs):
    """(pi / 2) * amax * eps_rho / |rho_ref|; absent when rho_ref == 0"""
    return 0.0 if rho_abs == 0.0 else 0.5 * math.pi * float(amax) * e_rho / rho_abs


def eps_lock(F, amax, state_max, e_rho, rho_abs):
    """LOCK: |S' - ref| <= sqrt(2) * (F + 19) * 2^-24 * M + (pi / 2) * amax * eps_rho / |rho_ref|"""
    return math.sqrt(2.0) * (F + 19) * ULP * max(float(amax), float(state_max)) + angle_term(amax, e_rho, rho_abs)


def eps_lock_mag(F, amax, state_max, e_rho, rho_abs):
    """LOCK: |mag - |ref|| <= sqrt(2) * (F + 21) * 2^-24 * M + the same angle term"""
    return math.sqrt(2.0) * (F + 21) * ULP * max(float(amax), float(state_max)) + angle_term(amax, e_rho, rho_abs)


def turn_dist(a, b):
    """distance of two angles in turns, mod 1"""
    return abs((a - b + 0.5) % 1.0 - 0.5)


# ---------------------------------------------------------------- planning
def fold_plan(n, t0, T):
    """(F, next_t0): tempest_hip_fold.h's rule, restated"""
    n, t0, T = float(n), float(t0), float(T)
    if t0 >= n:
        return 0, t0 - n
    F = max(int(math.floor((n - t0) / T)), 0)
    while F > 0 and t0 + F * T > n:
        F -= 1
    while t0 + (F + 1) * T <= n:
        F += 1
    return F, t0 + (F + 1) * T - n


def cstack_plan(n, t0, T, kappa, phi, theta=0.0):
    """(F, next_t0, next_phi): next_phi = frac(phi + theta + (F + 1) kappa); t0 >= n: (0, t0 - n, phi)"""
    F, nt0 = fold_plan(n, t0, T)
    if float(t0) >= float(n):
        return 0, nt0, float(phi)
    return F, nt0, frac(float(phi) + float(theta) + (F + 1) * float(kappa))
