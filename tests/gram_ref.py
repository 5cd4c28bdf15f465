"""numpy f64 reference of the frame Gram matrix, written from the contract in include/tempest_hip_gram.h (RESULT, ACCURACY), not from
the kernels, on top of ctrack_ref: the matrix itself, the error bound the GPU tests assert, and the host algorithms of gram.py restated
independently (the energy of a fold from G, the carrier from the lag sums, the blind phases, the slopes of a track, the blind
track and the period scan on the reference).  Everything is float64 / complex128."""
import math

import numpy as np

import cstack_ref as CS
import ctrack_ref as R
from cfold_ref import ULP

MAX_FRAMES, CHUNK = 64, 1024
CHAIN = 3 * CHUNK + 64   # c of ACCURACY


def frames(z, t0, T, track, F, y_t, x_t):
    """V[f][m] = v_f(m) in raster order, complex128 (F, P)"""
    return np.stack([R.turned_frame(z, t0, T, track, f, y_t, x_t) for f in range(F)])


def gram(z, t0, T, track, F, y_t, x_t):
    """G[f][g] = sum_m v_f(m) conj(v_g(m)), complex128 (F, F)"""
    V = frames(z, t0, T, track, F, y_t, x_t)
    return V @ V.conj().T


def eps_g(amax, P, E_f, E_g):
    """|G[f][g] - ref| <= eps_t (sqrt(P E_f) + sqrt(P E_g)) + P eps_t^2 + (c u + 2^-36) sqrt(E_f E_g)"""
    e = R.eps_t(amax)
    return e * (math.sqrt(P * E_f) + math.sqrt(P * E_g)) + P * e * e + (CHAIN * ULP + 2.0 ** -36) * math.sqrt(E_f * E_g)


def eps_matrix(amax, P, G):
    """eps_g for every entry of the reference G, float64 (F, F)"""
    E = np.real(np.diag(G))
    F = E.size
    return np.array([[eps_g(amax, P, E[f], E[g]) for g in range(F)] for f in range(F)])


def eps_energy(B, F):
    """the bound of gram_energy from the entries' bounds B: every |w_f conj(w_g)| is 1"""
    return float(np.sum(B)) / float(F) ** 2


# ---------------------------------------------------------------- the host algorithms, restated
def gram_energy(G, turns):
    F = len(turns)
    total = 0.0 + 0.0j
    for f in range(F):
        for g in range(F):
            total += complex(G[f][g]) * np.exp(-2j * math.pi * (float(turns[f]) - float(turns[g])))
    return total.real / F ** 2


def periodogram(G, kappa):
    """the energy at a_f = f kappa from the lag sums R(d) = sum_f G[f + d][f]"""
    F = G.shape[0]
    total = sum(G[f][f] for f in range(F)).real
    for d in range(1, F):
        Rd = sum(G[f + d][f] for f in range(F - d))
        total += 2.0 * (np.exp(-2j * math.pi * d * kappa) * Rd).real
    return total / F ** 2


def gram_carrier(G, fine=4096):
    """(kappa, energy): the first maximum of the periodogram on 16 F points, then the best of `fine` points across the two grid steps
    around it (a dense search where gram.py takes Newton steps)"""
    F = G.shape[0]
    if F == 1:
        return 0.0, periodogram(G, 0.0)
    n = 16 * F
    k0 = int(np.argmax([periodogram(G, j / n) for j in range(n)])) / n
    ks = k0 + (np.arange(fine + 1) / fine * 2.0 - 1.0) / n
    e = [periodogram(G, k) for k in ks]
    j = int(np.argmax(e))
    return float(ks[j]) % 1.0, float(e[j])


def gram_phases(G, iters=50):
    F = G.shape[0]
    G0 = np.array(G, np.complex128)
    for f in range(F):
        G0[f, f] = 0.0
    if F == 1:
        return np.ones(1, complex), np.zeros(1, complex)
    w, U = np.linalg.eigh(G0)
    v = U[:, int(np.argmax(w))].copy()
    for f in range(F):
        v[f] = v[f] / abs(v[f]) if abs(v[f]) > 0 else 1.0
    for _ in range(iters):
        r = G0 @ v
        nv = np.array([r[f] / abs(r[f]) if abs(r[f]) > 0 else v[f] for f in range(F)])
        step = float(np.max(np.abs(nv - v)))
        v = nv
        if step <= 1e-12:
            break
    v = v * np.conj(v[0])
    return v, G0 @ v


def gram_track(G, track=None):
    F = G.shape[0]
    t = np.zeros((F, 2)) if track is None else np.array(track, np.float64).reshape(F, 2).copy()
    v = gram_phases(G)[0]
    for f in range(F):
        t[f, 0] += math.atan2(v[f].imag, v[f].real) / (2.0 * math.pi)
    return t


def track_slopes(track):
    t = np.array(track, np.float64).reshape(-1, 2).copy()
    F = t.shape[0]
    if F < 2:
        t[:, 1] = 0.0
        return t
    d = [t[f + 1, 0] - t[f, 0] for f in range(F - 1)]
    d[0] -= math.floor(d[0] + 0.5)
    for f in range(1, F - 1):
        d[f] += round(d[f - 1] - d[f])
    for f in range(F):
        b = d[0] if f == 0 else d[-1] if f == F - 1 else 0.5 * (d[f - 1] + d[f])
        t[f, 1] = b
        t[f, 0] -= 0.5 * b
    return t


def blind_track(z, t0, T, F, y_t, x_t, passes=2):
    """gram.blind_track on the reference -> (track, |rho|, Z in state order along the track)"""
    G = gram(z, t0, T, None, F, y_t, x_t)
    track, rho = track_slopes(gram_track(G)), gram_phases(G)[1]
    for k in range(1, passes):
        if k > 1:
            track = track_slopes(np.stack([track[:, 0] + 0.5 * track[:, 1], np.zeros(F)], axis=1))
        slopes = np.stack([np.zeros(F), track[:, 1]], axis=1)
        G = gram(z, t0, T, slopes, F, y_t, x_t)
        track, rho = gram_track(G, slopes), gram_phases(G)[1]
    return track, np.abs(rho), R.zmean(z, t0, T, track, F, y_t, x_t)


def period_scan(z, t0, y_t, x_t, periods):
    """gram.coherent_period_scan on the reference -> (energies, kappas, best)"""
    out = []
    for T in periods:
        F = min(CS.fold_plan(len(z), t0, T)[0], MAX_FRAMES)
        out.append(gram_carrier(gram(z, t0, T, None, F, y_t, x_t)))
    e = np.array([o[1] for o in out])
    return e, np.array([o[0] for o in out]), int(np.argmax(e))
