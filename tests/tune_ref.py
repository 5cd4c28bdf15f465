"""numpy reference of the tuner (include/tempest_hip_tune.h): the exact uint64 phases, the oscillator and the sums in f64 -- what the
header's error bound is stated against.  There is no f32 restatement of the kernel: bit identity is asserted between GPU results
(chunked against whole, integer formats against ComplexF32, repeats), never against numpy.  Also the capability helpers: the wideband
capture with a strong interferer, the card, the correlation, and the fold through tests/fold_ref.py."""
import math

import numpy as np

import fold_ref as FR

ULP = 2.0 ** -24
M64 = (1 << 64) - 1


def phases(m0, n, nu_fix, phi_fix):
    """p[m] = (phi_fix + nu_fix * m) mod 2^64 for m = m0 .. m0 + n - 1, uint64 (the arithmetic wraps)"""
    with np.errstate(over="ignore"):
        m = np.uint64(int(m0) & M64) + np.arange(int(n), dtype=np.uint64)
        return np.uint64(int(phi_fix) & M64) + np.uint64(int(nu_fix) & M64) * m


def phase_exact(m, nu_fix, phi_fix):
    """the same for one index, in Python integers"""
    return (int(phi_fix) + int(nu_fix) * int(m)) & M64


def oscillator(p):
    """exp(2 pi i p / 2^64) in f64: p as a signed number of half turns (a whole turn less for p >= 2^63)"""
    t = np.asarray(p, np.uint64).view(np.int64).astype(np.float64) * 2.0 ** -63
    return np.cos(np.pi * t) + 1j * np.sin(np.pi * t)


def mixed(x, m0, nu_fix, phi_fix):
    """u[m] = x[m] * w[m] in f64 on the f32 samples, complex128"""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    return x * oscillator(phases(m0, x.size, nu_fix, phi_fix))


def n_out(m0, n, L, D, j0):
    end = int(m0) + int(n)
    return max((end - L) // D - int(j0) + 1, 0) if end >= L else 0


def fir(u, a0, taps, D, j0, count):
    """y[j] = sum_i h[i] u[j D + i], j = j0 .. j0 + count - 1, where u[0] is the mixed sample of absolute index a0; f64"""
    h = np.asarray(taps, np.float32).astype(np.float64)
    if count <= 0:
        return np.zeros(0, np.complex128)
    k0 = int(j0) * D - int(a0)
    assert k0 >= 0 and k0 + (count - 1) * D + h.size <= u.size, "every window lies inside the samples given"
    full = np.convolve(u[k0:k0 + (count - 1) * D + h.size], h[::-1], "valid")   # full[k] = sum_i h[i] u[k0 + k + i]
    return full[::D][:count].copy()


def call(x, m0, nu_fix, phi_fix, taps, D, j0, hist, n_hist):
    """one call of the library in f64: (y, hist_after, n_hist_after); hist: complex128[L - 1], its last n_hist entries u[m0 - n_hist .. m0)"""
    L = np.asarray(taps).size
    H = L - 1
    u_new = mixed(x, m0, nu_fix, phi_fix)
    old = np.asarray(hist, np.complex128)[H - n_hist:H] if n_hist else np.zeros(0, np.complex128)
    u = np.concatenate([old, u_new])
    assert int(j0) * D >= int(m0) - n_hist, "the window reaches before the history"
    y = fir(u, int(m0) - n_hist, taps, D, j0, n_out(m0, u_new.size, L, D, j0))
    keep = min(H, u.size)
    out = np.array(hist, np.complex128) if hist is not None else np.zeros(H, np.complex128)
    if keep:
        out[H - keep:] = u[u.size - keep:]
    return y, out, keep


def whole(x, m0, nu_fix, phi_fix, taps, D, j0=None):
    """the outputs of one call on the whole stream with no history; j0 None: the first window at or after m0"""
    L = np.asarray(taps).size
    if j0 is None:
        j0 = -((-int(m0)) // D)
    return call(x, m0, nu_fix, phi_fix, taps, D, j0, np.zeros(L - 1, np.complex128), 0)[0]


def bound(L, amax, taps):
    """|y[j] - y_ref[j]| <= (L + 8) * 2^-24 * A * H1"""
    return (L + 8) * ULP * float(amax) * float(np.abs(np.asarray(taps, np.float32).astype(np.float64)).sum())


# ---------------------------------------------------------------- the capability: a wideband capture with a strong interferer
CAP = dict(y=66, x=160, T=9150.37, D=4, L=63, F=11, df=0.23, f_int=-0.31, amp=5e-3)


def corr(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float(np.dot(a, b) / math.sqrt(np.dot(a, a) * np.dot(b, b)))


def cap_card(synth):
    """the noiseless card of the capability geometry, in state order"""
    b, y, x = synth.BLANK_BOX, CAP["y"], CAP["x"]
    return synth.test_card(x, y, row0=int(round(b["row0_frac"] * y)) % y, col0=int(round(b["col0_frac"] * x)) % x).reshape(-1, order="F")


_CAPS = {}


def cap_captures(synth):
    """(clean, jammed) complex64: synth_leak at Fs = 60 * 4 * T with the leak's carrier at +0.23 Fs, 0 dB per sample, n = ceil(12 * 4 T)
    + 71; jammed = clean + a carrier 20 dB above the leak's amplitude at -0.31 Fs with 30 % amplitude modulation.  Made once"""
    if "c" not in _CAPS:
        T, D = CAP["T"], CAP["D"]
        Fs = 60.0 * D * T
        n = int(math.ceil(12 * D * T)) + 71
        clean = synth.synth_leak(Fs, CAP["x"], CAP["y"], 60.0, n, snr_db=0.0, df=CAP["df"] * Fs)
        m = np.arange(n, dtype=np.float64)
        jam = 10.0 * CAP["amp"] * (1.0 + 0.3 * np.cos(2.0 * np.pi * 0.00137 * m)) * np.exp(2j * np.pi * ((CAP["f_int"] * m) % 1.0))
        jammed = (clean.astype(np.complex128) + jam).astype(np.complex64)
        clean.setflags(write=False)
        jammed.setflags(write=False)
        _CAPS["c"] = (clean, jammed)
    return _CAPS["c"]


def cap_taps():
    """L = 63: sinc(0.9 i / D) * blackman(L), i centred, normalised to sum 1, f32"""
    L, D = CAP["L"], CAP["D"]
    i = np.arange(L, dtype=np.float64) - (L - 1) / 2.0
    h = np.sinc(0.9 * i / D) * np.blackman(L)
    return (h / h.sum()).astype(np.float32)


def cap_nu():
    """a shift by -0.23 Fs"""
    return int(round(-CAP["df"] * 2.0 ** 64)) & M64


def cap_fold_tuned(y):
    """the tuned stream folded: 11 frames from t0 = T - 31 / 4 at period T, the envelope, state order"""
    return FR.fold(FR.amplitudes(y), CAP["T"] - (CAP["L"] - 1) / 2.0 / CAP["D"], CAP["T"], CAP["F"], CAP["y"], CAP["x"])


def cap_fold_raw(iq):
    """the capture itself folded: 11 frames from t0 = 4 T at period 4 T"""
    return FR.fold(FR.amplitudes(iq), CAP["D"] * CAP["T"], CAP["D"] * CAP["T"], CAP["F"], CAP["y"], CAP["x"])
