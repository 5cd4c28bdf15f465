"""Numpy restatement, in double, of the Float64 per-function path (the `_f64` entry points of include/tempest_hip.h).

It copies the operation ORDER that oracle/tempest_oracle.c documents for the f32 path (resize_axis / resize_coord /
lin_pos, the "summation orders" comment, fir_filt, fill_beta, argmax_col) with every value kept in f64:
  * numpy's elementwise float64 + - * / are single IEEE operations (no fusion), so each line below is one rounding;
  * the FIR's fused multiply-adds are formed exactly with Fraction and rounded once (CPython's Fraction -> float
    conversion is correctly rounded; Python 3.10 has no math.fma);
  * the Gaussian taps use math.exp, not numpy's vectorised exp, which may differ in the last ulp.
No GPU, no library: the tests pin this module against analytic answers and against the f32 oracle on f32-representable
input, then hold the GPU's f64 results to it bit for bit.
"""
import math
from fractions import Fraction

import numpy as np

RENDER_H, RENDER_W = 600, 800


# ---- imresize (Resampler.jl:117-126) ------------------------------------------------------------------------------
def _axis(n_in, n_out, i1):
    """0-based left index and right weight of the 1-based destination indices i1 (float64 array)"""
    sf = float(n_in) / float(n_out)
    off = (1.0 - 0.5) - sf * (1.0 - 0.5)
    x = sf * i1 + off
    x = np.minimum(np.maximum(x, 1.0), float(n_in))
    xf = np.floor(x)
    xf = np.where(xf > float(n_in) - 1.0, xf - 1.0, xf)
    return xf.astype(np.int64) - 1, x - xf


def _blend(a, b, d):
    return (1.0 - d) * a + d * b


def resize1d(sig, n_out):
    x = np.asarray(sig, np.float64)
    if x.size == n_out:
        return x.copy()
    k, d = _axis(x.size, n_out, np.arange(1, n_out + 1, dtype=np.float64))
    return _blend(x[k], x[k + 1], d)


def sig_to_image(sig, y_t, x_t):
    """column-major (y_t, x_t): img[l, p] = imresize(sig, y_t*x_t)[l*x_t + p]"""
    return np.asfortranarray(resize1d(sig, y_t * x_t).reshape(y_t, x_t))


def resize2d(img, h_out, w_out):
    a = np.asarray(img, np.float64)
    h_in, w_in = a.shape
    if (h_in, w_in) == (h_out, w_out):
        return np.asfortranarray(a.copy())
    ky, dy = _axis(h_in, h_out, np.arange(1, h_out + 1, dtype=np.float64))
    kx, dx = _axis(w_in, w_out, np.arange(1, w_out + 1, dtype=np.float64))
    a00, a10 = a[ky][:, kx], a[ky + 1][:, kx]
    a01, a11 = a[ky][:, kx + 1], a[ky + 1][:, kx + 1]
    top = _blend(a00, a01, dx[None, :])
    bot = _blend(a10, a11, dx[None, :])
    return np.asfortranarray(_blend(top, bot, dy[:, None]))


def downgrade(img):
    return resize2d(img, RENDER_H, RENDER_W)


def naive_resample(x, up):
    return np.repeat(np.asarray(x, np.float64), up)


# ---- FrameSynchronisation.jl --------------------------------------------------------------------------------------
def taps():
    """init_gaussian_filter(5): exp(-2k^2/25)/sum, k = -2..2, in f64 (FrameSynchronisation.jl:124-129)"""
    t = [math.exp(-2.0 * float(k * k) / 25.0) for k in range(-2, 3)]
    s = 0.0
    for v in t:
        s += v
    return [v / s for v in t]


def fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c   # NaN / Inf operands: no rounding is involved, the IEEE result of the unfused form is the fused one
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def col_sums(img):
    """sum(image;dims=1): per column, 64-row blocks accumulated top to bottom from 0.0, block sums added in order"""
    a = np.asarray(img, np.float64)
    y = a.shape[0]
    tot = None
    for r0 in range(0, y, 64):
        acc = np.zeros(a.shape[1])
        for r in range(r0, min(r0 + 64, y)):
            acc = acc + a[r, :]
        tot = acc if tot is None else tot + acc
    return tot


def row_sums(img):
    """sum(image;dims=2): strictly left to right from 0.0 + 0.0"""
    a = np.asarray(img, np.float64)
    acc = np.full(a.shape[0], 0.0 + 0.0)
    for c in range(a.shape[1]):
        acc = acc + a[:, c]
    return acc


def fir(h, x):
    """DSP.jl filt(h, x), transposed direct form with muladd (fma), zero initial state"""
    x = [float(v) for v in x]
    out = []
    for i in range(len(x)):
        g = lambda j: x[i - j] if i - j >= 0 else 0.0  # noqa: E731
        s = h[4] * g(4)
        s = fma(g(3), h[3], s)
        s = fma(g(2), h[2], s)
        s = fma(g(1), h[1], s)
        out.append(fma(g(0), h[0], s))
    return np.array(out)


def sum64(x):
    """sum(c_v): lane m accumulates x[m], x[m+64], ... from 0.0; the 64 partials folded by the tree 32, 16, .., 1"""
    x = np.asarray(x, np.float64)
    p = [0.0] * 64
    for m in range(64):
        a = 0.0
        for i in range(m, x.size, 64):
            a = a + float(x[i])
        p[m] = a
    off = 32
    while off:
        for i in range(off):
            p[i] = p[i] + p[i + off]
        off >>= 1
    return p[0]


def fill_beta(cv, n, w_min, w_max):
    """fill_beta!(beta, c_v, Sync(w_min, w_max, n)) -> (w_max-w_min+1, n) Fortran array (FrameSynchronisation.jl:94-112)"""
    cv = np.asarray(cv, np.float64)
    S = sum64(cv)
    c = np.arange(1, n + 1)
    mod0 = lambda k: (k - 1) % n  # noqa: E731   modIndex, 0-based
    acc = np.zeros(n)
    for k in range(-(w_min - 1), w_min):
        acc = acc + cv[mod0(c + k)]
    s = 2.0 * acc
    W = w_max - w_min + 1
    beta = np.empty((W, n), order="F")
    for cnt, w in enumerate(range(w_min, w_max + 1)):
        s = s + 2.0 * cv[mod0(c - w)]
        s = s + 2.0 * cv[mod0(c + w)]
        v = (S - s) / float(2 * (n - w)) + s / float(2 * w)
        beta[cnt, :] = v * v
    return beta


def argmax_col(beta):
    """findmax(beta)[2][2]: 1-based column of the first maximum in column-major order, NaN maximal"""
    f = np.asarray(beta).ravel(order="F")
    nan = np.flatnonzero(np.isnan(f))
    i = int(nan[0]) if nan.size else int(np.argmax(f))
    return i // beta.shape[0] + 1


def bounds(y_t, x_t):
    return (math.ceil(1.0 / 100.0 * y_t), y_t // 4, math.ceil(5.0 / 100.0 * x_t), x_t // 4)


class SyncXY64:
    """SyncXY{Float64} + vsync: s_y is the argmax of beta_y as the PREVIOUS call left it (FrameSynchronisation.jl:66)"""

    def __init__(self, y_t, x_t):
        self.y_t, self.x_t = y_t, x_t
        self.wmin_y, self.wmax_y, self.wmin_x, self.wmax_x = bounds(y_t, x_t)
        self.h = taps()
        self.reset()

    def reset(self):
        self.beta_x = np.zeros((1 + self.wmax_x - self.wmin_x, self.x_t), order="F")
        self.beta_y = np.zeros((1 + self.wmax_y - self.wmin_y, self.y_t), order="F")

    def vsync(self, img):
        a = np.asarray(img, np.float64)
        cv, ch = col_sums(a), row_sums(a)
        self.beta_x = fill_beta(fir(self.h, cv), self.x_t, self.wmin_x, self.wmax_x)
        s_y = argmax_col(self.beta_y)
        self.beta_y = fill_beta(fir(self.h, ch), self.y_t, self.wmin_y, self.wmax_y)
        return s_y, argmax_col(self.beta_x)


# ---- demodulation, spectra --------------------------------------------------------------------------------------------
def abs2(z):
    z = np.asarray(z, np.complex128)
    return z.real * z.real + z.imag * z.imag


def fm_product(z):
    """s[n+1]*conj(s[n]) without FMA, as (re, im)"""
    z = np.asarray(z, np.complex128)
    a, b = z.real[1:], z.imag[1:]
    c, d = z.real[:-1], -z.imag[:-1]
    return a * c - b * d, a * d + b * c


def autocorr(x, Fs, minDelay, maxDelay, log_scale=True):
    """calculate_autocorrelation in complex128 numpy FFTs (the tolerance reference of autocorr_f64)"""
    index_min = 1 + int(np.round(minDelay * Fs))
    index_max = int(np.round(maxDelay * Fs))
    n = min(2 * index_max, len(x))
    X = np.fft.fft(np.asarray(x[:n], np.float64).astype(np.complex128))
    c = np.fft.ifft(X.real * X.real + X.imag * X.imag)[index_min - 1: index_max]
    p = c.real * c.real + c.imag * c.imag
    return 10.0 * np.log10(p) if log_scale else p


def spectrum(sig, N, log_scale=True):
    X = np.fft.fftshift(np.fft.fft(np.asarray(sig[:N]).astype(np.complex128)))
    p = X.real * X.real + X.imag * X.imag
    return 10.0 * np.log10(p) if log_scale else p
