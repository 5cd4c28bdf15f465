"""The reference side of the SyncXY domain tests (sync_cases.py), on the CPU.

The oracle (oracle/tempest_oracle.c) is itself a restatement, and zero bands, NaN / Inf pixels, subnormal and overflowing
beta are inputs it had not seen.  So (1) an independent numpy restatement -- sequential Float32 operations in the documented
orders, the FIR's fused multiply-adds rounded once -- must give the oracle's beta_x / beta_y bit for bit (NaN == NaN) and the
same columns, for every family at three small sizes; (2) every family's condition must hold for the oracle at every size,
and for the Float64 restatement (f64_ref.py) at the Float64 sizes: a case that does not exercise its edge fails here.
"""
import numpy as np
import pytest

import f64_ref as R
import oracle_lib as O
import sync_cases as K

F32 = np.float32


# ---- independent Float32 restatement, vectorised over columns / centres -------------------------------------------------
def fma32(a, b, c):
    """RN_f32(a * b + c) for Float32 arrays: the product is exact in Float64, the sum is rounded to odd there (TwoSum gives
    the error's sign), and rounding that to Float32 is then the single correct rounding"""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64).copy()
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
        up = (err > 0) == (s > 0)   # the exact value lies further from zero than s
        bits[fix & up] += 1
        bits[fix & ~up] -= 1
        return bits.view(np.float64).astype(F32)


def col_sums32(img):
    """sum(image; dims=1): 64-row blocks accumulated top to bottom from 0.0f, block sums added in order"""
    tot = None
    for r0 in range(0, img.shape[0], 64):
        acc = np.zeros(img.shape[1], F32)
        for r in range(r0, min(r0 + 64, img.shape[0])):
            acc = acc + img[r, :]
        tot = acc if tot is None else tot + acc
    return tot


def row_sums32(img):
    """sum(image; dims=2): strictly left to right from 0.0f + 0.0f"""
    acc = np.zeros(img.shape[0], F32)
    for c in range(img.shape[1]):
        acc = acc + img[:, c]
    return acc


def taps32():
    return np.array(R.taps(), np.float64).astype(F32)


def fir32(h, x):
    """DSP.jl filt(h, x): y[i] = fma(x[i],h0, fma(x[i-1],h1, fma(x[i-2],h2, fma(x[i-3],h3, h4*x[i-4])))), x[<0] = 0"""
    n = x.size
    xp = np.concatenate([np.zeros(4, F32), x])
    g = lambda j: xp[4 - j: 4 - j + n]  # noqa: E731   x[i - j]
    with np.errstate(all="ignore"):
        s = h[4] * g(4)
    for j in (3, 2, 1, 0):
        s = fma32(g(j), np.full(n, h[j], F32), s)
    return s


def sum64_32(x):
    p = np.zeros(64, F32)
    with np.errstate(all="ignore"):
        for i0 in range(0, x.size, 64):
            seg = x[i0:i0 + 64]
            p[:seg.size] = p[:seg.size] + seg
        off = 32
        while off:
            p[:off] = p[:off] + p[off:2 * off]
            off >>= 1
    return p[0]


def fill_beta32(cv, n, w_min, w_max):
    c = np.arange(n)
    with np.errstate(all="ignore"):
        S = sum64_32(cv)
        acc = np.zeros(n, F32)
        for k in range(-(w_min - 1), w_min):
            acc = acc + cv[(c + k) % n]
        s = F32(2.0) * acc
        beta = np.empty((w_max - w_min + 1, n), F32, order="F")
        for cnt, w in enumerate(range(w_min, w_max + 1)):
            s = s + F32(2.0) * cv[(c - w) % n]
            s = s + F32(2.0) * cv[(c + w) % n]
            v = (S - s) / F32(2 * (n - w)) + s / F32(2 * w)
            beta[cnt, :] = v * v
    assert beta.dtype == F32
    return beta


def restated_vsync(img):
    y_t, x_t = img.shape
    wy0, wy1, wx0, wx1 = K.bounds(y_t, x_t)
    h = taps32()
    with np.errstate(all="ignore"):
        bx = fill_beta32(fir32(h, col_sums32(img)), x_t, wx0, wx1)
        by = fill_beta32(fir32(h, row_sums32(img)), y_t, wy0, wy1)
    return bx, by


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    u = np.uint32 if a.dtype == F32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def test_fma32_rounds_once():
    e = 2.0 ** -23
    a, b, c = F32(32.0 * (1.0 + e)), F32(1.0 - e), F32(2.0 ** 29 + 64.0)
    # a * b + c = 2^29 + 64 + 32 - 2^-41: just below the midpoint of 2^29 + 64 and 2^29 + 128.  Rounded to Float64 first it
    # IS the midpoint, which then ties to even, 2^29 + 128: the double rounding this emulation must not have
    assert float(a) * float(b) + float(c) == 2.0 ** 29 + 96.0
    assert fma32([a], [b], [c])[0] == F32(2.0 ** 29 + 64.0)
    assert fma32([-a], [b], [-c])[0] == F32(-(2.0 ** 29 + 64.0))
    assert fma32([F32(1 + 2.0 ** -12)], [F32(1 + 2.0 ** -12)], [F32(-(2.0 ** -11))])[0] == F32(1.0)   # an exact tie: to even
    x = fma32([F32(np.inf), F32(1.0), F32(0.0)], [F32(1.0), F32(np.nan), F32(5.0)], [F32(-np.inf), F32(1.0), F32(0.0)])
    assert np.isnan(x[0]) and np.isnan(x[1]) and x[2] == 0.0


@pytest.mark.parametrize("y_t,x_t", K.RESTATED_SIZES)
def test_oracle_equals_independent_restatement(y_t, x_t):
    o = O.SyncXY(y_t, x_t)
    assert (o.wmin_y, o.wmax_y, o.wmin_x, o.wmax_x) == K.bounds(y_t, x_t)
    prev_by = np.zeros((1 + o.wmax_y - o.wmin_y, y_t), F32, order="F")
    for fam in K.families(y_t, x_t) + ["noise"]:
        img = K.image(fam, y_t, x_t)
        s_y, s_x = o.vsync(img)
        bx, by = restated_vsync(img)
        assert same_bits(o.beta("x"), bx), f"{fam}: beta_x"
        assert same_bits(o.beta("y"), by), f"{fam}: beta_y"
        assert (s_y, s_x) == (K.argmax_col(prev_by), K.argmax_col(bx)), fam   # s_y: the beta_y the call before left (:66)
        prev_by = by


def _check_conditions(y_t, x_t, vsync, beta, project, dtype, min_normal, bar):
    fams = K.families(y_t, x_t)
    got = {}
    for fam in fams + ["noise"]:
        img = K.image(fam, y_t, x_t, dtype)
        s_y, s_x = vsync(img)
        if fam == "zero-band":
            K.cond_zero_band(y_t, x_t, *project(img))
        got[fam] = (s_y, s_x, beta("x"), beta("y"))
        if fam == "subnormal":
            K.cond_subnormal(got[fam][2], got[fam][3], min_normal)
        elif fam == "near-overflow":
            K.cond_near_overflow(y_t, x_t, got[fam][2], got[fam][3], bar)
        elif fam == "tie":
            K.cond_tie(y_t, x_t, got[fam][2], got[fam][3])
        elif fam in ("one-nan", "plus-minus-inf"):
            assert np.isnan(got[fam][2]).all() and np.isnan(got[fam][3]).all()   # Sigma is NaN: the first column wins
        elif fam == "one-inf":
            # NaN where the window holds the Inf, +Inf elsewhere: the first NaN is neither in column 1 nor where the pixel is
            for b, n in ((got[fam][2], x_t), (got[fam][3], y_t)):
                if n >= 64:   # (on a short axis the five filtered Inf and the widths reach every centre)
                    assert np.isnan(b).any() and np.isposinf(b).any()
                    assert 1 < K.argmax_col(b) < n // 2 + 1
    # overflow: s_x = 1 at once, s_y = 1 one call later
    i = fams.index("overflow")
    K.cond_overflow(got["overflow"][2], got["overflow"][3], got["overflow"][1], got[fams[i + 1]][0])


@pytest.mark.parametrize("y_t,x_t", K.SIZES)
def test_conditions_hold_for_the_oracle(y_t, x_t):
    o = O.SyncXY(y_t, x_t)
    _check_conditions(y_t, x_t, o.vsync, o.beta, o.project, F32, K.F32_MIN_NORMAL, 1e35)


class _Ref64(R.SyncXY64):
    def beta(self, which):
        return self.beta_x if which == "x" else self.beta_y

    def project(self, img):
        a = np.asarray(img, np.float64)
        return R.fir(self.h, R.col_sums(a)), R.fir(self.h, R.row_sums(a))


@pytest.mark.parametrize("y_t,x_t", K.SIZES_F64)
def test_conditions_hold_for_the_f64_restatement(y_t, x_t):
    with np.errstate(all="ignore"):
        r = _Ref64(y_t, x_t)
        _check_conditions(y_t, x_t, r.vsync, r.beta, r.project, np.float64, K.F64_MIN_NORMAL, 1e305)


def test_fill_beta_and_circshift_cases_are_well_formed():
    for n, w_min, w_max in K.FILL_BETA_CASES:
        assert 2 <= n <= 16384 and 1 <= w_min <= w_max < n
        for kind in K.FILL_BETA_INPUTS:
            assert K.fill_beta_input(kind, n, w_min).shape == (n,)
    cv = K.fill_beta_input("zero-band", 65, 3)
    assert (K.blank_sum_at_wmin(cv, 3) == 0).any() and np.isnan(K.fill_beta_input("one-nan", 65, 3)).sum() == 1
    for h, w in K.CIRCSHIFT_SIZES:
        for sy, sx in K.circshift_shifts(h, w):
            assert -2 ** 31 <= sy < 2 ** 31 and -2 ** 31 <= sx < 2 ** 31
        img = np.asfortranarray(np.arange(h * w, dtype=F32).reshape(h, w))
        for sy, sx in K.circshift_shifts(h, w):   # the oracle against numpy, whatever the shift's size
            assert np.array_equal(O.circshift_neg(img, sy, sx), np.roll(img, (-sy, -sx), axis=(0, 1)))
