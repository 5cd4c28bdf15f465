"""The domain the SyncXY tests run over: image sizes, image families and the condition each family has to meet.

Plain module (no fixtures).  Every condition takes the ORACLE's outputs (for the Float64 twin: the float64 restatement's) and asserts
that the image really exercises the edge it is there for, so a case that misses its edge fails on the CPU instead of
passing silently on the GPU.  test_sync_domain_host.py runs the conditions; test_sync_domain_gpu.py runs the kernels.

Sizes (y_t, x_t) and the branch of csrc/sync.hip each one is there for:
  (8, 20)      the minimum tsdr_sync_create accepts: W_y = 2, W_x = 5 (fewer widths than k_beta has wavefronts, most
               shares are empty), one partial 64-row block, one partial 100-column chunk of k_proj
  (9, 21), (63, 99)   odd, just below a full block / chunk
  (64, 100)    exactly one row block, exactly one full chunk
  (65, 101)    one row and one column past a full block / chunk
  (100, 125)   the second chunk is exactly one 25-column LDS sub-batch
  (128, 799)   one column short of an 800-column super-round
  (129, 801)   a second super-round that holds one column
  (200, 1337)  W_x = 268: a 4-wavefront share of 67 widths = a second reciprocal batch of 3
  (70, 2600)   W_x = 521: the same edge for 8 wavefronts (share 66, second batch of 2)
  (6000, 24)   maximum height (k_beta's LDS request within 3 KiB of 64 KiB)
  (8, 6000)    maximum width
"""
import math

import numpy as np

SIZES = [(8, 20), (9, 21), (63, 99), (64, 100), (65, 101), (100, 125), (128, 799), (129, 801), (200, 1337), (70, 2600),
         (6000, 24), (8, 6000)]
SIZES_F64 = [(8, 20), (65, 101), (129, 801), (200, 1337), (6000, 24)]
RESTATED_SIZES = [(8, 20), (9, 21), (65, 101)]   # where the independent numpy restatement checks the oracle

F32_MIN_NORMAL = 1.17e-38   # the issue's figure for the smallest normal Float32 (1.17549435e-38)
F64_MIN_NORMAL = 2.2250738585072014e-308


def bounds(n_y, n_x):
    """(wmin_y, wmax_y, wmin_x, wmax_x) of SyncXY (FrameSynchronisation.jl:25-48)"""
    return (math.ceil(1.0 / 100.0 * n_y), n_y // 4, math.ceil(5.0 / 100.0 * n_x), n_x // 4)


# ---- image families ------------------------------------------------------------------------------------------------
def _seed(name, y_t, x_t):
    return [sum(ord(ch) * (i + 1) for i, ch in enumerate(name)), y_t, x_t]


def _noise(name, y_t, x_t):
    """0.3 + 0.02 U in float64 (rounded by the caller)"""
    return 0.3 + 0.02 * np.random.default_rng(_seed(name, y_t, x_t)).random((y_t, x_t))


def zero_band(n, w_min):
    """[a, b): the block of an axis of length n that the zero-band family sets to 0.0.

    The filtered projection is exactly 0 from a + 4 on (the FIR is causal, 5 taps), so a centre's running sum s is exactly 0
    at the smallest width when [c - w_min, c + w_min] lies in [a + 4, b): the band is 2 w_min + 5 + 2 wide (three such
    centres) where the axis is long enough for that to stay below n / 2, else as wide as n / 2 allows (at y_t = 8, 9 a
    band narrower than n / 2 cannot hold a zero s: band_holds_zero_s)."""
    width = min(2 * w_min + 7, (n - 1) // 2)
    a = n // 3
    while a % 64 == 0 or (a + width) % 64 == 0:
        a += 1
    assert a + width < n
    return a, a + width


def band_holds_zero_s(n, w_min):
    a, b = zero_band(n, w_min)
    return b - a >= 2 * w_min + 5


TIE_TILE = (16, 32)   # rows x columns of the tie family's periodic block
TIE_MIN_AXIS = 96     # shortest axis on which that block ties across 64-centre blocks


def tie_axis(n):
    """whether an axis of length n can tie across 64-centre blocks.

    Centres c and c + P (P the tile's period) have bit-equal beta at every width whose window [c - w, c + w] neither wraps
    round the axis nor touches the FIR's start-up (the first four outputs); the bright band is narrow, so that the maximum
    sits at a small width.  That needs a few periods on both sides of a block boundary: from 96 on.  (At y_t = 65 and 70
    the second block holds 1 and 6 centres, all of whose windows wrap: no tie there, whatever the image.)"""
    return n >= TIE_MIN_AXIS


def has_tie(y_t, x_t):
    return tie_axis(y_t) or tie_axis(x_t)


def _tie_image(y_t, x_t):
    wy, _, wx, _ = bounds(y_t, x_t)
    py, px = TIE_TILE
    blk = 0.3 + 0.02 * np.random.default_rng(_seed("tie", py, px)).random((py, px))
    a = np.tile(blk, (-(-y_t // py), -(-x_t // px)))[:y_t, :x_t]
    # the bright bands, in whole periods only: round the seam where the axis wraps the pattern is broken, and a window there
    # must see less brightness (a smaller beta) than the periodic ones, not more
    for c0 in range(0, x_t - px + 1, px):
        a[:, c0 + 4:c0 + 4 + min(2 * wx + 1, px // 2)] = 1.0
    for r0 in range(0, y_t - py + 1, py):
        a[r0 + 4:r0 + 4 + min(2 * wy + 1, py // 2), :] = 1.0
    return a


# Scales of the three scaled families.  With m = 0.31 * (length of the summed axis) * scale the mean of a projection, a
# centre of the noise image has s = 2 (2w + 1) m and Sigma = n m, so v = m ((n - 4w - 2) / (2 (n - w)) + (2w + 1) / w), largest
# at w_min.  The axis with the larger beta = v^2 is put at the target; the conditions below then check the oracle at every size.
_TARGET = {np.float32: {"subnormal": 6e-39, "near-overflow": 1e38},    # of [1.4e-45, 1.17e-38) and (1e35, 3.4e38)
           np.float64: {"subnormal": 1e-308, "near-overflow": 5e307}}  # of [4.9e-324, 2.2e-308) and (1e305, 1.8e308)


def _beta_estimate(n, w_min, summed):
    m = 0.31 * summed
    return (m * ((n - 4 * w_min - 2) / (2.0 * (n - w_min)) + (2 * w_min + 1) / w_min)) ** 2


def family_scale(name, y_t, x_t, dtype=np.float32):
    dtype = np.dtype(dtype).type
    if name == "overflow":
        # every beta +Inf while every sum stays finite: the smaller projection mean is 32 sqrt(realmax), v is 2.4 to 3.5 times
        # that, and the largest Sigma (6000 values of 750 times that mean) is still below realmax
        return 32.0 * math.sqrt(float(np.finfo(dtype).max)) / (0.31 * min(y_t, x_t))
    wy, _, wx, _ = bounds(y_t, x_t)
    return math.sqrt(_TARGET[dtype][name] / max(_beta_estimate(x_t, wx, y_t), _beta_estimate(y_t, wy, x_t)))


def both_axes_near_overflow(y_t, x_t):
    """The two axes' beta differ by about (x_t / y_t)^2 (times up to 2).  Between the bar and the target there is room for a
    factor 1000 (Float64: 500): where the sizes are closer than that, BOTH axes have to be near overflow, else the axis
    with the larger beta."""
    r = max(y_t, x_t) / min(y_t, x_t)
    return r * r <= 100.0


FAMILIES = ["noise", "zero-band", "negative", "subnormal", "near-overflow", "overflow", "one-nan", "one-inf",
            "plus-minus-inf", "tie"]


def families(y_t, x_t):
    """the families that exist at this size, in the fixed order the GPU tests call vsync in"""
    return [f for f in FAMILIES if f != "tie" or has_tie(y_t, x_t)]


def image(name, y_t, x_t, dtype=np.float32):
    """the image of a family: Fortran order, float32 (or float64 with scales of its own)"""
    wy, _, wx, _ = bounds(y_t, x_t)
    if name == "tie":
        a = _tie_image(y_t, x_t)
    else:
        a = _noise(name, y_t, x_t)
    if name == "negative":
        a = a - 0.31
    elif name == "zero-band":
        c0, c1 = zero_band(x_t, wx)
        r0, r1 = zero_band(y_t, wy)
        a[:, c0:c1] = 0.0
        a[r0:r1, :] = 0.0
    elif name in ("subnormal", "near-overflow", "overflow"):
        a = a * family_scale(name, y_t, x_t, dtype)
    elif name == "one-nan":
        a[y_t // 2, x_t // 2] = np.nan
    elif name == "one-inf":
        a[y_t // 2, x_t // 2] = np.inf
    elif name == "plus-minus-inf":
        a[y_t // 2, x_t // 2] = np.inf
        a[y_t // 2 - 2, x_t // 2 + 3] = -np.inf
    return np.asfortranarray(a.astype(dtype))


# ---- conditions ------------------------------------------------------------------------------------------------------
def argmax_col(beta):
    """findmax(beta)[2][2]: 1-based column of the first maximum in column-major order, NaN maximal"""
    f = np.asarray(beta).ravel(order="F")
    nan = np.flatnonzero(np.isnan(f))
    i = int(nan[0]) if nan.size else int(np.argmax(f))
    return i // beta.shape[0] + 1


def blank_sum_at_wmin(cv, w_min):
    """s of every centre at the smallest width, from a filtered projection: 2 * sum(cv[c - w_min .. c + w_min]) -- whether
    it is exactly 0 does not depend on the order of the adds when no entry of the window is negative"""
    cv = np.asarray(cv, np.float64)
    assert not (cv < 0).any()
    n = cv.size
    idx = (np.arange(n)[:, None] + np.arange(-w_min, w_min + 1)[None, :]) % n
    return 2.0 * cv[idx].sum(axis=1)


def cond_zero_band(y_t, x_t, cv_f, ch_f):
    """per axis that can hold one: a centre whose s is exactly 0 at the smallest width and, in the same 64-centre block,
    one whose s is not (one lane of a k_beta wavefront re-runs with IEEE divisions, its neighbours do not)"""
    wy, _, wx, _ = bounds(y_t, x_t)
    checked = 0
    for n, w_min, p in ((x_t, wx, cv_f), (y_t, wy, ch_f)):
        if not band_holds_zero_s(n, w_min):
            continue
        z = blank_sum_at_wmin(p, w_min) == 0.0
        blocks = [b for b in range(0, n, 64) if z[b:b + 64].any() and not z[b:b + 64].all()]
        assert blocks, f"zero-band {y_t}x{x_t}: no 64-centre block of the axis of length {n} mixes s == 0 and s != 0"
        checked += 1
    assert checked, "zero-band: neither axis can hold a zero s"
    assert band_holds_zero_s(x_t, wx), "every accepted width (>= 20) can"


def cond_subnormal(beta_x, beta_y, min_normal=F32_MIN_NORMAL):
    for b in (beta_x, beta_y):
        assert 0.0 < float(np.max(b)) < min_normal, float(np.max(b))


def cond_near_overflow(y_t, x_t, beta_x, beta_y, bar=1e35):
    mx, my = float(np.max(beta_x)), float(np.max(beta_y))
    assert np.isfinite(mx) and np.isfinite(my), (mx, my)
    if both_axes_near_overflow(y_t, x_t):
        assert mx > bar and my > bar, (mx, my)
    else:
        assert max(mx, my) > bar, (mx, my)


def cond_overflow(beta_x, beta_y, s_x, next_s_y):
    for b in (beta_x, beta_y):
        assert np.all(np.isposinf(b))
    assert s_x == 1 and next_s_y == 1


def tied_blocks(beta):
    """64-centre blocks that hold a column where the maximum of beta is attained bit for bit"""
    m = np.max(beta)
    assert np.isfinite(m)
    cols = np.flatnonzero((np.asarray(beta) == m).any(axis=0))
    return sorted({int(c) // 64 for c in cols})


def cond_tie(y_t, x_t, beta_x, beta_y):
    checked = 0
    for n, b, what in ((x_t, beta_x, "x"), (y_t, beta_y, "y")):
        if tie_axis(n):
            blocks = tied_blocks(b)
            assert len(blocks) >= 2, f"tie {y_t}x{x_t}: the maximum of beta_{what} lies in block(s) {blocks} only"
            checked += 1
    assert checked


# ---- fill_beta and circshift_neg on their own -------------------------------------------------------------------------
FILL_BETA_CASES = [(2, 1, 1), (5, 4, 4), (63, 1, 62), (64, 1, 63), (65, 3, 16), (6000, 300, 1500), (16384, 164, 4096)]
FILL_BETA_MAX_N = 16384   # Float32: c_v is held in 64 KiB of LDS
FILL_BETA_INPUTS = ["noise", "zero-band", "one-nan"]


def fill_beta_input(kind, n, w_min, dtype=np.float32):
    """a filtered projection of length n: 600 U; with a block of exact zeros wide enough for a zero s where n allows; with one NaN"""
    cv = 600.0 * np.random.default_rng(_seed(kind, n, w_min)).random(n)
    if kind == "zero-band":
        a, b = zero_band(n, w_min) if n >= 8 else (0, 1)
        cv[a:b] = 0.0
    elif kind == "one-nan":
        cv[n // 2] = np.nan
    return cv.astype(dtype)


CIRCSHIFT_SIZES = [(8, 20), (65, 101), (600, 800)]


def circshift_shifts(h, w):
    return [(0, 0), (1, 1), (h - 1, w - 1), (h, w), (h + 1, w + 1), (-1, -1), (-h - 3, 5), (2 ** 31 - 1, -2 ** 31 + 1)]
