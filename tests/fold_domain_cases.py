"""The domain the fold family's tests run over: the parts of what the headers accept (SAMPLING and REFUSALS of
include/tempest_hip_fold.h, _cfold.h, _cstack.h, _ctrack.h, _gram.h) that the six captures of tests/test_cstack_gpu.py never reach.

Plain module: the table, the data and pure numpy functions, no fixtures.  test_fold_domain_host.py recomputes every column from the
references' own coordinates, so a case that misses its edge fails on the CPU instead of passing silently on the GPU;
test_fold_domain_gpu.py runs every case through the eight device entry points.

n = ceil(t0 + F T).  `end`: t0 + F T == n exactly in f64, the last call the refusal rule lets through.  W = ceil(128 T / P) + 3 is the
span of a tile line; the envelope fold stages it up to TSDR_FOLD_STAGE_MAX = 240, the coherent entry points up to
TSDR_CFOLD_STAGE_MAX = 120 (`tile`), and load both taps themselves above that (`direct`).  low / high: pixels, counted over all frames,
whose u_f(m) lies below 0 / above n - 1 before the buffer clamp.  d0 / d1: pixels whose weight of the right tap is exactly 0 / exactly 1.

    P1    1 x 1,   T 2       the smallest of everything: P = 1, T = 2, n = 6
    ROW   1 x 300            one line: 63 idle lanes in every wavefront; both clamps bind in the staged kernels
    COL   300 x 1            one pixel per line: five line tiles, each one pixel wide
    UPS   20 x 140, T 310.5  nine pixels per sample: five pixels clamp at either end; staged by every entry point
    UPD   20 x 140, T 2660.5 W 125: staged by the envelope fold, direct for the coherent family, with both clamps binding
    INT   20 x 140, T = P    every position on the integer grid: d == 0 everywhere, and the last pixel sits at n - 1 with d == 1
    T64   64 x 128           exactly one tile, no ragged edge
    T65   65 x 129           a second line tile of one line, a second pixel tile of one pixel
    D65   65 x 129, W 388    the same ragged edges in the direct kernels
    NAR   8 x 5              x_t below the 16 pixels of a direct tile
    LONG  8 x 16, F 1500     the f32 sum over 1500 terms against (F + 8) ulp; refused by the Gram matrix (F > 64)
    G32   8 x 16, F 32       fills the Gram kernel's 32-row block exactly
    FAR   70 x 150, t0 2^24 + 1234.625, sc8   the frame origin above 2^24 samples: an index or origin that passes through f32 shows here

The envelope fold's direct kernel cannot clamp: it runs above about 1.85 samples per pixel, where the first pixel of a frame sits at
(T/P - 1) / 2 > 0 past the frame's origin and the last one as far before its end, and with t0 >= 0 and t0 + F T <= n every u then lies
inside (0, n - 1).  That is a property of the domain, not an omission of the table; the coherent direct kernels (above 0.91 samples per
pixel) do clamp, in UPD.

Input: (standard_normal + i standard_normal + 0.5) as ComplexF32 from a generator seeded by the case's name; these tests need no
picture.  FAR is raw sc8, int8 pairs in [-127, 127] at scale 1/128 (33 MB instead of 134 MB of ComplexF32), and only the window its
frames touch is ever expanded.

The test track is tests/test_ctrack_gpu.py's, a_f = 0.37 + f kappa_true + 0.01 f^2, b_f = 0.02 f - 0.03.  For LONG a_f is reduced mod 1
(its f^2 term otherwise reaches 22 500 turns): whole turns of a_f are within the contract but are not what this case is about."""
import functools
import math

import numpy as np

F32, C64 = np.float32, np.complex64
FOLD_STAGE_MAX, CFOLD_STAGE_MAX = 240, 120     # TSDR_FOLD_STAGE_MAX, TSDR_CFOLD_STAGE_MAX
GRAM_MAX_FRAMES = 64                           # TSDR_GRAM_MAX_FRAMES
KAPPA_TRUE = (1000.0 / 60.0) % 1.0
FAR_T0 = 2.0 ** 24 + 1234.625
SC8_SCALE = 1.0 / 128.0

_COLS = ("y", "x", "T", "F", "t0", "n", "end", "W", "envelope", "coherent", "low", "high", "d0", "d1")
_ROWS = {
    "P1": (1, 1, 2.0, 3, 0.0, 6, True, 259, "direct", "direct", 0, 0, 0, 0),
    "ROW": (1, 300, 250.0, 4, 0.0, 1000, True, 110, "tile", "tile", 1, 1, 1, 1),
    "COL": (300, 1, 250.0, 4, 0.0, 1000, True, 110, "tile", "tile", 1, 1, 1, 1),
    "UPS": (20, 140, 310.5, 2, 0.0, 621, True, 18, "tile", "tile", 5, 5, 5, 5),
    "UPD": (20, 140, 2660.5, 2, 0.0, 5321, True, 125, "tile", "direct", 1, 1, 1, 1),
    "INT": (20, 140, 2800.0, 3, 0.0, 8400, True, 131, "tile", "direct", 0, 0, 8399, 1),
    "T64": (64, 128, 7000.5, 2, 0.0, 14001, True, 113, "tile", "tile", 1, 1, 1, 1),
    "T65": (65, 129, 7100.25, 4, 0.0, 28401, True, 112, "tile", "tile", 1, 1, 1, 1),
    "D65": (65, 129, 25155.5, 2, 0.0, 50311, True, 388, "direct", "direct", 0, 0, 0, 0),
    "NAR": (8, 5, 977.25, 4, 0.0, 3909, True, 3131, "direct", "direct", 0, 0, 0, 0),
    "LONG": (8, 16, 300.25, 1500, 0.75, 450376, False, 304, "direct", "direct", 0, 0, 0, 0),
    "G32": (8, 16, 300.25, 32, 0.75, 9609, False, 304, "direct", "direct", 0, 0, 0, 0),
    "FAR": (70, 150, 1207.73, 7, FAR_T0, 16786905, False, 18, "tile", "tile", 0, 2, 0, 2),
}
CASES = {name: dict(zip(_COLS, row), name=name, fmt="sc8" if name == "FAR" else "cf32") for name, row in _ROWS.items()}
ALL = list(CASES)
FORMAT_CASES = ["UPS", "INT"]                  # also run in sc16, sc8 and uc8: format invariance under binding clamps
FMT_CODE = {"cf32": 0, "sc16": 1, "sc8": 2, "uc8": 3}
# a code the quantised data never takes, for the sample that pads an odd 8-bit buffer to whole words: the most negative value of
# either format, below everything the data holds
PAD_CODE = {"sc8": -128, "uc8": 0}


# ---------------------------------------------------------------- the headers' rules, restated
def n_of(c):
    return int(math.ceil(c["t0"] + c["F"] * c["T"]))


def span(c):
    """W = ceil(128 T / P) + 3, in the f64 operations of the host geometry"""
    return int(math.ceil(128.0 * (c["T"] / (float(c["y"]) * float(c["x"])))) + 3.0)


def route(c, stage_max):
    return "tile" if span(c) <= stage_max else "direct"


def accepted(c, n=None, T=None):
    """REFUSALS, the part about the geometry: T >= 2, t0 >= 0, t0 + F T <= n in f64, n in [2, 2^31), 0 < P < 2^31"""
    n = c["n"] if n is None else n
    T = c["T"] if T is None else T
    return (c["y"] > 0 and c["x"] > 0 and c["y"] * c["x"] < 2 ** 31 and 2 <= n < 2 ** 31 and c["F"] >= 0 and math.isfinite(T)
            and math.isfinite(c["t0"]) and T >= 2.0 and c["t0"] >= 0.0 and c["t0"] + float(c["F"]) * T <= float(n))


def coordinates(c, f, t0=None, n=None):
    """(u before the clamps, k, d) of frame f, float64[P] / int64[P] / float64[P]: SAMPLING as the references evaluate it
    (fold_ref.fold_mean, cfold_ref.zfold_mean, ctrack_ref.frame_samples)"""
    t0 = c["t0"] if t0 is None else t0
    n = c["n"] if n is None else n
    P, T = c["y"] * c["x"], c["T"]
    raw = (t0 + f * T) + ((np.arange(P, dtype=np.float64) + 0.5) * (T / P) - 0.5)
    u = np.clip(raw, 0.0, n - 1.0)
    k = np.minimum(np.floor(u), n - 2.0).astype(np.int64)
    return raw, k, u - k


def counts(c):
    """(low, high, d0, d1) over all frames, and the largest sample index a tap reads"""
    low = high = d0 = d1 = 0
    last = -1
    for f in range(c["F"]):
        raw, k, d = coordinates(c, f)
        low += int(np.count_nonzero(raw < 0.0))
        high += int(np.count_nonzero(raw > c["n"] - 1.0))
        d0 += int(np.count_nonzero(d == 0.0))
        d1 += int(np.count_nonzero(d == 1.0))
        last = max(last, int(k.max()) + 1)
    return (low, high, d0, d1), last


# ---------------------------------------------------------------- the window of a far case
def window(c):
    """(w0, t0 - w0): the references add t0 + f T and the in-frame part at the buffer's magnitude, which costs about 2^-28 samples at
    2^24; on z[w0:], w0 = floor(t0) - 2, they run at the magnitude of the frames.  The subtraction is exact, and the clamp at n - 1 is
    the whole buffer's because the window runs to the buffer's end.  w0 = 0 where t0 < 2."""
    w0 = max(int(math.floor(c["t0"])) - 2, 0)
    return w0, c["t0"] - w0


def windowed(c):
    """the case on its window: t0 and n counted from w0"""
    w0, t0 = window(c)
    return dict(c, t0=t0, n=c["n"] - w0)


# ---------------------------------------------------------------- data
def seed(name):
    return int.from_bytes(name.encode(), "big")


@functools.lru_cache(maxsize=None)
def raw_sc8(name):
    """FAR's buffer: int8[2 n], I and Q interleaved, in [-127, 127]"""
    c = CASES[name]
    raw = np.random.default_rng(seed(name)).integers(-127, 128, size=2 * c["n"], dtype=np.int8)
    raw.setflags(write=False)
    return raw


def expand(raw, fmt, scale):
    """the integer formats' conversion rule on the host: (f32(code) - offset) * f32(scale), the product the one rounding"""
    off = F32(127.5) if fmt == "uc8" else F32(0.0)
    return np.ascontiguousarray(((np.asarray(raw).astype(F32) - off) * F32(scale)).view(C64))


@functools.lru_cache(maxsize=None)
def samples(name):
    """complex64: the case's converted samples from its window on (the whole buffer wherever t0 < 2)"""
    c = CASES[name]
    if c["fmt"] == "sc8":
        z = expand(raw_sc8(name)[2 * window(c)[0]:], "sc8", SC8_SCALE)
    else:
        rng = np.random.default_rng(seed(name))
        z = (rng.standard_normal(c["n"]) + 1j * rng.standard_normal(c["n"]) + 0.5).astype(C64)[window(c)[0]:]
    z.setflags(write=False)
    return z


def quantise(z, fmt):
    """(raw integer components, scale, expanded complex64) of ComplexF32 samples in an integer format: the rule of
    tests/test_cstack_gpu.py's _quantised, for any number of samples"""
    z = np.ascontiguousarray(z, C64)
    full = {"sc16": 32767.0, "sc8": 127.0, "uc8": 127.0}[fmt]
    scale = float(np.abs(z.view(F32)).max()) / full * 1.01
    comp = np.round(z.view(F32).astype(np.float64) / scale)
    if fmt == "uc8":
        comp = np.floor(comp + 127.5)
    raw = comp.astype({"sc16": np.int16, "sc8": np.int8, "uc8": np.uint8}[fmt])
    return raw, scale, expand(raw, fmt, scale)


def padded(raw, fmt):
    """an integer buffer as whole 32-bit words for a guarded arena: an odd number of 8-bit samples gets one sample of PAD_CODE"""
    raw = np.ascontiguousarray(raw)
    if raw.nbytes % 4 == 0:
        return raw
    assert raw.nbytes % 4 == 2 and fmt in PAD_CODE
    return np.concatenate([raw, np.full(2, PAD_CODE[fmt], raw.dtype)])


def track(c, F=None):
    """the test track, float64 (F, 2)"""
    f = np.arange(c["F"] if F is None else F, dtype=np.float64)
    a = 0.37 + f * KAPPA_TRUE + 0.01 * f * f
    if c["name"] == "LONG":
        a = a - np.floor(a)
    return np.ascontiguousarray(np.stack([a, 0.02 * f - 0.03], axis=1))


def far_term(c, amax):
    """what a windowed reference adds to every per-term bound: the largest slope, 2 amax per sample, times the n 2^-52 samples by
    which the windowed and the whole-buffer coordinates may differ (test_fold_domain_host.py); 0 where the window is the buffer"""
    return 2.0 * float(amax) * c["n"] * 2.0 ** -52 if window(c)[0] else 0.0
