"""Inventory of the capped, looping launches of csrc/ and the cases that drive each one past its cap.  Data and small builders;
no test lives here (test_grid_cap_host.py checks the table against the sources, test_grid_cap_gpu.py runs the cases).

common.h:stream_blocks caps a streaming grid at cu_count * 8 workgroups of 256 threads, `cap(cu)` work items: with more work than
that every kernel below walks a grid-stride loop, and everything that exists only on its second trip -- the stride arithmetic,
state kept in registers from trip to trip, the tail that workgroup 0 alone handles -- runs only then.  fft_plan.h:plan_rows caps
the whole-row FFT launches at a few workgroups per CU, each walking tiles of rows.

SITES has one entry per launch site:
    file, token, expr   where it is: the source file, the launch's name argument (or, where the grid is formed in a statement
                        of its own, that statement's left-hand side) and the work-item expression handed to stream_grid /
                        stream_blocks, as written -- test_grid_cap_host.py finds every such launch in the sources and compares,
                        so a new or changed launch makes this table stale loudly
    names               the profile names the site can emit (tsdr_profile_get)
    cases               {case: work items as a function of the case's parameters}: the cases of CASES that run the site past the
                        cap, cap < work <= 3 * cap
    exempt              or the reason it has none (EXEMPT_REASONS: two are accepted, at most four entries in all)
    fixed               a power of two / a multiple of 256 by construction: the site cannot be given a ragged size

CASES maps a case to its parameters as a function of the device's CU count; the sizes are the smallest convenient ones, odd
wherever the entry point lets them be (no multiple of 256, none of a vector width: the tail exists, and some threads take one
trip more than others).  The entry point, the reference and the bar of each case are in test_grid_cap_gpu.py (RUNNERS), next to
the test they are taken from.
"""
from collections import namedtuple

BLOCK = 256
BLOCKS_PER_CU = 8
ACC_BLOCKS = 2048          # group.hip:k_acc
ARGMAX_BLOCKS = 256        # autocorr.hip:argmax_launch (2048 values per workgroup and trip)
CU_COUNTS = (256, 64)      # an MI355X, and a partition of one


def cap(cu):
    """work items of a full streaming grid: common.h:stream_blocks"""
    return (cu if cu > 0 else 256) * BLOCKS_PER_CU * BLOCK


def cdiv(a, b):
    return -(-a // b)


def pow2_at_least(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def is_smooth(n, primes=(2, 3, 5)):
    for p in primes:
        while n % p == 0:
            n //= p
    return n == 1


def next_rough(n, primes=(2, 3, 5)):
    """the first odd number >= n that is no product of `primes` (takes the chirp-z route)"""
    n |= 1
    while is_smooth(n, primes):
        n += 2
    return n


def smooth_in(lo, hi, primes=(3, 5), avoid_pow2=True):
    """the smallest product of `primes` in (lo, hi]; with 2 among them: no power of two, no multiple of 256"""
    best = None

    def walk(v, i):
        nonlocal best
        if v > hi:
            return
        if v > lo and (best is None or v < best) and v % 256 and not (avoid_pow2 and v & (v - 1) == 0):
            best = v
        for j in range(i, len(primes)):
            walk(v * primes[j], j)
    walk(1, 0)
    assert best is not None, (lo, hi, primes)
    return best


def w3(cu):
    """an odd number of work items a little above 2 1/3 caps: three trips for a third of the threads, two for the rest"""
    c = cap(cu)
    return (2 * c + c // 3) | 1


def w2(cu):
    """the same a little above 1 1/3 caps (where the data a case moves grows with more than the work items)"""
    c = cap(cu)
    return (c + c // 3) | 1


FMTS = ("sc16", "sc8", "uc8")
SPV = {"cf32": 4, "sc16": 4, "sc8": 8, "uc8": 8}      # samples per work item of the 16-byte vector kernels

CASES = {}


def _case(name, fn):
    assert name not in CASES, name
    CASES[name] = fn


# ---- demodulators --------------------------------------------------------------------------------------------------------------
for _kind in ("am", "abs2", "invert"):
    for _fmt in ("cf32",) + FMTS:
        # vector kernels: work items = ceil(n / SPV), and SPV - 1 samples left for workgroup 0's tail
        _case(f"{_kind}-{_fmt}-vec", lambda cu, v=SPV[_fmt]: dict(n=v * (w3(cu) - 1) + v - 1, spv=v))
        _case(f"{_kind}-{_fmt}-one", lambda cu: dict(n=w3(cu), spv=1))
    _case(f"{_kind}-f64", lambda cu: dict(n=w3(cu), spv=1))
for _fmt in ("cf32", "f64") + FMTS:
    _case(f"fm-{_fmt}", lambda cu: dict(n=w3(cu)))
_case("expand-sc16", lambda cu: dict(n=w3(cu)))
for _fmt in ("sc8", "uc8"):
    _case(f"expand-{_fmt}-pair", lambda cu: dict(n=2 * w3(cu) - 1))      # (n + 1) / 2 work items, the odd last sample goes alone
    _case(f"expand-{_fmt}-one", lambda cu: dict(n=w3(cu)))
_case("ring-sc16", lambda cu: dict(n=w3(cu)))
_case("ring-sc8", lambda cu: dict(n=2 * w3(cu) - 1))
_case("ring-uc8", lambda cu: dict(n=2 * w3(cu) - 1))

# ---- resizing ------------------------------------------------------------------------------------------------------------------
for _t in ("f32", "f64"):
    _case(f"resize1d-{_t}", lambda cu: dict(n_in=w3(cu) // 3, n_out=w3(cu)))
    _case(f"naive-{_t}", lambda cu: dict(n=(w3(cu) // 3) | 1, up=3))
    _case(f"resize2d-{_t}", lambda cu: dict(h_in=333, w_in=517, h_out=(w3(cu) // 1201) | 1, w_out=1201))


# ---- f32 Bluestein and its helpers ---------------------------------------------------------------------------------------------
def _blu(n, batch=1):
    return dict(n=n, batch=batch, L=pow2_at_least(2 * n - 1))


# batch = 3 at a length whose L * batch wraps while L does not; batch = 1 at a length whose L itself wraps
_case("blu-batch3", lambda cu: _blu(next_rough(2 * cap(cu) // 5), 3))
_case("blu-L", lambda cu: _blu(next_rough(cap(cu) // 2 + cap(cu) // 6)))
_case("spectrum-blu-real", lambda cu: _blu(next_rough(w2(cu))))


def _cac(cu):
    cnt = w2(cu)
    while is_smooth(2 * cnt - 1):
        cnt += 2
    return dict(cnt=cnt, **_blu(2 * cnt - 1))     # len = 2 cnt - 1 samples: n = len, every lag up to cnt


_case("cac-blu", _cac)
# r2c and the writer behind a batched transform the whole-row launch declines (960 points: no three-step kernel; real rows)
_case("waterfall-960-real", lambda cu: dict(N=960, nb=(2 * cap(cu) // 960 + 37) | 1))

# ---- autocorrelation helpers (the routes without fusions) -------------------------------------------------------------------------
# n = 2 * 2^k real samples: forward, "ac_power", inverse, "ac_finish"; the lag window ends at n / 2
_case("ac-pow2", lambda cu: dict(n=8 * cap(cu), Mc=4 * cap(cu), cnt=w3(cu), k0=4 * cap(cu) - w3(cu)))
# IQ at an odd sample: "ac_pack", the zero-padded transform, "ac_fold"
_case("ac-pack-iq-odd", lambda cu: dict(n=w2(cu), Mc=pow2_at_least(2 * (w2(cu) - 1)) // 2, cnt=w2(cu) // 2))
# an odd number of real samples: the zero-padded transform straight from the samples, "ac_fold" over more lags than the cap
_case("ac-fold-odd", lambda cu: dict(n=2 * w2(cu) - 1, cnt=w2(cu)))
_case("ac-finish", lambda cu: dict(k0=777, cnt=w3(cu)))


def _pc(cu):
    c = cap(cu)
    n_lags, cnt = c + 999, c // 2 + 77
    n = n_lags + 5001
    return dict(n=n, m0=n - cnt // 2, cnt=cnt, n_lags=n_lags, M=pow2_at_least(cnt + n_lags - 1))


_case("pc", _pc)
_case("group-acc", lambda cu: dict(cnt=ACC_BLOCKS * BLOCK + ACC_BLOCKS * BLOCK // 3 + 1))     # its cap does not follow the CU count

# ---- Float64 ---------------------------------------------------------------------------------------------------------------------
P13 = (2, 3, 5, 7, 11, 13)     # fft64.hip's Stockham radices; any other length is its chirp-z


def _blu64(n):
    return dict(N=n, L=pow2_at_least(2 * n - 1))


_case("spectrum-f64-blu", lambda cu: _blu64(next_rough(w2(cu), P13)))                      # N wraps (L = 4 caps)
_case("spectrum-f64-blu-L", lambda cu: _blu64(next_rough(cap(cu) // 2 + cap(cu) // 6, P13)))   # L = 2 caps


def _ac64(cu):
    c = cap(cu)
    imax = smooth_in(c + c // 8, c + c // 2, (3, 5, 7))       # odd; n = 2 imax has Stockham passes only
    return dict(n=2 * imax, cnt=imax, len=2 * imax + 11)


_case("autocorr-f64", _ac64)
_case("welch-f64-big", lambda cu: dict(N=smooth_in(2 * cap(cu), 3 * cap(cu), (3, 5)), nb=1))
_case("seg64-blu-post", lambda cu: dict(N=4093, L=8192, nb=2 * cap(cu) // 4093 + 20))
_case("seg64-blu-prep", lambda cu: dict(N=4093, L=8192, nb=2 * cap(cu) // 8192 + 10))
# (7 times a product of 3s and 5s: no 2^a 3^b 5^c length, so the plain stuff / filter / real kernels run, around Stockham passes)
_case("resampler-f64", lambda cu: dict(bufferSize=7 * smooth_in(2 * cap(cu) // 14, 3 * cap(cu) // 14), up=2))

# ---- init_resampler / resampler! (Float32) -----------------------------------------------------------------------------------------
_case("resampler-f32-odd", lambda cu: dict(bufferSize=7 * smooth_in(2 * cap(cu) // 21, 3 * cap(cu) // 21), up=3))


def _rs_mid(cu):
    c = cap(cu)
    s = smooth_in(c // 2 + c // 8, 3 * c // 4, (2, 3, 5))
    return dict(bufferSize=2 * s, up=4)


_case("resampler-f32-mid", _rs_mid)


# ---- the direct raster kernel of the frame loop ------------------------------------------------------------------------------------
def _direct(cu):
    c = cap(cu)
    y_t = 700
    x_t = (c + c // 8) // (cdiv(y_t, 64) * 64) + 1
    return dict(y_t=y_t, x_t=x_t, S=16 * y_t * x_t, fmt="sc8")      # 16 samples per raster pixel: no tile fits


_case("raster-direct", _direct)

# ---- whole-row FFT launches --------------------------------------------------------------------------------------------------------
# (mode, N) -> (rows per tile, workgroups per CU): fft_plan.h's tables, restated so that the row count follows from the CU count
# alone; test_grid_cap_host.py holds them against the planner itself (tools/host_plan/fft_plan_dump --rows)
ROW_TILES = {("welch", 1000): (8, 2), ("welch", 2000): (4, 2), ("welch", 500): (8, 3),
             ("store", 1000): (4, 3), ("store", 2000): (4, 2), ("store", 500): (4, 3),
             ("wfall", 1000): (4, 4), ("wfall", 2000): (4, 2), ("wfall", 500): (4, 8),
             ("welch", 960): (4, 3)}
ROW_KINDS = {"welch": ("cf32", "real", "sc16"), "store": ("cf32",), "wfall": ("cf32", "real", "sc8")}
ROW_NAMES = {"welch": "welch_rows_acc3", "store": "fft_rows3", "wfall": "waterfall_rows3"}
ROW_SIG_KIND = {"real": 0, "cf32": 1, "sc16": 2, "sc8": 3, "uc8": 4}       # fft_dev.h: SIG_*


def _rows(mode, N):
    T, per_cu = ROW_TILES[(mode, N)]

    def fn(cu):
        grid = (cu if cu > 0 else 256) * per_cu
        ntiles = grid + grid // 8 + 1          # an eighth of the workgroups walk a second tile (every case moves N * rows samples)
        return dict(N=N, rows=T * ntiles - (T - 1), T=T, grid=grid, ntiles=ntiles)     # one row in the last tile
    return fn


ROW_CASES = []       # (case, mode, N, kind)
for _mode in ("welch", "store", "wfall"):
    for _N in (1000, 2000, 500):     # the lengths of TSDR_MIX3_LIST
        for _k in ROW_KINDS[_mode]:
            ROW_CASES.append((f"rows-{_mode}-{_N}-{_k}", _mode, _N, _k))
ROW_CASES.append(("rows-welch-960-cf32", "welch", 960, "cf32"))      # "welch_rows_acc": the generic LDS-stage kernel
for _c, _mode, _N, _k in ROW_CASES:
    _case(_c, _rows(_mode, _N))
# (ROWS_TO_STORE of integer IQ -- M3_ROWS_IQ -- has no case: tsdr_fft_c2c_d takes ComplexF32, and the spectra hand integer rows of
# these lengths to the Welch / waterfall launches, never to the row store)

# ---- the sites -------------------------------------------------------------------------------------------------------------------------
Site = namedtuple("Site", "file token expr names cases exempt fixed note")
EXEMPT_REASONS = ("cannot exceed the cap by construction", "smallest wrapping input above 256 MB of device memory")
SITES = []


def S(file, token, expr, names, cases=None, exempt=None, fixed=False, note=""):
    SITES.append(Site(file, token, expr, tuple(names), dict(cases or {}), exempt, fixed, note))


def _each(pattern, keys, work):
    return {pattern.format(k): work for k in keys}


n_ = lambda p: p["n"]                       # noqa: E731
_vec = lambda p: cdiv(p["n"], p["spv"])     # noqa: E731
_K3 = ("am", "abs2", "invert")

# demod.hip
S("demod.hip", 'MODE == DM_ABS ? "am_demod" : "abs2"', "ceil_div(n, 4)", ("am_demod", "abs2"), _each("{}-cf32-vec", ("am", "abs2"), _vec))
S("demod.hip", 'MODE == DM_ABS ? "am_demod1" : "abs2_1"', "n", ("am_demod1", "abs2_1"), _each("{}-cf32-one", ("am", "abs2"), n_))
S("demod.hip", "kVec[iqf_name(iqf)]", "ceil_div(n, iqf == IQF_SC16 ? 4 : 8)", ("demod_iq_sc16", "demod_iq_sc8", "demod_iq_uc8"),
  {f"{k}-{f}-vec": _vec for k in _K3 for f in FMTS})
S("demod.hip", "kOne[iqf_name(iqf)]", "n", ("demod1_iq_sc16", "demod1_iq_sc8", "demod1_iq_uc8"), {f"{k}-{f}-one": n_ for k in _K3 for f in FMTS})
S("demod.hip", '"invert_am_abs"', "ceil_div(n, 4)", ("invert_am_abs",), {"invert-cf32-vec": _vec})
S("demod.hip", '"invert_am_abs1"', "n", ("invert_am_abs1",), {"invert-cf32-one": n_})
S("demod.hip", '"invert_am_scale"', "n", ("invert_am_scale",), {"invert-cf32-one": n_}, note="tsdr_invert_am_d")
S("demod.hip", '"invert_am_scale"', "n", ("invert_am_scale",), {"invert-sc16-one": n_, "invert-sc8-one": n_, "invert-uc8-one": n_}, note="tsdr_invert_am_iq_d")
S("demod.hip", '"fm_demod"', "n", ("fm_demod",), {"fm-cf32": n_})
S("demod.hip", "kName[iqf_name(iqf)]", "n", ("fm_demod_iq_sc16", "fm_demod_iq_sc8", "fm_demod_iq_uc8"), _each("fm-{}", FMTS, n_))
# demod64.hip
S("demod64.hip", "kname", "n", ("am_demod_f64", "abs2_f64"), {"am-f64": n_, "abs2-f64": n_})
S("demod64.hip", "const int grid", "n", ("invert_am_f64_abs", "invert_am_f64_scale"), {"invert-f64": n_})
S("demod64.hip", '"fm_demod_f64"', "n", ("fm_demod_f64",), {"fm-f64": n_})
# ring.hip
S("ring.hip", '"iq_expand_sc16"', "n", ("iq_expand_sc16",), {"expand-sc16": n_})
S("ring.hip", "const dim3 grid", "(n + 1) / 2", ("iq_expand_uc8", "iq_expand_sc8"), _each("expand-{}-pair", ("sc8", "uc8"), lambda p: (p["n"] + 1) // 2))
S("ring.hip", "const dim3 grid", "n", ("iq_expand_uc8_1", "iq_expand_sc8_1"), _each("expand-{}-one", ("sc8", "uc8"), n_))
S("ring.hip", "const dim3 grid", "(r->nEch + 1) / 2", (), _each("ring-{}", ("sc8", "uc8"), lambda p: (p["n"] + 1) // 2),
  note="the staging ring's own expansion on its copy stream: no profile name")
S("ring.hip", "k_sc16_to_cf32", "r->nEch", (), {"ring-sc16": n_}, note="the staging ring's own expansion on its copy stream: no profile name")
# resample.hip / resample64.hip
_hw = lambda p: p["h_out"] * p["w_out"]     # noqa: E731
_nup = lambda p: p["n"] * p["up"]           # noqa: E731
S("resample.hip", '"resize2d"', "(size_t)h_out * w_out", ("resize2d",), {"resize2d-f32": _hw})
S("resample.hip", '"resize1d"', "n_out", ("resize1d",), {"resize1d-f32": lambda p: p["n_out"]})
S("resample.hip", '"naive_resample"', "n * (size_t)up", ("naive_resample",), {"naive-f32": _nup})
S("resample64.hip", '"resize1d_f64"', "n_out", ("resize1d_f64",), {"resize1d-f64": lambda p: p["n_out"]})
S("resample64.hip", '"resize2d_f64"', "(size_t)h_out * w_out", ("resize2d_f64",), {"resize2d-f64": _hw})
S("resample64.hip", '"naive_resample_f64"', "n * (size_t)up", ("naive_resample_f64",), {"naive-f64": _nup})
# fft.hip
_Lb = lambda p: p["L"] * p["batch"]         # noqa: E731
_nb = lambda p: p["n"] * p["batch"]         # noqa: E731
S("fft.hip", '"blu_chirp"', "n", ("blu_chirp",), {"cac-blu": n_})
S("fft.hip", '"blu_b"', "pl.L", ("blu_b",), {"blu-L": lambda p: p["L"]}, fixed=True)
S("fft.hip", '"r2c"', "n * batch", ("r2c",), {"waterfall-960-real": lambda p: p["N"] * p["nb"]})
S("fft.hip", '"blu_pre"', "L * batch", ("blu_pre",), {"blu-batch3": _Lb, "blu-L": _Lb}, fixed=True)
S("fft.hip", '"blu_mul"', "L * batch", ("blu_mul",), {"blu-batch3": _Lb, "blu-L": _Lb}, fixed=True)
S("fft.hip", '"blu_post"', "n * batch", ("blu_post",), {"blu-batch3": _nb, "cac-blu": _nb, "spectrum-blu-real": _nb})
# spectrum.hip
S("spectrum.hip", '"spectrum_out"', "N", ("spectrum_out",), {"spectrum-blu-real": n_})
S("spectrum.hip", '"waterfall_out"', "sizeFFT * nbSeg", ("waterfall_out",), {"waterfall-960-real": lambda p: p["N"] * p["nb"]})
_rsN = lambda p: p["bufferSize"] * p["up"]  # noqa: E731
S("spectrum.hip", '"lpf_window64"', "N", ("lpf_window64",), {"resampler-f32-odd": _rsN, "resampler-f64": _rsN})
S("spectrum.hip", '"lpf_altsign64"', "N", ("lpf_altsign64",), {"resampler-f32-odd": _rsN, "resampler-f64": _rsN})
S("spectrum.hip", '"lpf_herm_half"', "N / 2 + 1", ("lpf_herm_half",), {"resampler-f32-mid": lambda p: _rsN(p) // 2 + 1})
S("spectrum.hip", '"resampler_mid"', "M / 2 + 1", ("resampler_mid",), {"resampler-f32-mid": lambda p: _rsN(p) // 4 + 1})
S("spectrum.hip", '"resampler_stuff"', "N", ("resampler_stuff",), {"resampler-f32-odd": _rsN})
S("spectrum.hip", '"resampler_filter"', "N", ("resampler_filter",), {"resampler-f32-odd": _rsN})
S("spectrum.hip", '"resampler_out"', "N", ("resampler_out",), {"resampler-f32-odd": _rsN})
S("spectrum.hip", '"lpf_c32"', "r->sizeFFT", ("lpf_c32",), {"resampler-f32-odd": _rsN})
# autocorr.hip / autocorr_cplx.hip
_cnt = lambda p: p["cnt"]                   # noqa: E731
S("autocorr.hip", '"ac_power"', "Mc / 2 + 1", ("ac_power",), {"ac-pow2": lambda p: p["Mc"] // 2 + 1}, note="n = 2 * 2^k")
S("autocorr.hip", '"ac_finish"', "cnt", ("ac_finish",), {"ac-pow2": _cnt}, note="autocorr_core")
S("autocorr.hip", '"ac_pack"', "Mc", ("ac_pack",), {"ac-pack-iq-odd": lambda p: p["Mc"]}, fixed=True)
S("autocorr.hip", '"ac_power"', "Mc / 2 + 1", ("ac_power",), exempt=EXEMPT_REASONS[0],
  note="the in-place power spectrum of the zero-padded route runs for single-pass transforms only (logM - 1 <= 8): Mc / 2 + 1 <= 129 work items")
S("autocorr.hip", '"ac_fold"', "cnt", ("ac_fold",), {"ac-fold-odd": _cnt})
S("autocorr.hip", '"pc_pack"', "M", ("pc_pack",), {"pc": lambda p: p["M"]}, fixed=True)
S("autocorr.hip", '"pc_cross"', "M / 2 + 1", ("pc_cross",), {"pc": lambda p: p["M"] // 2 + 1})
S("autocorr.hip", '"pc_real"', "n_lags", ("pc_real",), {"pc": lambda p: p["n_lags"]})
S("autocorr.hip", '"ac_finish"', "cnt", ("ac_finish",), {"ac-finish": _cnt}, note="tsdr_autocorr_finish_d")
S("autocorr_cplx.hip", '"cac_power"', "n", ("cac_power",), {"cac-blu": n_})
S("autocorr_cplx.hip", '"cac_finish"', "cnt", ("cac_finish",), {"cac-blu": _cnt})
# fft64.hip / spectrum64.hip / spectra64.hip
_N = lambda p: p["N"]                       # noqa: E731
_L = lambda p: p["L"]                       # noqa: E731
S("fft64.hip", '"fft64_pass"', "N / r", ("fft64_pass",), {"spectrum-f64-blu": lambda p: p["L"] // 2}, fixed=True,
  note="N / r items per radix-r pass; past the cap only with r = 2 (any N up to three caps): the chirp-z's power-of-two passes")
S("fft64.hip", '"fft64_scale"', "N", ("fft64_scale",), {"autocorr-f64": n_})
S("fft64.hip", '"fft64_blue_prep"', "L", ("fft64_blue_prep",), {"spectrum-f64-blu-L": _L}, fixed=True)
S("fft64.hip", '"fft64_blue_mul"', "L", ("fft64_blue_mul",), {"spectrum-f64-blu-L": _L}, fixed=True)
S("fft64.hip", '"fft64_blue_post"', "N", ("fft64_blue_post",), {"spectrum-f64-blu": _N})
S("spectrum64.hip", '"autocorr_f64_load"', "n", ("autocorr_f64_load",), {"autocorr-f64": n_})
S("spectrum64.hip", '"autocorr_f64_power"', "n", ("autocorr_f64_power",), {"autocorr-f64": n_})
S("spectrum64.hip", '"autocorr_f64_out"', "cnt", ("autocorr_f64_out",), {"autocorr-f64": _cnt})
S("spectrum64.hip", '"spectrum_f64_load"', "N", ("spectrum_f64_load",), {"spectrum-f64-blu": _N})
S("spectrum64.hip", '"spectrum_f64_out"', "N", ("spectrum_f64_out",), {"spectrum-f64-blu": _N})
_BN = lambda p: p["N"] * p["nb"]            # noqa: E731
_BL = lambda p: p["L"] * p["nb"]            # noqa: E731
S("spectra64.hip", '"seg64_widen"', "B * N", ("seg64_widen",), {"welch-f64-big": _BN})
S("spectra64.hip", '"seg64_blue_prep"', "B * L", ("seg64_blue_prep",), {"seg64-blu-prep": _BL}, fixed=True)
S("spectra64.hip", '"seg64_blue_mul"', "B * L", ("seg64_blue_mul",), {"seg64-blu-prep": _BL}, fixed=True)
S("spectra64.hip", '"seg64_blue_post"', "B * N", ("seg64_blue_post",), {"seg64-blu-post": _BN})
S("spectra64.hip", '"welch64_acc"', "N", ("welch64_acc",), {"welch-f64-big": _N})
S("spectra64.hip", '"waterfall64_rows"', "b * N", ("waterfall64_rows",), {"welch-f64-big": _BN, "seg64-blu-post": _BN})
S("spectra64.hip", '"resampler64_stuff"', "N", ("resampler64_stuff",), {"resampler-f64": _rsN})
S("spectra64.hip", '"resampler64_filter"', "N", ("resampler64_filter",), {"resampler-f64": _rsN})
S("spectra64.hip", '"resampler64_out"', "N", ("resampler64_out",), {"resampler-f64": _rsN})
# image_plan.h
S("image_plan.h", "s.grid[0]", "ceil_div((size_t)y_t, 64) * 64 * (size_t)x_t", ("raster_direct_iq", "raster_direct_f32"),
  {"raster-direct": lambda p: cdiv(p["y_t"], 64) * 64 * p["x_t"]}, fixed=True, note="k_raster_direct: whole 64-line strips")
S("image_plan.h", "s.grid[0]", "(size_t)h_out * w_out", ("resize2d",), exempt=EXEMPT_REASONS[0],
  note="the frame loop's per-frame fallback always writes the 600 x 800 = 480 000 rendered pixels: below the cap of a device with 235 CUs "
       "or more (the MI355X has 256); tsdr_resize2d_d, which takes any size, runs the same kernel past it (resize2d-f32)")

# ---- launches with a cap of their own ------------------------------------------------------------------------------------------------
OWN_CAP = {
    # k_argmax: 256 workgroups of 256, i.e. 65 536 values per trip
    "argmax": dict(file="autocorr.hip", token='"argmax"', expr="std::min<size_t>(ceil_div(n, 2048), 256)", names=("argmax",), cap=ARGMAX_BLOCKS * BLOCK,
                   covered_by=("test_dptr_gpu.py", "test_argmax_at_offsets", "100_003")),
    # group.hip:k_acc: 2048 workgroups of 256; the sharded search of two members sharing a device adds the second member's partial sums
    "k_acc": dict(file="group.hip", token="k_acc", expr="std::min<size_t>(ceil_div(count, 256), 2048)", names=(), cap=ACC_BLOCKS * BLOCK,
                  cases={"group-acc": _cnt}),
}

# ---- the steps plan_rows adds ----------------------------------------------------------------------------------------------------------
# name -> (grid expression as written, cases)
ROW_STEPS = {
    "welch_rows_acc3": ("std::min(ntiles, opts_cus(o) * (unsigned)per_cu)", [c for c, m, N, k in ROW_CASES if m == "welch" and N != 960]),
    "fft_rows3": ("std::min(ntiles, opts_cus(o) * (unsigned)per_cu)", [c for c, m, N, k in ROW_CASES if m == "store"]),
    "waterfall_rows3": ("std::min(ntiles, opts_cus(o) * (unsigned)per_cu)", [c for c, m, N, k in ROW_CASES if m == "wfall"]),
    "welch_rows_acc": ("std::min(ntiles, opts_cus(o) * per_cu)", ["rows-welch-960-cf32"]),
}


def params(case, cu):
    return CASES[case](cu)


def sites_of(case):
    """the entries a case drives past the cap: [(site, work function)]"""
    out = [(s, s.cases[case]) for s in SITES if case in s.cases]
    out += [(Site(o["file"], o["token"], o["expr"], o["names"], o["cases"], None, False, ""), o["cases"][case])
            for o in OWN_CAP.values() if case in o.get("cases", {})]
    return out


def cap_of(site, cu):
    for o in OWN_CAP.values():
        if (o["file"], o["token"]) == (site.file, site.token):
            return o["cap"]
    return cap(cu)
