"""GPU tests of phase-coherent frame folding (include/tempest_hip_cfold.h): the fold and the carrier scan against tests/cfold_ref.py
within the contract's error bounds, format invariance and repeatability bit for bit, the known answers of a constant sample, the
capability itself (a picture the envelope fold loses at -10 dB), the carry across buffers, and every refusal.  Every device pointer sits
inside a guarded arena (tests/dptr_util.py): `state` at 4, 8 and 12 mod 16, ComplexF32 `iq` at 0 and 8 mod 16.

The captures are synth_leak(60 T, x, y, 60.0, n): one frame lasts exactly T samples and the carrier (df = 1 kHz) advances by
kappa_true = frac(1000 / 60) = 0.6667 turns per frame.  Which case reaches which kernel (W = ceil(128 * T / P) + 3 against
TSDR_CFOLD_STAGE_MAX = 120; asserted by profile name):
    U  70 x 150, T 1207.73   W  18  cfold_tile / cfold_scan_tile      partial second line tile, partial pixel tile
    M  66 x 160, T 9150.37   W 114  cfold_tile / cfold_scan_tile
    D  77 x 131, T 11600.61  W 151  cfold_direct / cfold_scan_direct  odd sizes; starts one period in
    S  20 x 140, T 2550.3    W 120  cfold_tile / cfold_scan_tile      the widest span the tiled kernel stages
    R  20 x 140, T 2565.3    W 121  cfold_direct / cfold_scan_direct  the narrowest span of the direct kernel
    X   8 x 16,  T 5000.5    W 5004 cfold_direct / cfold_scan_direct  39 samples per pixel
    Q  66 x 160, T 9150.37, F 16, -10 dB: the capability case

Captures and references are made once per case (functools caches); nothing modifies them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cfold_ref as R
import dptr_util as D
import fold_ref as FR

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = {
    "U": dict(y=70, x=150, T=1207.73, F=7, t0=3.25),
    "M": dict(y=66, x=160, T=9150.37, F=5, t0=0.0),
    "D": dict(y=77, x=131, T=11600.61, F=4, t0=11599.9),
    "S": dict(y=20, x=140, T=2550.3, F=3, t0=1.5),
    "R": dict(y=20, x=140, T=2565.3, F=3, t0=1.5),
    "X": dict(y=8, x=16, T=5000.5, F=3, t0=0.5),
    "Q": dict(y=66, x=160, T=9150.37, F=16, t0=0.0),
}
FOLD_CASES = ["U", "M", "D", "S", "R", "X"]
KERNEL = {"U": "tile", "M": "tile", "D": "direct", "S": "tile", "R": "direct", "X": "direct"}
STATE_PHASE = {"U": 4, "M": 8, "D": 12, "X": 4, "S": 8, "R": 12}
IQ_PHASE = {"U": 0, "M": 8, "D": 0, "X": 8, "S": 0, "R": 8}
KAPPA_TRUE = (1000.0 / 60.0) % 1.0
KAPPAS = {"true": KAPPA_TRUE, "zero": 0.0, "minus3": KAPPA_TRUE - 3.0}
KB = 8                        # trials per workgroup of the scan kernels (raster_cfold.hip:kBatch)
N_TRIALS, N_RAGGED = 9, 2 * KB + 3


def _n(c):
    return int(math.ceil(c["t0"] + c["F"] * (c["T"] + 2.0))) + 5


def _pkg(name):
    import importlib
    from tempest_loader import load_package
    load_package()
    return importlib.import_module("tempestsdr_jl_amd." + name)


@functools.lru_cache(maxsize=None)
def _capture(name, snr_db=20.0, extra=0):
    """(iq complex64[n], amax) of a case: Fs = 60 T, so one frame of the synthetic leak lasts exactly T samples"""
    c = CASES[name]
    iq = _pkg("synth").synth_leak(60.0 * c["T"], c["x"], c["y"], 60.0, _n(c) + extra, snr_db=snr_db)
    iq.setflags(write=False)
    return iq, float(np.abs(R.samples(iq)).max())


@functools.lru_cache(maxsize=None)
def _ref_fold(name, kappa):
    c = CASES[name]
    return R.cfold(R.samples(_capture(name)[0]), c["t0"], c["T"], kappa, c["F"], c["y"], c["x"])


def _dk(c):
    return 1.0 / (8 * c["F"])


@functools.lru_cache(maxsize=None)
def _ref_scan(name, n_trials):
    c = CASES[name]
    half = (n_trials - 1) // 2
    return R.scan(R.samples(_capture(name)[0]), c["t0"], c["T"], KAPPA_TRUE - half * _dk(c), _dk(c), n_trials, c["F"], c["y"], c["x"])


def _fill(ctx, arena, data):
    """put `data` into an OUTPUT arena's payload (a state the call may overwrite)"""
    d = np.ascontiguousarray(data)
    assert d.nbytes == arena.payload
    ctx.call("tsdr_upload", arena.ptr, C.c_void_p(d.ctypes.data), d.nbytes)


def _fold_d(ctx, iq, fmt, scale, n, t0, T, kappa, F, y, x, alpha, state):
    ctx.call("tsdr_cfold_iq_d", iq, fmt, C.c_float(scale), n, C.c_double(t0), C.c_double(T), C.c_double(kappa), F, y, x, C.c_float(alpha),
             state)


def _scan_d(ctx, iq, fmt, scale, n, t0, T, k0, dk, nt, F, y, x, score):
    ctx.call("tsdr_cfold_scan_iq_d", iq, fmt, C.c_float(scale), n, C.c_double(t0), C.c_double(T), C.c_double(k0), C.c_double(dk), nt, F, y,
             x, score)


def _profiled(ctx, fn):
    """the profile names of the launches fn() makes"""
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_reset()
    try:
        fn()
        ctx.synchronize()
        return set(ctx.profile_results())
    finally:
        ctx.profile(False)


def _report(what, err, bound):
    print(f"{what}: max error {err:.4g}, bound {bound:.4g}, max error / bound {err / bound:.3f}")


# ---------------------------------------------------------------- 1. the fold against the reference
@pytest.mark.parametrize("kappa", list(KAPPAS))
@pytest.mark.parametrize("alpha", [0.0, 0.25])
@pytest.mark.parametrize("name", FOLD_CASES)
def test_fold_matches_the_reference(ctx, name, alpha, kappa):
    """|state - ref| <= 1.5 (F + 16) 2^-24 max(amax, max |state_in|).  alpha = 0 runs on an all-NaN state, which must not be read;
    alpha = 0.25 on a random positive state.  kappa: the capture's own, 0, and the capture's own minus three turns (only frac(kappa)
    matters).  The kernel the case takes is asserted by its profile name."""
    c = CASES[name]
    iq, amax = _capture(name)
    k = KAPPAS[kappa]
    P = c["y"] * c["x"]
    if alpha == 0:
        st_in = np.full(P, np.nan, F32)
    else:
        st_in = np.random.default_rng(P).uniform(0.001, 0.02, P).astype(F32)
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, IQ_PHASE[name])
        d_st = A.output("state", 4 * P, STATE_PHASE[name])
        _fill(ctx, d_st, st_in)
        names = _profiled(ctx, lambda: _fold_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], c["T"], k, c["F"], c["y"], c["x"], alpha, d_st.ptr))
        A.check()
        got = d_st.get(F32)
    assert names == {"cfold_" + KERNEL[name]}, names
    assert not np.isnan(got).any()
    ref = _ref_fold(name, k)
    if alpha:
        ref = float(F32(alpha)) * st_in.astype(np.float64) + (1.0 - float(F32(alpha))) * ref
    bound = R.eps_c(c["F"], amax, 0.0 if alpha == 0 else st_in.max())
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    _report(f"cfold {name} alpha {alpha} kappa {kappa}", err, bound)
    assert err <= bound, (name, alpha, kappa, err, bound)
    if kappa == "minus3":   # the references of kappa and kappa - 3 differ by the rounding of f * kappa alone
        assert np.max(np.abs(_ref_fold(name, k) - _ref_fold(name, KAPPA_TRUE))) <= 1e-9 * amax


def test_python_forms_agree_with_the_device_form(ctx):
    """Context.cfold (host arrays, tsdr_cfold_iq) and Context.cfold_d give the same bits; state comes back as (y_t, x_t)"""
    c = CASES["U"]
    iq, amax = _capture("U")
    P = c["y"] * c["x"]
    host = ctx.cfold(iq, c["t0"], c["T"], KAPPA_TRUE, c["F"], c["y"], c["x"])
    assert host.shape == (c["y"], c["x"]) and host.dtype == F32
    with D.Arenas(ctx) as A:
        d_iq, d_st = A.input("iq", iq, 8), A.output("state", 4 * P, 12)
        ctx.cfold_d(d_iq.addr, "cf32", 1.0, iq.size, c["t0"], c["T"], KAPPA_TRUE, c["F"], c["y"], c["x"], 0.0, d_st.addr)
        A.check()
        dev = d_st.get(F32)
    assert np.array_equal(host.reshape(-1, order="F"), dev)
    assert np.max(np.abs(dev - _ref_fold("U", KAPPA_TRUE))) <= R.eps_c(c["F"], amax)
    st = np.asfortranarray(np.random.default_rng(1).uniform(0.001, 0.01, (c["y"], c["x"])).astype(F32))
    keep = st.copy()
    out = ctx.cfold(iq, c["t0"], c["T"], KAPPA_TRUE, c["F"], c["y"], c["x"], alpha=0.5, state=st)
    assert np.array_equal(st, keep), "the caller's state is an input"
    ref = 0.5 * st.reshape(-1, order="F").astype(np.float64) + 0.5 * _ref_fold("U", KAPPA_TRUE)
    assert np.max(np.abs(out.reshape(-1, order="F") - ref)) <= R.eps_c(c["F"], amax, st.max())
    raw = np.full((c["y"], c["x"]), np.nan, F32, order="F")
    ctx.call("tsdr_cfold_iq", C.c_void_p(iq.ctypes.data), 0, C.c_float(1.0), iq.size, C.c_double(c["t0"]), C.c_double(c["T"]),
             C.c_double(KAPPA_TRUE), c["F"], c["y"], c["x"], C.c_float(0.0), C.c_void_p(raw.ctypes.data))
    assert np.array_equal(raw, host)


# ---------------------------------------------------------------- 2. the scan against the reference
@pytest.mark.parametrize("name, n_trials", [("U", N_TRIALS), ("M", N_TRIALS), ("D", N_TRIALS), ("X", N_TRIALS), ("U", N_RAGGED),
                                            ("D", N_RAGGED)])
def test_scan_scores_and_maximum(ctx, name, n_trials):
    """trials spaced 1 / (8 F) around kappa_true -- nine of them, and 2 KB + 3 (more than one batch, not a multiple of it): every score
    within 2 eps_z sqrt(P ref) + P eps_z^2 of the reference's, the first maximum where the reference puts it (the middle).
    Precondition, on the reference: the top-2 relative margin is at least 4 x the relative score bound, so a tie cannot hide a
    failure.  The host form returns the same scores and `best`."""
    c = CASES[name]
    iq, amax = _capture(name)
    P, dk, half = c["y"] * c["x"], _dk(c), (n_trials - 1) // 2
    k0 = KAPPA_TRUE - half * dk
    ref = _ref_scan(name, n_trials)
    e = R.eps_z(c["F"], amax)
    bounds = np.array([R.score_bound(e, P, r) for r in ref])
    margin = R.top2_margin(ref)
    print(f"cscan {name} x{n_trials}: reference margin {margin:.4g}, relative bound {float(np.max(bounds / ref)):.4g}")
    assert R.first_max(ref) == half and margin >= 4 * float(np.max(bounds / ref)), (margin, bounds / ref)
    with D.Arenas(ctx) as A:
        d_iq, d_sc = A.input("iq", iq, IQ_PHASE[name]), A.output("score", 8 * n_trials, 8)
        names = _profiled(ctx, lambda: _scan_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], c["T"], k0, dk, n_trials, c["F"], c["y"], c["x"],
                                               d_sc.ptr))
        A.check()
        got = d_sc.get(np.float64)
    assert names == {"cfold_scan_" + KERNEL[name], "cfold_score"}, names
    _report(f"cscan {name} x{n_trials}", float(np.max(np.abs(got - ref) / bounds)), 1.0)
    assert np.all(np.abs(got - ref) <= bounds), (got, ref, bounds)
    assert R.first_max(got) == half
    host, best = ctx.cfold_scan(iq, c["t0"], c["T"], k0, dk, n_trials, c["F"], c["y"], c["x"])
    assert np.array_equal(host, got) and best == half
    sc, b = np.zeros(n_trials), C.c_int(-5)
    ctx.call("tsdr_cfold_scan_iq", C.c_void_p(iq.ctypes.data), 0, C.c_float(1.0), iq.size, C.c_double(c["t0"]), C.c_double(c["T"]),
             C.c_double(k0), C.c_double(dk), n_trials, c["F"], c["y"], c["x"], C.c_void_p(sc.ctypes.data), C.byref(b))
    assert np.array_equal(sc, got) and b.value == half


@pytest.mark.parametrize("name", ["S", "R"])
def test_scan_at_the_staging_boundary(ctx, name):
    """nine trials (a batch and one more) at the boundary cases: the scan makes the fold's choice (W 120: cfold_scan_tile, W 121:
    cfold_scan_direct), every score within the bound of the reference's.  No claim about the maximum: these cases carry no margin
    precondition."""
    c = CASES[name]
    iq, amax = _capture(name)
    P, dk = c["y"] * c["x"], _dk(c)
    k0 = KAPPA_TRUE - 4 * dk
    ref = _ref_scan(name, N_TRIALS)
    bounds = np.array([R.score_bound(R.eps_z(c["F"], amax), P, r) for r in ref])
    with D.Arenas(ctx) as A:
        d_iq, d_sc = A.input("iq", iq, IQ_PHASE[name]), A.output("score", 8 * N_TRIALS, 8)
        names = _profiled(ctx, lambda: _scan_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], c["T"], k0, dk, N_TRIALS, c["F"], c["y"], c["x"],
                                               d_sc.ptr))
        A.check()
        got = d_sc.get(np.float64)
    assert names == {"cfold_scan_" + KERNEL[name], "cfold_score"}, names
    _report(f"cscan {name} at the boundary", float(np.max(np.abs(got - ref) / bounds)), 1.0)
    assert np.all(np.abs(got - ref) <= bounds), (got, ref, bounds)


def test_a_trial_scores_the_picture_the_fold_leaves(ctx):
    """case X: trial 3 of a scan and the fold at kappa0 + 3 dkappa run the same operations; with alpha = 0 the state is |Z|, so the
    score is sum state^2 within the square root's rounding (2 * 2^-24 relative per pixel: (1 + 2u)^2 < 1 + 5u on the square)"""
    c = CASES["X"]
    iq, amax = _capture("X")
    P, dk = c["y"] * c["x"], _dk(c)
    k0 = KAPPA_TRUE - 4 * dk
    with D.Arenas(ctx) as A:
        d_iq, d_sc, d_st = A.input("iq", iq, 8), A.output("score", 8 * N_TRIALS, 0), A.output("state", 4 * P, 4)
        ctx.cfold_scan_d(d_iq.addr, 0, 1.0, iq.size, c["t0"], c["T"], k0, dk, N_TRIALS, c["F"], c["y"], c["x"], d_sc.addr)
        _fold_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], c["T"], k0 + 3 * dk, c["F"], c["y"], c["x"], 0.0, d_st.ptr)
        A.check()
        got, pic = d_sc.get(np.float64), d_st.get(F32).astype(np.float64)
    assert abs(got[3] - float(np.sum(pic * pic))) <= 5 * FR.ULP * got[3]


# ---------------------------------------------------------------- 3. formats and repeats
def _quantised(name, fmt):
    """(raw integer components, scale, expanded complex64) of a case's capture in an integer format"""
    api = _pkg("api")
    iq = _capture(name)[0]
    iq = iq[:iq.size - iq.size % 2]     # an even number of samples: 8-bit buffers then fill whole words of their arena
    full = {"sc16": 32767.0, "sc8": 127.0, "uc8": 127.0}[fmt]
    scale = float(np.abs(np.concatenate([iq.real, iq.imag])).max()) / full * 1.01
    comp = np.round(iq.view(F32).astype(np.float64) / scale)
    if fmt == "uc8":
        comp = np.floor(comp + 127.5)
    raw = comp.astype({"sc16": np.int16, "sc8": np.int8, "uc8": np.uint8}[fmt])
    return raw, scale, np.ascontiguousarray(api.expand_iq(raw, fmt, scale))


@pytest.mark.parametrize("fmt", ["sc16", "sc8", "uc8"])
def test_integer_formats_give_the_bits_of_the_expanded_buffer(ctx, fmt):
    """fold and scan scores (cases U: tiled, D: direct): sc16 / sc8 / uc8 in, the bits of the same call on the host-expanded ComplexF32"""
    code = {"sc16": 1, "sc8": 2, "uc8": 3}[fmt]
    for name in ("U", "D"):
        c = CASES[name]
        raw, scale, z = _quantised(name, fmt)
        n, P, dk = z.size, c["y"] * c["x"], _dk(c)
        k0 = KAPPA_TRUE - 4 * dk
        with D.Arenas(ctx) as A:
            d_raw, d_z = A.input("raw", raw, 0), A.input("expanded", z, 8)
            s_raw, s_z = A.output("state raw", 4 * P, 4), A.output("state expanded", 4 * P, 12)
            k_raw, k_z = A.output("score raw", 8 * N_TRIALS, 8), A.output("score expanded", 8 * N_TRIALS, 0)
            _fold_d(ctx, d_raw.ptr, code, scale, n, c["t0"], c["T"], KAPPA_TRUE, c["F"], c["y"], c["x"], 0.0, s_raw.ptr)
            _fold_d(ctx, d_z.ptr, 0, 1.0, n, c["t0"], c["T"], KAPPA_TRUE, c["F"], c["y"], c["x"], 0.0, s_z.ptr)
            _scan_d(ctx, d_raw.ptr, code, scale, n, c["t0"], c["T"], k0, dk, N_TRIALS, c["F"], c["y"], c["x"], k_raw.ptr)
            _scan_d(ctx, d_z.ptr, 0, 1.0, n, c["t0"], c["T"], k0, dk, N_TRIALS, c["F"], c["y"], c["x"], k_z.ptr)
            A.check()
            a, b = s_raw.get(np.uint32), s_z.get(np.uint32)
            assert np.array_equal(a, b), (name, fmt, int(np.count_nonzero(a != b)))
            ref = R.cfold(R.samples(z), c["t0"], c["T"], KAPPA_TRUE, c["F"], c["y"], c["x"])
            assert np.max(np.abs(s_z.get(F32) - ref)) <= R.eps_c(c["F"], np.abs(R.samples(z)).max()), "and they are the fold of that buffer"
            assert np.array_equal(k_raw.get(np.uint64), k_z.get(np.uint64)), (fmt, k_raw.get(np.float64), k_z.get(np.float64))
            assert np.all(k_z.get(np.float64) > 0)


@pytest.mark.parametrize("name", ["U", "D", "X"])
def test_two_calls_leave_identical_bits(ctx, name):
    c = CASES[name]
    iq = _capture(name)[0]
    P, dk = c["y"] * c["x"], _dk(c)
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, IQ_PHASE[name])
        st = [A.output(f"state {k}", 4 * P, 4 + 8 * k) for k in range(2)]
        sc = [A.output(f"score {k}", 8 * N_RAGGED, 8 * k) for k in range(2)]
        for k in range(2):
            _fold_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], c["T"], KAPPA_TRUE, c["F"], c["y"], c["x"], 0.0, st[k].ptr)
            _scan_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], c["T"], KAPPA_TRUE - 9 * dk, dk, N_RAGGED, c["F"], c["y"], c["x"], sc[k].ptr)
        A.check()
        assert np.array_equal(st[0].get(np.uint32), st[1].get(np.uint32))
        assert np.array_equal(sc[0].get(np.uint64), sc[1].get(np.uint64))
        assert np.all(np.isfinite(sc[0].get(np.float64)))


# ---------------------------------------------------------------- 4. known answers
@pytest.mark.parametrize("name", ["U", "R"])
def test_constant_sample_folds_to_its_magnitude_or_cancels(ctx, name):
    """a constant complex sample: kappa = 0 folds it to |z|; kappa = j / F, j not a multiple of F, to nothing -- the F roots of unity
    cancel -- both within eps_c; and the scan's scores are P |z|^2 and (below the bound) nothing"""
    c = CASES[name]
    z0 = np.complex64(0.3 - 0.4j)
    n, P, F = _n(c), c["y"] * c["x"], c["F"]
    iq = np.full(n, z0, np.complex64)
    bound = R.eps_c(F, abs(z0))
    with D.Arenas(ctx) as A:
        d_iq, d_st, d_sc = A.input("iq", iq, 8), A.output("state", 4 * P, 4), A.output("score", 8 * F, 8)
        for j in (0, 1, F - 1, F + 1, -1, -F):
            _fold_d(ctx, d_iq.ptr, 0, 1.0, n, c["t0"], c["T"], j / F, F, c["y"], c["x"], 0.0, d_st.ptr)
            A.check()
            got = d_st.get(F32).astype(np.float64)
            want = float(abs(z0)) if j % F == 0 else 0.0
            err = float(np.max(np.abs(got - want)))
            _report(f"constant {name} kappa {j}/{F}", err, bound)
            assert err <= bound, (j, err, bound)
        _scan_d(ctx, d_iq.ptr, 0, 1.0, n, c["t0"], c["T"], 0.0, 1.0 / F, F, F, c["y"], c["x"], d_sc.ptr)
        A.check()
        s = d_sc.get(np.float64)
    e = R.eps_z(F, abs(z0))
    ref0 = P * float(abs(z0)) ** 2
    assert abs(s[0] - ref0) <= R.score_bound(e, P, ref0) and np.all(s[1:] <= R.score_bound(e, P, 0.0)), s


# ---------------------------------------------------------------- 5. the capability
def _corr(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float(np.dot(a, b) / math.sqrt(np.dot(a, a) * np.dot(b, b)))


def test_coherent_fold_keeps_the_picture_the_envelope_fold_loses(ctx):
    """case Q: 16 frames at -10 dB per sample.  refine_carrier with levels = 1 scans 64 trials over [0, 1) and returns index 43
    (kappa = 0.671875; kappa_true = 0.6667), as the reference does (its top-2 margin: 0.048; the score bound is below a quarter of it).
    The coherent fold at that kappa correlates with the noiseless test card at c >= 0.60 and c >= e + 0.2, e the envelope fold's
    correlation on the same capture (reference: 0.680 and 0.373; the GPU differs from it by at most eps_c per pixel)."""
    c = CASES["Q"]
    synth = _pkg("synth")
    iq, amax = _capture("Q", -10.0)
    y, x, T, F = c["y"], c["x"], c["T"], c["F"]
    P = y * x
    z = R.samples(iq)
    k_ref, last_ref, levels = R.ladder(z, 0.0, T, F, y, x, levels=1)
    ref = levels[0]
    e_z = R.eps_z(F, amax)
    rel = float(np.max([R.score_bound(e_z, P, r) / r for r in ref]))
    margin = R.top2_margin(ref)
    print(f"capability: reference margin {margin:.4g}, relative score bound {rel:.4g}")
    assert ref.shape == (64,) and R.first_max(ref) == 43 and k_ref == 0.671875 and last_ref == 1.0 / 64
    assert rel < margin / 4
    b = synth.BLANK_BOX
    card = synth.test_card(x, y, row0=int(round(b["row0_frac"] * y)) % y, col0=int(round(b["col0_frac"] * x)) % x)
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, 8)
        d_c, d_e = A.output("coherent", 4 * P, 4), A.output("envelope", 4 * P, 12)
        k_hat, last, scores = ctx.refine_carrier(d_iq.addr, "cf32", 1.0, iq.size, 0.0, T, F, y, x, levels=1)
        assert len(scores) == 1 and scores[0].shape == (64,)
        assert np.all(np.abs(scores[0] - ref) <= [R.score_bound(e_z, P, r) for r in ref])
        assert R.first_max(scores[0]) == 43 and k_hat == 0.671875 and last == 1.0 / 64
        _fold_d(ctx, d_iq.ptr, 0, 1.0, iq.size, 0.0, T, k_hat, F, y, x, 0.0, d_c.ptr)
        ctx.call("tsdr_fold_iq_d", d_iq.ptr, 0, C.c_float(1.0), iq.size, C.c_double(0.0), C.c_double(T), F, y, x, C.c_float(0.0), d_e.ptr)
        A.check()
        coh = d_c.get(F32).reshape((y, x), order="F")
        env = d_e.get(F32).reshape((y, x), order="F")
    err = float(np.max(np.abs(coh.reshape(-1, order="F") - R.cfold(z, 0.0, T, k_hat, F, y, x))))
    _report("capability fold", err, R.eps_c(F, amax))
    assert err <= R.eps_c(F, amax)
    cc, ee = _corr(coh, card), _corr(env, card)
    print(f"capability: corr(card, coherent fold) {cc:.3f}, corr(card, envelope fold) {ee:.3f}")
    assert cc >= 0.60 and cc >= ee + 0.2, (cc, ee)


# ---------------------------------------------------------------- 6. the carry across buffers
def test_two_buffers_chained_by_fold_plan(ctx):
    """One capture of case M, 3.4 frames longer, cut after the case's n1 samples and chained by fold_plan: buffer 1 holds frames
    0 .. 4 (alpha = 0), frame 5 straddles the cut and is skipped, buffer 2 holds frames 6, 7 at the carried t0 and is averaged in
    with alpha = 0.5 -- the MAGNITUDES are averaged; each buffer's weights start at f = 0.  Against the reference's two steps:
    the first call's error, halved by the IIR, plus the second call's bound on a state_in that is at most amax + eps_c."""
    plan = _pkg("fold").fold_plan
    c = CASES["M"]
    T, y, x = c["T"], c["y"], c["x"]
    P, n1 = y * x, _n(c)
    n_long = int(math.ceil(8.4 * T)) + 5
    iq, amax = _capture("M", 20.0, n_long - n1)
    assert iq.size == n_long
    F1, t1 = plan(n1, 0.0, T)
    F2, t2 = plan(n_long - n1, t1, T)
    assert (F1, F2) == (5, 2) and abs((n1 + t1) - 6 * T) < 1e-9 and 0 < t2 <= T
    z = R.samples(iq)
    ref1 = R.cfold(z[:n1], 0.0, T, KAPPA_TRUE, F1, y, x)
    ref2 = R.cfold(z[n1:], t1, T, KAPPA_TRUE, F2, y, x, 0.5, ref1)
    with D.Arenas(ctx) as A:
        d_a, d_b = A.input("first", iq[:n1], 0), A.input("second", iq[n1:], 8)
        d_st = A.output("chained", 4 * P, 12)
        _fold_d(ctx, d_a.ptr, 0, 1.0, n1, 0.0, T, KAPPA_TRUE, F1, y, x, 0.0, d_st.ptr)
        _fold_d(ctx, d_b.ptr, 0, 1.0, n_long - n1, t1, T, KAPPA_TRUE, F2, y, x, 0.5, d_st.ptr)
        A.check()
        got = d_st.get(F32).astype(np.float64)
    bound = 0.5 * R.eps_c(F1, amax) + R.eps_c(F2, amax, amax + R.eps_c(F1, amax))
    err = float(np.max(np.abs(got - ref2)))
    _report("carry across buffers", err, bound)
    assert err <= bound


# ---------------------------------------------------------------- 7. refusals and untouched memory
def test_refusals_leave_everything_untouched(ctx):
    """every TSDR_EINVAL of the header, and F == 0 (TSDR_OK): the sentinels around iq, state and score, and the sentinel-filled state
    and score themselves, are as uploaded; iq is never written"""
    c = CASES["U"]
    iq = _capture("U")[0]
    raw = np.zeros(2 * 4096, np.int16)
    n, P, y, x, F, t0, T = iq.size, c["y"] * c["x"], c["y"], c["x"], c["F"], c["t0"], c["T"]
    nan, inf, dk = float("nan"), float("inf"), _dk(c)
    with D.Arenas(ctx) as A:
        d_iq, d_raw = A.input("iq", iq, 8), A.input("raw", raw, 0)
        d_st, d_sc = A.output("state", 4 * P, 4), A.output("score", 8 * N_TRIALS, 8)
        good = dict(iq=d_iq.addr, fmt=0, n=n, t0=t0, T=T, k=KAPPA_TRUE, F=F, y=y, x=x, alpha=0.0, state=d_st.addr)

        def fold(**kw):
            k = dict(good, **kw)
            _fold_d(ctx, C.c_void_p(k["iq"]), k["fmt"], 1.0, k["n"], k["t0"], k["T"], k["k"], k["F"], k["y"], k["x"], k["alpha"],
                    C.c_void_p(k["state"]))

        def scan(**kw):
            k = dict(dict(good, dk=dk, nt=N_TRIALS, score=d_sc.addr), **kw)
            _scan_d(ctx, C.c_void_p(k["iq"]), k["fmt"], 1.0, k["n"], k["t0"], k["T"], k["k"], k["dk"], k["nt"], k["F"], k["y"], k["x"],
                    C.c_void_p(k["score"]))

        bad_fold = [dict(iq=0), dict(state=0), dict(fmt=4), dict(fmt=-1), dict(y=0), dict(x=-3), dict(y=65536, x=32768), dict(n=1),
                    dict(n=1 << 31), dict(F=-1), dict(T=nan), dict(T=inf), dict(t0=nan), dict(t0=inf), dict(T=1.5), dict(t0=-0.5),
                    dict(k=nan), dict(k=inf), dict(k=-inf),
                    dict(F=F + 1), dict(t0=t0 + 20.0), dict(n=n - 20), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan),
                    dict(state=d_st.addr + 2), dict(iq=d_iq.addr + 4), dict(iq=d_raw.addr + 8, fmt=1, n=2048, F=1),
                    dict(iq=d_raw.addr + 4, fmt=2, n=2048, F=1)]
        bad_scan = [dict(iq=0), dict(score=0), dict(fmt=9), dict(y=0), dict(x=0), dict(n=0), dict(F=-2), dict(T=nan), dict(k=nan),
                    dict(k=inf), dict(dk=nan), dict(dk=inf), dict(dk=-inf), dict(T=1.0), dict(t0=-1.0), dict(nt=0), dict(nt=-1),
                    dict(nt=4097), dict(score=d_sc.addr + 4), dict(iq=d_iq.addr + 2), dict(iq=d_raw.addr + 2, fmt=3, n=2048, F=1),
                    dict(F=F + 1), dict(y=46341, x=46341)]
        for kw in bad_fold:
            with pytest.raises(AssertionError, match="invalid|cfold"):
                fold(**kw)
        for kw in bad_scan:
            with pytest.raises(AssertionError, match="invalid|cfold"):
                scan(**kw)
        fold(F=0)
        scan(F=0)
        assert ctx.lib.tsdr_cfold_iq_d(None, d_iq.ptr, 0, 1.0, n, t0, T, KAPPA_TRUE, F, y, x, 0.0, d_st.ptr) == -1
        assert ctx.lib.tsdr_cfold_scan_iq_d(None, d_iq.ptr, 0, 1.0, n, t0, T, 0.0, dk, N_TRIALS, F, y, x, d_sc.ptr) == -1
        A.check()
        assert np.array_equal(d_st.get(np.uint32), D.sentinel_words(d_st.size // 4)[d_st.lead // 4: (d_st.lead + d_st.payload) // 4])
        assert np.array_equal(d_sc.get(np.uint32), D.sentinel_words(d_sc.size // 4)[d_sc.lead // 4: (d_sc.lead + d_sc.payload) // 4])
        # and the context still serves valid calls afterwards: negative kappa and a negative step are accepted
        scan(k=-KAPPA_TRUE, dk=-dk)
        fold(k=-2.5)
        A.check()
        assert np.all(np.isfinite(d_sc.get(np.float64))) and np.all(np.isfinite(d_st.get(F32)))
    # host forms: the same refusals, host arrays untouched; F == 0 touches nothing
    st = np.full(P, 7.0, F32)
    sc = np.full(N_TRIALS, 7.0)
    best = C.c_int(-7)
    z = iq.copy()
    for kw in (dict(T=nan), dict(k=nan), dict(F=F + 1), dict(alpha=2.0), dict(fmt=5), dict(y=0), dict(F=0)):
        k = dict(good, **kw)
        rc = ctx.lib.tsdr_cfold_iq(ctx.h, C.c_void_p(z.ctypes.data), k["fmt"], 1.0, n, k["t0"], k["T"], k["k"], k["F"], k["y"], k["x"],
                                   k["alpha"], C.c_void_p(st.ctypes.data))
        assert rc == (0 if kw == dict(F=0) else -1), kw
    for kw in (dict(dk=inf), dict(nt=0), dict(F=F + 1), dict(T=1.0), dict(F=0)):
        k = dict(dict(good, dk=dk, nt=N_TRIALS), **kw)
        rc = ctx.lib.tsdr_cfold_scan_iq(ctx.h, C.c_void_p(z.ctypes.data), k["fmt"], 1.0, n, k["t0"], k["T"], k["k"], k["dk"], k["nt"], k["F"],
                                        k["y"], k["x"], C.c_void_p(sc.ctypes.data), C.byref(best))
        assert rc == (0 if kw == dict(F=0) else -1), kw
    assert np.all(st == 7.0) and np.all(sc == 7.0) and best.value == -7 and np.array_equal(z, iq)
