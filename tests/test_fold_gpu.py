"""GPU tests of coherent frame folding (include/tempest_hip_fold.h): the fold and the period scan against tests/fold_ref.py within the
contract's error bounds, against sig_to_image where the two coincide, format invariance and repeatability bit for bit, the period
ladder, the phase carried across buffers, and every refusal.  Every device pointer sits inside a guarded arena (tests/dptr_util.py):
`state` at 4, 8 and 12 mod 16, ComplexF32 `iq` at 0 and 8 mod 16.

Which case reaches which kernel (W = ceil(128 * T / P) + 3 against TSDR_FOLD_STAGE_MAX = 240; asserted by profile name):
    U  70 x 150, T 1207.73   W  18  fold_tile / fold_scan_tile   P/T = 8.69; partial second line tile, partial pixel tile
    M  66 x 160, T 9150.37   W 114  fold_tile / fold_scan_tile   P/T = 1.15
    D  77 x 131, T 11600.61  W 151  fold_tile / fold_scan_tile   P/T = 0.87; odd sizes; starts one period in
    S  20 x 140, T 5180.3    W 240  fold_tile / fold_scan_tile   the widest span the tiled kernel stages
    R  20 x 140, T 5195.3    W 241  fold_direct / fold_scan_direct   the narrowest span of the direct kernel
    X   8 x 16,  T 5000.5    W 5004 fold_direct / fold_scan_direct   39 samples per pixel

Captures and references are made once per case (functools caches); nothing modifies them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import dptr_util as D
import fold_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = {
    "U": dict(y=70, x=150, T=1207.73, F=7, t0=3.25),
    "M": dict(y=66, x=160, T=9150.37, F=5, t0=0.0),
    "D": dict(y=77, x=131, T=11600.61, F=4, t0=11599.9),
    "X": dict(y=8, x=16, T=5000.5, F=3, t0=0.5),
    "S": dict(y=20, x=140, T=5180.3, F=3, t0=1.5),
    "R": dict(y=20, x=140, T=5195.3, F=3, t0=1.5),
}
KERNEL = {"U": "tile", "M": "tile", "D": "tile", "S": "tile", "R": "direct", "X": "direct"}
STATE_PHASE = {"U": 4, "M": 8, "D": 12, "X": 4, "S": 8, "R": 12}
IQ_PHASE = {"U": 0, "M": 8, "D": 0, "X": 8, "S": 0, "R": 8}
N_TRIALS, DT = 9, 0.25


def _n(c):
    return int(math.ceil(c["t0"] + c["F"] * (c["T"] + 2.0))) + 5


@functools.lru_cache(maxsize=None)
def _capture(name, snr_db=20.0, extra=0):
    """(iq complex64[n], a float32[n]) of a case: Fs = 60 T, so one frame of the synthetic leak lasts exactly T samples"""
    from tempest_loader import load_package
    load_package()
    import importlib
    synth = importlib.import_module("tempestsdr_jl_amd.synth")
    c = CASES[name]
    iq = synth.synth_leak(60.0 * c["T"], c["x"], c["y"], 60.0, _n(c) + extra, snr_db=snr_db)
    a = R.amplitudes(iq)
    iq.setflags(write=False)
    a.setflags(write=False)
    return iq, a


@functools.lru_cache(maxsize=None)
def _ref_fold(name):
    c = CASES[name]
    return R.fold(_capture(name)[1], c["t0"], c["T"], c["F"], c["y"], c["x"])


@functools.lru_cache(maxsize=None)
def _ref_scan(name, snr_db):
    c = CASES[name]
    return R.scan(_capture(name, snr_db)[1], c["t0"], c["T"] - 6 * DT, DT, N_TRIALS, c["F"], c["y"], c["x"])


def _fill(ctx, arena, data):
    """put `data` into an OUTPUT arena's payload (a state the call may overwrite)"""
    d = np.ascontiguousarray(data)
    assert d.nbytes == arena.payload
    ctx.call("tsdr_upload", arena.ptr, C.c_void_p(d.ctypes.data), d.nbytes)


def _fold_d(ctx, iq, fmt, scale, n, t0, T, F, y, x, alpha, state):
    ctx.call("tsdr_fold_iq_d", iq, fmt, C.c_float(scale), n, C.c_double(t0), C.c_double(T), F, y, x, C.c_float(alpha), state)


def _scan_d(ctx, iq, fmt, scale, n, t0, T0, dT, nt, F, y, x, score):
    ctx.call("tsdr_fold_scan_iq_d", iq, fmt, C.c_float(scale), n, C.c_double(t0), C.c_double(T0), C.c_double(dT), nt, F, y, x, score)


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
    print(f"{what}: max error {err:.4g}, bound {bound:.4g}, ratio {err / bound:.3f}")


# ---------------------------------------------------------------- 1. the fold against the reference
@pytest.mark.parametrize("alpha", [0.0, 0.25])
@pytest.mark.parametrize("name", list(CASES))
def test_fold_matches_the_reference(ctx, name, alpha):
    """|state - ref| <= (F + 8) 2^-24 max(amax, max |state_in|).  alpha = 0 runs on an all-NaN state, which must not be read;
    alpha = 0.25 on a random positive state.  The kernel the case takes is asserted by its profile name."""
    c = CASES[name]
    iq, a = _capture(name)
    P = c["y"] * c["x"]
    if alpha == 0:
        st_in = np.full(P, np.nan, F32)
    else:
        st_in = np.random.default_rng(P).uniform(0.001, 0.02, P).astype(F32)
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, IQ_PHASE[name])
        d_st = A.output("state", 4 * P, STATE_PHASE[name])
        _fill(ctx, d_st, st_in)
        names = _profiled(ctx, lambda: _fold_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], c["T"], c["F"], c["y"], c["x"], alpha, d_st.ptr))
        A.check()
        got = d_st.get(F32)
    assert names == {"fold_" + KERNEL[name]}, names
    assert not np.isnan(got).any()
    ref = R.fold(a, c["t0"], c["T"], c["F"], c["y"], c["x"], alpha, st_in) if alpha else _ref_fold(name)
    bound = R.eps(c["F"], a.max(), 0.0 if alpha == 0 else st_in.max())
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    _report(f"fold {name} alpha {alpha}", err, bound)
    assert err <= bound, (name, alpha, err, bound)


def test_python_forms_agree_with_the_device_form(ctx):
    """Context.fold (host arrays, tsdr_fold_iq) and Context.fold_d give the bits of the call above; state comes back as (y_t, x_t)"""
    c = CASES["U"]
    iq, a = _capture("U")
    P = c["y"] * c["x"]
    host = ctx.fold(iq, c["t0"], c["T"], c["F"], c["y"], c["x"])
    assert host.shape == (c["y"], c["x"]) and host.dtype == F32
    with D.Arenas(ctx) as A:
        d_iq, d_st = A.input("iq", iq, 8), A.output("state", 4 * P, 12)
        ctx.fold_d(d_iq.addr, "cf32", 1.0, iq.size, c["t0"], c["T"], c["F"], c["y"], c["x"], 0.0, d_st.addr)
        A.check()
        dev = d_st.get(F32)
    assert np.array_equal(host.reshape(-1, order="F"), dev)
    assert np.max(np.abs(dev - _ref_fold("U"))) <= R.eps(c["F"], a.max())
    st = np.asfortranarray(np.random.default_rng(1).uniform(0.001, 0.01, (c["y"], c["x"])).astype(F32))
    keep = st.copy()
    out = ctx.fold(iq, c["t0"], c["T"], c["F"], c["y"], c["x"], alpha=0.5, state=st)
    assert np.array_equal(st, keep), "the caller's state is an input"
    ref = R.fold(a, c["t0"], c["T"], c["F"], c["y"], c["x"], 0.5, st.reshape(-1, order="F"))
    assert np.max(np.abs(out.reshape(-1, order="F") - ref)) <= R.eps(c["F"], a.max(), st.max())
    raw = np.full((c["y"], c["x"]), np.nan, F32, order="F")
    ctx.call("tsdr_fold_iq", C.c_void_p(iq.ctypes.data), 0, C.c_float(1.0), iq.size, C.c_double(c["t0"]), C.c_double(c["T"]), c["F"], c["y"],
             c["x"], C.c_float(0.0), C.c_void_p(raw.ctypes.data))
    assert np.array_equal(raw, host)


# ---------------------------------------------------------------- 2. against what exists
def test_one_frame_from_zero_is_sig_to_image(ctx):
    """F = 1, t0 = 0, T = n = S: the buffer clamp equals the frame clamp, and the fold is sig_to_image(amDemod(iq)) within eps(F = 1)
    = 9 * 2^-24 * amax -- at case U's geometry with S = 1208"""
    y, x, S = 70, 150, 1208
    iq = _capture("U")[0][:S].copy()
    before = ctx.precision
    ctx.set_precision("exact")
    try:
        want = ctx.sig_to_image(ctx.amDemod(iq), y, x)
    finally:
        ctx.set_precision(before)
    with D.Arenas(ctx) as A:
        d_iq, d_st = A.input("iq", iq, 8), A.output("state", 4 * y * x, 4)
        _fold_d(ctx, d_iq.ptr, 0, 1.0, S, 0.0, float(S), 1, y, x, 0.0, d_st.ptr)
        A.check()
        got = d_st.get(F32)
    bound = R.eps(1, np.abs(iq).max())
    err = float(np.max(np.abs(got.astype(np.float64) - want.reshape(-1, order="F").astype(np.float64))))
    _report("fold vs sig_to_image", err, bound)
    assert err <= bound


# ---------------------------------------------------------------- 3. formats
def _quantised(name, fmt):
    """(raw integer components, scale, expanded complex64) of a case's capture in an integer format"""
    import importlib
    from tempest_loader import load_package
    load_package()
    api = importlib.import_module("tempestsdr_jl_amd.api")
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
    """fold (cases U, D) and scan scores (case U): sc16 / sc8 / uc8 in, the bits of the same call on the host-expanded ComplexF32"""
    code = {"sc16": 1, "sc8": 2, "uc8": 3}[fmt]
    for name in ("U", "D"):
        c = CASES[name]
        raw, scale, z = _quantised(name, fmt)
        n, P = z.size, c["y"] * c["x"]
        T0 = c["T"] - 6 * DT
        with D.Arenas(ctx) as A:
            d_raw, d_z = A.input("raw", raw, 0), A.input("expanded", z, 8)
            s_raw, s_z = A.output("state raw", 4 * P, 4), A.output("state expanded", 4 * P, 12)
            k_raw, k_z = A.output("score raw", 8 * N_TRIALS, 8), A.output("score expanded", 8 * N_TRIALS, 0)
            _fold_d(ctx, d_raw.ptr, code, scale, n, c["t0"], c["T"], c["F"], c["y"], c["x"], 0.0, s_raw.ptr)
            _fold_d(ctx, d_z.ptr, 0, 1.0, n, c["t0"], c["T"], c["F"], c["y"], c["x"], 0.0, s_z.ptr)
            if name == "U":
                _scan_d(ctx, d_raw.ptr, code, scale, n, c["t0"], T0, DT, N_TRIALS, c["F"], c["y"], c["x"], k_raw.ptr)
                _scan_d(ctx, d_z.ptr, 0, 1.0, n, c["t0"], T0, DT, N_TRIALS, c["F"], c["y"], c["x"], k_z.ptr)
            A.check()
            a, b = s_raw.get(np.uint32), s_z.get(np.uint32)
            assert np.array_equal(a, b), (name, fmt, int(np.count_nonzero(a != b)))
            ref = R.fold(R.amplitudes(z), c["t0"], c["T"], c["F"], c["y"], c["x"])
            assert np.max(np.abs(s_z.get(F32) - ref)) <= R.eps(c["F"], np.abs(z).max()), "and they are the fold of that buffer"
            if name == "U":
                assert np.array_equal(k_raw.get(np.uint64), k_z.get(np.uint64)), (fmt, k_raw.get(np.float64), k_z.get(np.float64))
                assert np.all(k_z.get(np.float64) > 0)


# ---------------------------------------------------------------- 4. twice -> identical bits
@pytest.mark.parametrize("name", ["U", "D", "X"])
def test_two_calls_leave_identical_bits(ctx, name):
    c = CASES[name]
    iq = _capture(name)[0]
    P = c["y"] * c["x"]
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, IQ_PHASE[name])
        st = [A.output(f"state {k}", 4 * P, 4 + 8 * k) for k in range(2)]
        sc = [A.output(f"score {k}", 8 * N_TRIALS, 8 * k) for k in range(2)]
        for k in range(2):
            _fold_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], c["T"], c["F"], c["y"], c["x"], 0.0, st[k].ptr)
            _scan_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], c["T"] - 6 * DT, DT, N_TRIALS, c["F"], c["y"], c["x"], sc[k].ptr)
        A.check()
        assert np.array_equal(st[0].get(np.uint32), st[1].get(np.uint32))
        assert np.array_equal(sc[0].get(np.uint64), sc[1].get(np.uint64))
        assert np.all(np.isfinite(sc[0].get(np.float64)))


# ---------------------------------------------------------------- 5. the scan
@pytest.mark.parametrize("snr_db", [20.0, 0.0])
@pytest.mark.parametrize("name", ["U", "M", "D"])
def test_scan_scores_and_maximum(ctx, name, snr_db):
    """nine trials at a quarter sample, the true period at index 6: every score within 2 eps sqrt(P ref) + P eps^2 of the reference's,
    the first maximum where the reference puts it (index 6).  Precondition, on the reference: the top-2 relative margin is at least
    4 x the relative score bound, so a tie cannot hide a failure.  The host form returns the same scores and `best`."""
    c = CASES[name]
    iq, a = _capture(name, snr_db)
    P, T0 = c["y"] * c["x"], c["T"] - 6 * DT
    ref = _ref_scan(name, snr_db)
    e = R.eps(c["F"], a.max())
    bounds = np.array([R.score_bound(e, P, r) for r in ref])
    margin = R.top2_margin(ref)
    print(f"scan {name} {snr_db} dB: reference margin {margin:.4g}, relative bound {float(np.max(bounds / ref)):.4g}")
    assert R.first_max(ref) == 6 and margin >= 4 * float(np.max(bounds / ref)), (margin, bounds / ref)
    with D.Arenas(ctx) as A:
        d_iq, d_sc = A.input("iq", iq, IQ_PHASE[name]), A.output("score", 8 * N_TRIALS, 8)
        names = _profiled(ctx, lambda: _scan_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], T0, DT, N_TRIALS, c["F"], c["y"], c["x"], d_sc.ptr))
        A.check()
        got = d_sc.get(np.float64)
    assert names == {"fold_scan_tile", "fold_score"}, names
    _report(f"scan {name} {snr_db} dB", float(np.max(np.abs(got - ref) / bounds)), 1.0)
    assert np.all(np.abs(got - ref) <= bounds), (got, ref, bounds)
    assert R.first_max(got) == 6
    host, best = ctx.fold_scan(iq, c["t0"], T0, DT, N_TRIALS, c["F"], c["y"], c["x"])
    assert np.array_equal(host, got) and best == 6
    sc, b = np.zeros(N_TRIALS), C.c_int(-5)
    ctx.call("tsdr_fold_scan_iq", C.c_void_p(iq.ctypes.data), 0, C.c_float(1.0), iq.size, C.c_double(c["t0"]), C.c_double(T0), C.c_double(DT),
             N_TRIALS, c["F"], c["y"], c["x"], C.c_void_p(sc.ctypes.data), C.byref(b))
    assert np.array_equal(sc, got) and b.value == 6


def test_scan_on_the_direct_path(ctx):
    """case X (39 samples per pixel): the scan's direct kernel, scores within the bound; the trial periods T0 + k dT are the fold's"""
    c = CASES["X"]
    iq, a = _capture("X")
    P, T0 = c["y"] * c["x"], c["T"] - 6 * DT
    ref = _ref_scan("X", 20.0)
    e = R.eps(c["F"], a.max())
    with D.Arenas(ctx) as A:
        d_iq, d_sc, d_st = A.input("iq", iq, 8), A.output("score", 8 * N_TRIALS, 0), A.output("state", 4 * P, 4)
        names = _profiled(ctx, lambda: ctx.fold_scan_d(d_iq.addr, 0, 1.0, iq.size, c["t0"], T0, DT, N_TRIALS, c["F"], c["y"], c["x"], d_sc.addr))
        _fold_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], T0 + 3 * DT, c["F"], c["y"], c["x"], 0.0, d_st.ptr)
        A.check()
        got, pic = d_sc.get(np.float64), d_st.get(F32).astype(np.float64)
    assert names == {"fold_scan_direct", "fold_score"}, names
    assert np.all(np.abs(got - ref) <= [R.score_bound(e, P, r) for r in ref]), (got, ref)
    assert abs(got[3] - R.score_of(pic)) <= 1e-12 * got[3], "trial 3 scores the picture the fold leaves at T0 + 3 dT"


@pytest.mark.parametrize("name", ["S", "R"])
def test_scan_at_the_staging_boundary(ctx, name):
    """three trials at a quarter sample whose largest is the case's T: the scan makes the fold's choice at the boundary (W 240:
    fold_scan_tile, W 241: fold_scan_direct; 128 T / P = 236.8 and 237.5, so the rounding of T0 + 2 dT cannot move it), every score
    within the bound of the reference's.  No claim about the maximum: these cases carry no margin precondition."""
    c = CASES[name]
    iq, a = _capture(name)
    P, T0, nt = c["y"] * c["x"], c["T"] - 2 * DT, 3
    ref = R.scan(a, c["t0"], T0, DT, nt, c["F"], c["y"], c["x"])
    bounds = np.array([R.score_bound(R.eps(c["F"], a.max()), P, r) for r in ref])
    with D.Arenas(ctx) as A:
        d_iq, d_sc = A.input("iq", iq, IQ_PHASE[name]), A.output("score", 8 * nt, 8)
        names = _profiled(ctx, lambda: _scan_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], T0, DT, nt, c["F"], c["y"], c["x"], d_sc.ptr))
        A.check()
        got = d_sc.get(np.float64)
    assert names == {"fold_scan_" + KERNEL[name], "fold_score"}, names
    _report(f"scan {name} at the boundary", float(np.max(np.abs(got - ref) / bounds)), 1.0)
    assert np.all(np.abs(got - ref) <= bounds), (got, ref, bounds)


# ---------------------------------------------------------------- 6. refine_period
@pytest.mark.parametrize("name, want", [("U", 1207.71875), ("M", 9150.375)])
def test_refine_period_follows_the_reference_ladder(ctx, name, want):
    """defaults (17 trials at 1/8 sample, then at 1/32) from T_guess = round(T): T_hat is the reference ladder's pick, within a
    sixteenth of a sample of T.  Precondition, on the reference: every level's top-2 margin >= 1e-4."""
    c = CASES[name]
    iq, a = _capture(name)
    T_ref, last_ref, levels = R.ladder(a, round(c["T"]), c["F"], c["y"], c["x"])
    assert all(R.top2_margin(s) >= 1e-4 for s in levels), [R.top2_margin(s) for s in levels]
    assert T_ref == want and last_ref == 0.03125
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, IQ_PHASE[name])
        T_hat, last, scores = ctx.refine_period(d_iq.addr, "cf32", 1.0, iq.size, round(c["T"]), c["F"], c["y"], c["x"])
        A.check()
    assert T_hat == want and last == 0.03125 and abs(T_hat - c["T"]) <= 0.0625
    assert len(scores) == 2 and all(s.shape == (17,) for s in scores)
    e = R.eps(c["F"], a.max())
    for s, r in zip(scores, levels):
        assert np.all(np.abs(s - r) <= [R.score_bound(e, c["y"] * c["x"], v) for v in r])


# ---------------------------------------------------------------- 7. the phase carried across buffers
def test_phase_carries_across_buffers(ctx):
    """One capture of case M, 3.4 frames longer (8 whole frames), against the same capture cut after the case's n1 samples and
    chained by fold_plan: buffer 1 holds frames 0 .. 4 (alpha = 0), frame 5 straddles the cut and is skipped, buffer 2 holds frames
    6, 7 at the carried t0 and is averaged in with alpha = 5/7, which makes the state the mean of the seven frames.

    The long buffer gives the same seven frames as (8 L - S5) / 7, L = its fold over F = 8, S5 = its fold of frame 5 alone.  With
    e(F) = (F + 8) 2^-24 amax:  |L - ref| <= e(8) and |S5 - ref| <= e(1), so that side is within (8 e(8) + e(1)) / 7; the chained side
    is within alpha e(5) (the first call's error, scaled by the IIR) + e(2) (the second call, whose state_in <= amax) + 2^-24 amax
    (alpha = f32(5/7) instead of 5/7).  The two sides agree within the sum."""
    from tempest_loader import load_package
    plan = load_package().fold_plan
    c = CASES["M"]
    T, y, x = c["T"], c["y"], c["x"]
    P, n1 = y * x, _n(c)
    n_long = int(math.ceil(8.4 * T)) + 5
    iq, a = _capture("M", 20.0, n_long - n1)
    assert iq.size == n_long and plan(n_long, 0.0, T)[0] == 8
    F1, t1 = plan(n1, 0.0, T)
    F2, t2 = plan(n_long - n1, t1, T)
    assert (F1, F2) == (5, 2) and abs((n1 + t1) - 6 * T) < 1e-9 and 0 < t2 <= T
    alpha = F1 / (F1 + F2)
    with D.Arenas(ctx) as A:
        d_long = A.input("long", iq, 8)
        d_a, d_b = A.input("first", iq[:n1], 0), A.input("second", iq[n1:], 8)
        s_long, s_5, s_ch = A.output("L", 4 * P, 4), A.output("S5", 4 * P, 8), A.output("chained", 4 * P, 12)
        _fold_d(ctx, d_long.ptr, 0, 1.0, n_long, 0.0, T, 8, y, x, 0.0, s_long.ptr)
        _fold_d(ctx, d_long.ptr, 0, 1.0, n_long, 5 * T, T, 1, y, x, 0.0, s_5.ptr)
        _fold_d(ctx, d_a.ptr, 0, 1.0, n1, 0.0, T, F1, y, x, 0.0, s_ch.ptr)
        _fold_d(ctx, d_b.ptr, 0, 1.0, n_long - n1, t1, T, F2, y, x, alpha, s_ch.ptr)
        A.check()
        L, S5, ch = (s.get(F32).astype(np.float64) for s in (s_long, s_5, s_ch))
    amax = float(a.max())
    e = lambda F: R.eps(F, amax)   # noqa: E731
    bound = (8 * e(8) + e(1)) / 7 + alpha * e(5) + e(2) + R.ULP * amax
    err = float(np.max(np.abs((8 * L - S5) / 7 - ch)))
    _report("phase carry", err, bound)
    assert err <= bound
    # and both are the seven shared frames of the reference
    ref7 = (8 * R.fold(a, 0.0, T, 8, y, x) - R.fold(a, 5 * T, T, 1, y, x)) / 7
    assert np.max(np.abs(ch - ref7)) <= alpha * e(5) + e(2) + R.ULP * amax


# ---------------------------------------------------------------- 8. refusals and untouched memory
def test_refusals_leave_everything_untouched(ctx):
    """every TSDR_EINVAL of the header, and F == 0 (TSDR_OK): the sentinels around iq, state and score, and the sentinel-filled state
    and score themselves, are as uploaded; iq is never written"""
    c = CASES["U"]
    iq = _capture("U")[0]
    raw = np.zeros(2 * 4096, np.int16)
    n, P, y, x, F, t0, T = iq.size, c["y"] * c["x"], c["y"], c["x"], c["F"], c["t0"], c["T"]
    nan, inf = float("nan"), float("inf")
    with D.Arenas(ctx) as A:
        d_iq, d_raw = A.input("iq", iq, 8), A.input("raw", raw, 0)
        d_st, d_sc = A.output("state", 4 * P, 4), A.output("score", 8 * N_TRIALS, 8)
        good = dict(iq=d_iq.addr, fmt=0, n=n, t0=t0, T=T, F=F, y=y, x=x, alpha=0.0, state=d_st.addr)

        def fold(**kw):
            k = dict(good, **kw)
            _fold_d(ctx, C.c_void_p(k["iq"]), k["fmt"], 1.0, k["n"], k["t0"], k["T"], k["F"], k["y"], k["x"], k["alpha"], C.c_void_p(k["state"]))

        def scan(**kw):
            k = dict(dict(good, dT=DT, nt=N_TRIALS, score=d_sc.addr), **kw)
            _scan_d(ctx, C.c_void_p(k["iq"]), k["fmt"], 1.0, k["n"], k["t0"], k["T"], k["dT"], k["nt"], k["F"], k["y"], k["x"], C.c_void_p(k["score"]))

        bad_fold = [dict(iq=0), dict(state=0), dict(fmt=4), dict(fmt=-1), dict(y=0), dict(x=-3), dict(y=65536, x=32768), dict(n=1),
                    dict(n=1 << 31), dict(F=-1), dict(T=nan), dict(T=inf), dict(t0=nan), dict(t0=inf), dict(T=1.5), dict(t0=-0.5),
                    dict(F=F + 1), dict(t0=t0 + 20.0), dict(n=n - 20), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan),
                    dict(state=d_st.addr + 2), dict(iq=d_iq.addr + 4), dict(iq=d_raw.addr + 8, fmt=1, n=2048, F=1),
                    dict(iq=d_raw.addr + 4, fmt=2, n=2048, F=1)]
        bad_scan = [dict(iq=0), dict(score=0), dict(fmt=9), dict(y=0), dict(x=0), dict(n=0), dict(F=-2), dict(T=nan), dict(dT=nan),
                    dict(dT=inf), dict(dT=-0.25), dict(T=1.0), dict(t0=-1.0), dict(nt=0), dict(nt=-1), dict(nt=4097),
                    dict(score=d_sc.addr + 4), dict(iq=d_iq.addr + 2), dict(iq=d_raw.addr + 2, fmt=3, n=2048, F=1),
                    dict(T=T + 2.0 - 7 * DT, dT=DT, nt=9, n=int(math.ceil(t0 + F * (T + 2.0)))),   # only the largest trial overruns
                    dict(y=46341, x=46341)]
        for kw in bad_fold:
            with pytest.raises(AssertionError, match="invalid|fold"):
                fold(**kw)
        for kw in bad_scan:
            with pytest.raises(AssertionError, match="invalid|fold"):
                scan(**kw)
        fold(F=0)
        scan(F=0)
        assert ctx.lib.tsdr_fold_iq_d(None, d_iq.ptr, 0, 1.0, n, t0, T, F, y, x, 0.0, d_st.ptr) == -1
        assert ctx.lib.tsdr_fold_scan_iq_d(None, d_iq.ptr, 0, 1.0, n, t0, T, DT, N_TRIALS, F, y, x, d_sc.ptr) == -1
        A.check()
        assert np.array_equal(d_st.get(np.uint32), D.sentinel_words(d_st.size // 4)[d_st.lead // 4: (d_st.lead + d_st.payload) // 4])
        assert np.array_equal(d_sc.get(np.uint32), D.sentinel_words(d_sc.size // 4)[d_sc.lead // 4: (d_sc.lead + d_sc.payload) // 4])
        # and the context still serves a valid call afterwards
        scan(T=T - 6 * DT)
        A.check()
    # host forms: the same refusals, host arrays untouched; F == 0 touches nothing
    st = np.full(P, 7.0, F32)
    sc = np.full(N_TRIALS, 7.0)
    best = C.c_int(-7)
    z = iq.copy()
    for kw in (dict(T=nan), dict(F=F + 1), dict(alpha=2.0), dict(fmt=5), dict(y=0), dict(F=0)):
        k = dict(good, **kw)
        rc = ctx.lib.tsdr_fold_iq(ctx.h, C.c_void_p(z.ctypes.data), k["fmt"], 1.0, n, k["t0"], k["T"], k["F"], k["y"], k["x"], k["alpha"],
                                  C.c_void_p(st.ctypes.data))
        assert rc == (0 if kw == dict(F=0) else -1), kw
    for kw in (dict(dT=-1.0), dict(nt=0), dict(F=F + 1), dict(T=1.0), dict(F=0)):
        k = dict(dict(good, dT=DT, nt=N_TRIALS), **kw)
        rc = ctx.lib.tsdr_fold_scan_iq(ctx.h, C.c_void_p(z.ctypes.data), k["fmt"], 1.0, n, k["t0"], k["T"], k["dT"], k["nt"], k["F"], k["y"],
                                       k["x"], C.c_void_p(sc.ctypes.data), C.byref(best))
        assert rc == (0 if kw == dict(F=0) else -1), kw
    assert np.all(st == 7.0) and np.all(sc == 7.0) and best.value == -7 and np.array_equal(z, iq)
