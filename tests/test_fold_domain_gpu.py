"""GPU tests of the fold family over its accepted domain: every case of tests/fold_domain_cases.py (one pixel, one line, one column,
clamps that bind at both ends of the buffer, t0 + F T == n, positions on the integer grid, single and ragged tiles, 1500 frames, a
frame origin above 2^24 samples) through the eight device entry points -- tsdr_fold_iq_d, tsdr_fold_scan_iq_d, tsdr_cfold_iq_d,
tsdr_cfold_scan_iq_d, tsdr_cstack_iq_d, tsdr_ctrack_stack_iq_d, tsdr_ctrack_probe_iq_d, tsdr_ctrack_gram_iq_d -- against the numpy
references (fold_ref, cfold_ref, cstack_ref, ctrack_ref, gram_ref) within the bounds the headers state.  No tolerance is new: the call
helpers, _report and _check_info are the existing GPU modules'.  tests/test_fold_domain_host.py proves on the CPU that each case
meets the condition it is there for.

Every call: the launched kernels by profile name, exactly, against the table's route; finite outputs; every device pointer inside
a guarded arena (tests/dptr_util.py), checked afterwards; and once per entry point and case the same call again, bit for bit.

The IQ buffer ends where its arena's guard begins, so a load past sample n - 1 reads no sample.  The guard words are finite on
purpose (about -5e5 as f32): a tap there with a positive weight is a gross error -- but one with weight 0, which is what a tap index
clamped at n - 1 instead of n - 2 produces, would vanish in the blend.  A ComplexF32 buffer therefore carries one NaN sample as the
first element of its guard (the call is told n, the arena holds n + 1): any load of sample n, whatever its weight, makes an output
NaN.  The integer formats have no NaN: sc16 and an even number of 8-bit samples end at the guard words; an odd number of 8-bit samples
is padded to a whole word with one sample of a code the data never takes (fold_domain_cases.PAD_CODE).

FAR's references run on the window its frames touch (fold_domain_cases.window); every per-term bound then grows by
far_term = 2 amax n 2^-52, printed with each figure: added to the bounds that are a per-term error themselves, and carried into the
composite ones (scores, rho, E, the matrix) through their eps_z or eps_t, by widening the amax those are proportional to."""
import functools
import math

import numpy as np
import pytest

import cfold_ref as CF
import cstack_ref as CS
import ctrack_ref as TR
import dptr_util as D
import fold_domain_cases as K
import fold_ref as FR
import gram_ref as GR
import test_cfold_gpu as TC
import test_fold_gpu as TF
from test_cstack_gpu import MODE_NAME, _case_d, _check_info, _fill, _null, _pkg, _profiled, _report
from test_ctrack_gpu import _case_probe, _case_stack
from test_gram_gpu import _gram_d

pytestmark = pytest.mark.gpu

F32, C64 = np.float32, np.complex64
CASES, KAPPA = K.CASES, K.KAPPA_TRUE
GIVEN, LOCK = CS.GIVEN, CS.LOCK
PHI = 0.37
ULP = FR.ULP
NAN_SAMPLE = np.array([complex(np.nan, np.nan)], C64)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """what the references of a case share: the converted samples of its window (complex128), their f32 magnitudes, the two amax, the
    case counted from its window, and FAR's term per unit of amax"""
    c = CASES[name]
    z = K.samples(name)
    a = FR.amplitudes(z)
    zz = CF.samples(z)
    return dict(z=zz, a=a, a_max=float(a.max()), amax=float(np.abs(zz).max()), cw=K.windowed(c), far=K.far_term(c, 1.0))


def _wide(r, amax, coeff):
    """amax such that a per-term bound coeff * amax has grown by far_term(amax): for the composite bounds of FAR; amax itself elsewhere"""
    return amax * (1.0 + r["far"] / coeff)


def _iq(A, name):
    """the case's buffer in a guarded arena -> (pointer, format code, scale, n)"""
    c = CASES[name]
    if c["fmt"] == "sc8":
        return A.input("iq", K.padded(K.raw_sc8(name), "sc8"), 0).ptr, K.FMT_CODE["sc8"], K.SC8_SCALE, c["n"]
    return A.input("iq", np.concatenate([K.samples(name), NAN_SAMPLE]), 8 * (K.ALL.index(name) % 2)).ptr, 0, 1.0, c["n"]


def _run(ctx, want, fn):
    names = _profiled(ctx, fn)
    assert names == want, (names, want)


def _same_bits(a, b):
    assert np.array_equal(a.get(np.uint32), b.get(np.uint32)), (a.name, b.name)


def _finite(*arrays):
    for x in arrays:
        x = np.asarray(x)
        assert np.isfinite(x.view(x.real.dtype) if x.dtype.kind == "c" else x).all()


# ---------------------------------------------------------------- 1. the envelope fold and its period scan
@pytest.mark.parametrize("name", K.ALL)
def test_fold_and_period_scan(ctx, name):
    """tsdr_fold_iq_d at alpha 0 on an all-NaN state and at alpha 0.25 on a random positive state within eps = (F + 8) u max(amax,
    max |state_in|); tsdr_fold_scan_iq_d at T - 0.25, T - 0.125, T -- the largest trial ends at n -- within 2 eps sqrt(P ref) + P eps^2.
    P1's smallest trial would be 1.75 < 2: that scan is refused, as the header says, and P1 scans T three times (dT = 0)."""
    c, r = CASES[name], _ref(name)
    cw, y, x, F, T, P = r["cw"], c["y"], c["x"], c["F"], c["T"], c["y"] * c["x"]
    kern = c["envelope"]
    st_in = np.random.default_rng(P).uniform(0.001, 0.02, P).astype(F32)
    T0, dT = (T, 0.0) if name == "P1" else (T - 0.25, 0.125)
    with D.Arenas(ctx) as A:
        iq, fmt, scale, n = _iq(A, name)
        s0, s0b, s1 = A.output("state", 4 * P, 4), A.output("state again", 4 * P, 12), A.output("state alpha", 4 * P, 8)
        sc, scb = A.output("score", 24, 8), A.output("score again", 24, 0)
        for a in (s0, s0b):
            _fill(ctx, a, np.full(P, np.nan, F32))
        _fill(ctx, s1, st_in)
        for a, alpha in ((s0, 0.0), (s0b, 0.0), (s1, 0.25)):
            _run(ctx, {"fold_" + kern}, lambda: TF._fold_d(ctx, iq, fmt, scale, n, c["t0"], T, F, y, x, alpha, a.ptr))
        if name == "P1":
            with pytest.raises(AssertionError, match="invalid|fold"):
                TF._scan_d(ctx, iq, fmt, scale, n, c["t0"], T - 0.25, 0.125, 3, F, y, x, sc.ptr)
        for a in (sc, scb):
            _run(ctx, {"fold_scan_" + kern, "fold_score"}, lambda: TF._scan_d(ctx, iq, fmt, scale, n, c["t0"], T0, dT, 3, F, y, x, a.ptr))
        A.check()
        _same_bits(s0, s0b)
        _same_bits(sc, scb)
        got0, got1, score = s0.get(F32), s1.get(F32), sc.get(np.float64)
    _finite(got0, got1, score)
    extra = r["far"] * r["a_max"]
    for got, alpha in ((got0, 0.0), (got1, 0.25)):
        ref = FR.fold(r["a"], cw["t0"], T, F, y, x, alpha, st_in)
        bound = FR.eps(F, r["a_max"], st_in.max() if alpha else 0.0) + extra
        _report(f"domain {name} fold alpha {alpha} (far term {extra:.3g})", float(np.max(np.abs(got.astype(np.float64) - ref))), bound)
        assert np.max(np.abs(got.astype(np.float64) - ref)) <= bound
    ref = FR.scan(r["a"], cw["t0"], T0, dT, 3, F, y, x)
    bounds = np.array([FR.score_bound(FR.eps(F, r["a_max"]) + extra, P, v) for v in ref])
    _report(f"domain {name} fold scan", float(np.max(np.abs(score - ref) / bounds)), 1.0)
    assert np.all(np.abs(score - ref) <= bounds), (score, ref, bounds)


# ---------------------------------------------------------------- 2. the coherent fold and its carrier scan
@pytest.mark.parametrize("name", K.ALL)
def test_cfold_and_carrier_scan(ctx, name):
    """tsdr_cfold_iq_d at kappa_true, alpha 0 on NaN and alpha 0.25, within eps_c; tsdr_cfold_scan_iq_d over 9 values of kappa spaced
    1 / (8 F) around kappa_true (a ragged second batch) within 2 eps_z sqrt(P ref) + P eps_z^2"""
    c, r = CASES[name], _ref(name)
    cw, y, x, F, T, P = r["cw"], c["y"], c["x"], c["F"], c["T"], c["y"] * c["x"]
    kern = c["coherent"]
    st_in = np.random.default_rng(P).uniform(0.001, 0.02, P).astype(F32)
    dk = 1.0 / (8 * F)
    k0 = KAPPA - 4 * dk
    with D.Arenas(ctx) as A:
        iq, fmt, scale, n = _iq(A, name)
        s0, s0b, s1 = A.output("state", 4 * P, 12), A.output("state again", 4 * P, 4), A.output("state alpha", 4 * P, 8)
        sc, scb = A.output("score", 72, 8), A.output("score again", 72, 0)
        for a in (s0, s0b):
            _fill(ctx, a, np.full(P, np.nan, F32))
        _fill(ctx, s1, st_in)
        for a, alpha in ((s0, 0.0), (s0b, 0.0), (s1, 0.25)):
            _run(ctx, {"cfold_" + kern}, lambda: TC._fold_d(ctx, iq, fmt, scale, n, c["t0"], T, KAPPA, F, y, x, alpha, a.ptr))
        for a in (sc, scb):
            _run(ctx, {"cfold_scan_" + kern, "cfold_score"}, lambda: TC._scan_d(ctx, iq, fmt, scale, n, c["t0"], T, k0, dk, 9, F, y, x, a.ptr))
        A.check()
        _same_bits(s0, s0b)
        _same_bits(sc, scb)
        got0, got1, score = s0.get(F32), s1.get(F32), sc.get(np.float64)
    _finite(got0, got1, score)
    extra = r["far"] * r["amax"]
    for got, alpha in ((got0, 0.0), (got1, 0.25)):
        ref = CF.cfold(r["z"], cw["t0"], T, KAPPA, F, y, x, alpha, st_in)
        bound = CF.eps_c(F, r["amax"], st_in.max() if alpha else 0.0) + extra
        _report(f"domain {name} cfold alpha {alpha} (far term {extra:.3g})", float(np.max(np.abs(got.astype(np.float64) - ref))), bound)
        assert np.max(np.abs(got.astype(np.float64) - ref)) <= bound
    ref = CF.scan(r["z"], cw["t0"], T, k0, dk, 9, F, y, x)
    bounds = np.array([CF.score_bound(CF.eps_z(F, r["amax"]) + extra, P, v) for v in ref])
    _report(f"domain {name} cfold scan", float(np.max(np.abs(score - ref) / bounds)), 1.0)
    assert np.all(np.abs(score - ref) <= bounds), (score, ref, bounds)


# ---------------------------------------------------------------- 3. the stack
def _check_stack(what, r, F, P, mode, alpha, Z, S_in, zs, mag, info):
    """zstate, mag and info of one stacking call against cstack_ref.step within tempest_hip_cstack.h's bounds (ACCURACY), as
    tests/test_cstack_gpu.py's test_both_modes_match_the_reference asserts them"""
    _finite(zs, mag, info)
    zs, mag = zs.astype(np.complex128), mag.astype(np.float64)
    M = 0.0 if alpha == 0 else float(np.abs(S_in.astype(np.complex128)).max())
    ref, ref_info = CS.step(Z, alpha, mode, None if alpha == 0 else S_in.astype(np.complex128))
    extra = r["far"] * r["amax"]
    e_rho, rho_abs = _check_info(what, info, ref_info, F, _wide(r, r["amax"], math.sqrt(2.0) * (F + 12) * ULP), P)
    if mode == GIVEN:
        b_s, b_m = CS.eps_s(F, r["amax"], M) + extra, CS.eps_mag(F, r["amax"], M) + extra
        assert (info[6], info[7]) == (1.0, 0.0)
    else:
        b_s, b_m = CS.eps_lock(F, r["amax"], M, e_rho, rho_abs) + extra, CS.eps_lock_mag(F, r["amax"], M, e_rho, rho_abs) + extra
        if rho_abs:
            q = complex(info[0], info[1]) / math.hypot(info[0], info[1])
            assert abs(complex(info[6], info[7]) - q) <= 2.0 ** -23, "q is the direction of the record's own rho, rounded to f32"
    err_s, err_m = float(np.max(np.abs(zs - ref))), float(np.max(np.abs(mag - np.abs(ref))))
    _report(f"{what} zstate (far term {extra:.3g})", err_s, b_s)
    _report(f"{what} mag", err_m, b_m)
    assert err_s <= b_s and err_m <= b_m, (what, err_s, b_s, err_m, b_m)
    return ref_info


@pytest.mark.parametrize("name", K.ALL)
def test_cstack_given_then_lock(ctx, name):
    """tsdr_cstack_iq_d at (kappa_true, phi 0.37): GIVEN at alpha 0 on a NaN zstate, then LOCK at alpha 0.25 onto the state that call
    left -- Z against itself, so rho_ref = E_z: positive in every case, P1's single pixel included (its samples are not zero)"""
    c, r = CASES[name], _ref(name)
    cw, y, x, F, T, P = r["cw"], c["y"], c["x"], c["F"], c["T"], c["y"] * c["x"]
    kern = c["coherent"]
    Z = CS.zmean(r["z"], cw["t0"], T, KAPPA, PHI, F, y, x)
    with D.Arenas(ctx) as A:
        iq, fmt, scale, n = _iq(A, name)
        outs = [[A.output(f"zstate {k}", 8 * P, 8 * k), A.output(f"mag {k}", 4 * P, 4 + 8 * k), A.output(f"info {k}", 64, 8 * k)] for k in range(2)]
        for mode, alpha in ((GIVEN, 0.0), (LOCK, 0.25)):
            want = {"cstack_" + kern, "cstack_lock"} | ({"cstack_blend"} if mode == LOCK else set())
            S_in = np.full(P, np.nan + 1j * np.nan, C64) if alpha == 0 else outs[0][0].get(C64)
            for o in outs:
                _fill(ctx, o[0], S_in)
                _run(ctx, want, lambda: _case_d(ctx, c, iq, n, PHI, alpha, mode, o[0].ptr, o[1].ptr, o[2].ptr, fmt=fmt, scale=scale))
            A.check()
            for a, b in zip(*outs):
                _same_bits(a, b)
            info = _check_stack(f"domain {name} cstack {MODE_NAME[mode]}", r, F, P, mode, alpha, Z, S_in, outs[0][0].get(C64),
                                outs[0][1].get(F32), outs[0][2].get(np.float64))
            if mode == LOCK:
                assert info[5] >= 0.99, "the state is the call's own picture"


# ---------------------------------------------------------------- 4. the tracked stack and the probe
@pytest.mark.parametrize("name", K.ALL)
def test_ctrack_stack_and_probe(ctx, name):
    """tsdr_ctrack_stack_iq_d along the test track (GIVEN, alpha 0, a NaN zstate) within cstack's bounds; tsdr_ctrack_probe_iq_d of
    every frame against that zstate, with the NULL track and with the test track: rho_f, E_f and E_s within tempest_hip_ctrack.h, 9.,
    gamma_f consistent with the record's own sums.  The frames are noise around 0.5: a frame's coherence with the stack of F of them is
    near 1 / sqrt(F), and what the comparison sees is absolute -- one wrong sample moves rho_f by |S(m)|, far outside eps_rho."""
    c, r = CASES[name], _ref(name)
    cw, y, x, F, T, P = r["cw"], c["y"], c["x"], c["F"], c["T"], c["y"] * c["x"]
    kern = c["coherent"]
    track = K.track(c)
    n_out = 8 * (4 * F + 1)
    with D.Arenas(ctx) as A:
        iq, fmt, scale, n = _iq(A, name)
        d_tr = A.input("track", track, 8)
        outs = [[A.output(f"zstate {k}", 8 * P, 8 * k), A.output(f"mag {k}", 4 * P, 4 + 8 * k), A.output(f"info {k}", 64, 8 * k)] for k in range(2)]
        for o in outs:
            _fill(ctx, o[0], np.full(P, np.nan + 1j * np.nan, C64))
            _run(ctx, {"ctrack_stack_" + kern, "cstack_lock"},
                 lambda: _case_stack(ctx, c, iq, n, d_tr.ptr, 0.0, GIVEN, o[0].ptr, o[1].ptr, o[2].ptr, fmt=fmt, scale=scale))
        p_null, p_trk, p_again = A.output("out NULL", n_out, 8), A.output("out track", n_out, 0), A.output("out track again", n_out, 8)
        for o, tr in ((p_null, _null()), (p_trk, d_tr.ptr), (p_again, d_tr.ptr)):
            _run(ctx, {"ctrack_probe_" + kern, "ctrack_probe_sum"},
                 lambda: _case_probe(ctx, c, iq, n, tr, outs[0][0].ptr, o.ptr, fmt=fmt, scale=scale))
        A.check()
        for a, b in zip(*outs):
            _same_bits(a, b)
        _same_bits(p_trk, p_again)
        S = outs[0][0].get(C64)
        _check_stack(f"domain {name} ctrack stack", r, F, P, GIVEN, 0.0, TR.zmean(r["z"], cw["t0"], T, track, F, y, x), None, S,
                     outs[0][1].get(F32), outs[0][2].get(np.float64))
        records = {"NULL": p_null.get(np.float64), "track": p_trk.get(np.float64)}
    amax_t = _wide(r, r["amax"], math.sqrt(2.0) * TR.TERM * ULP)
    for tag, out in records.items():
        _finite(out)
        rho, E_f, gamma, E_s = TR.probe(r["z"], cw["t0"], T, track if tag == "track" else None, F, y, x, S.astype(np.complex128))
        g_rho, g_E, g_gamma, g_Es = _pkg("ctrack").probe_record(out, F)
        assert E_s > 0 and abs(g_Es - E_s) <= TR.eps_es(E_s), (g_Es, E_s)
        worst = [0.0, 0.0]
        for f in range(F):
            b_rho, b_E = TR.eps_rho(amax_t, P, E_f[f], E_s), TR.eps_ef(amax_t, P, E_f[f])
            worst = [max(worst[0], abs(g_rho[f] - rho[f]) / b_rho), max(worst[1], abs(g_E[f] - E_f[f]) / b_E)]
            assert abs(g_rho[f] - rho[f]) <= b_rho and abs(g_E[f] - E_f[f]) <= b_E, (name, tag, f, abs(g_rho[f] - rho[f]), b_rho,
                                                                                      abs(g_E[f] - E_f[f]), b_E)
            assert g_E[f] > 0 and abs(g_gamma[f] - abs(g_rho[f]) / math.sqrt(g_E[f] * g_Es)) <= 1e-12
            # gamma = |rho| (E_f E_s)^(-1/2), as tests/test_ctrack_gpu.py bounds it
            b_gamma = 1.01 * gamma[f] * (b_rho / abs(rho[f]) + 0.5 * b_E / E_f[f] + 0.5 * TR.eps_es(E_s) / E_s) + 1e-12
            assert abs(g_gamma[f] - gamma[f]) <= b_gamma, (name, tag, f, g_gamma[f], gamma[f], b_gamma)
        print(f"domain {name} ctrack probe {tag} (far term {r['far'] * r['amax']:.3g}): max |rho_f - ref| / bound {worst[0]:.3f}, "
              f"max |E_f - ref| / bound {worst[1]:.3f}")


# ---------------------------------------------------------------- 5. the Gram matrix
@pytest.mark.parametrize("name", K.ALL)
def test_gram(ctx, name):
    """tsdr_ctrack_gram_iq_d with the NULL track and the test track: every entry within tempest_hip_gram.h's bound, G[g][f] the bits of
    conj(G[f][g]), Im of the diagonal +0.  LONG's 1500 frames are refused (F > 64) with nothing launched and nothing written; its
    matrix is that of its first 64 frames"""
    c, r = CASES[name], _ref(name)
    cw, y, x, T, P = r["cw"], c["y"], c["x"], c["T"], c["y"] * c["x"]
    F = min(c["F"], K.GRAM_MAX_FRAMES)
    kern = c["coherent"]
    track = K.track(c, F)
    amax_t = _wide(r, r["amax"], math.sqrt(2.0) * TR.TERM * ULP)
    with D.Arenas(ctx) as A:
        iq, fmt, scale, n = _iq(A, name)
        d_tr = A.input("track", track, 8)
        g_null, g_trk, g_again = A.output("gram NULL", 16 * F * F, 8), A.output("gram track", 16 * F * F, 0), A.output("gram again", 16 * F * F, 8)
        if c["F"] > K.GRAM_MAX_FRAMES:
            d_all = A.input("track of every frame", K.track(c), 8)

            def refused():
                with pytest.raises(AssertionError, match="invalid|ctrack_gram"):
                    _gram_d(ctx, iq, fmt, scale, n, c["t0"], T, d_all.ptr, c["F"], y, x, g_trk.ptr)
            _run(ctx, set(), refused)
            A.check()
            assert np.array_equal(g_trk.get(np.uint32), D.sentinel_words(g_trk.size // 4)[g_trk.lead // 4: (g_trk.lead + g_trk.payload) // 4])
        for o, tr in ((g_null, _null()), (g_trk, d_tr.ptr), (g_again, d_tr.ptr)):
            _run(ctx, {"gram_" + kern, "gram_sum"}, lambda: _gram_d(ctx, iq, fmt, scale, n, c["t0"], T, tr, F, y, x, o.ptr))
        A.check()
        _same_bits(g_trk, g_again)
        got = {"NULL": (g_null.get(np.uint64).reshape(F, F, 2), _pkg("gram").gram_matrix(g_null.get(np.float64), F)),
               "track": (g_trk.get(np.uint64).reshape(F, F, 2), _pkg("gram").gram_matrix(g_trk.get(np.float64), F))}
    sign = np.uint64(1) << np.uint64(63)
    for tag, (raw, G) in got.items():
        _finite(G)
        ref = GR.gram(r["z"], cw["t0"], T, track if tag == "track" else None, F, y, x)
        ratio = np.abs(G - ref) / GR.eps_matrix(amax_t, P, ref)
        print(f"domain {name} gram {tag} (far term {r['far'] * r['amax']:.3g}): max |G - ref| / bound {ratio.max():.4f} "
              f"(diagonal {np.diag(ratio).max():.4f})")
        assert np.all(ratio <= 1.0), (name, tag, float(ratio.max()))
        for f in range(F):
            assert raw[f, f, 1] == 0 and G[f, f].real > 0, "Im G[f][f] is +0"
            for g in range(f):
                assert raw[g, f, 0] == raw[f, g, 0] and raw[g, f, 1] == raw[f, g, 1] ^ sign, (f, g)


# ---------------------------------------------------------------- 6. integer formats under binding clamps
@pytest.mark.parametrize("fmt", ["sc16", "sc8", "uc8"])
@pytest.mark.parametrize("name", K.FORMAT_CASES)
def test_integer_formats_give_the_bits_of_the_expanded_buffer(ctx, name, fmt):
    """FORMAT INVARIANCE where the clamps bind (UPS: five pixels at either end, staged; INT: every d exactly 0 or 1, direct):
    tsdr_cfold_iq_d, tsdr_ctrack_probe_iq_d and tsdr_ctrack_gram_iq_d on sc16 / sc8 / uc8 leave the bits of the same call on the
    host-expanded ComplexF32; and that result is the coherent fold of the expanded buffer within eps_c"""
    c = CASES[name]
    y, x, F, T, P, n = c["y"], c["x"], c["F"], c["T"], c["y"] * c["x"], c["n"]
    kern = c["coherent"]
    raw, scale, z = K.quantise(K.samples(name), fmt)
    rng = np.random.default_rng(P + 1)
    S = (rng.standard_normal(P) + 1j * rng.standard_normal(P)).astype(C64)
    with D.Arenas(ctx) as A:
        d_raw, d_z = A.input("raw", K.padded(raw, fmt), 0), A.input("expanded", np.concatenate([z, NAN_SAMPLE]), 8)
        d_tr, d_zr = A.input("track", K.track(c), 8), A.input("zref", S, 8)
        outs = []
        for tag, ptr, code, sc in (("raw", d_raw.ptr, K.FMT_CODE[fmt], scale), ("expanded", d_z.ptr, 0, 1.0)):
            o = [A.output("state " + tag, 4 * P, 4), A.output("out " + tag, 8 * (4 * F + 1), 8), A.output("gram " + tag, 16 * F * F, 8)]
            _run(ctx, {"cfold_" + kern}, lambda: TC._fold_d(ctx, ptr, code, sc, n, c["t0"], T, KAPPA, F, y, x, 0.0, o[0].ptr))
            _run(ctx, {"ctrack_probe_" + kern, "ctrack_probe_sum"},
                 lambda: _case_probe(ctx, c, ptr, n, d_tr.ptr, d_zr.ptr, o[1].ptr, fmt=code, scale=sc))
            _run(ctx, {"gram_" + kern, "gram_sum"}, lambda: _gram_d(ctx, ptr, code, sc, n, c["t0"], T, d_tr.ptr, F, y, x, o[2].ptr))
            outs.append(o)
        A.check()
        for a, b in zip(*outs):
            _same_bits(a, b)
        state, out, gram = outs[0][0].get(F32), outs[0][1].get(np.float64), outs[0][2].get(np.float64)
    _finite(state, out, gram)
    zz = CF.samples(z)
    err = float(np.max(np.abs(state.astype(np.float64) - CF.cfold(zz, c["t0"], T, KAPPA, F, y, x))))
    _report(f"domain {name} {fmt} cfold", err, CF.eps_c(F, np.abs(zz).max()))
    assert err <= CF.eps_c(F, np.abs(zz).max())


# ---------------------------------------------------------------- 7. zero denominators
def test_zero_denominators_give_what_the_headers_say(ctx):
    """P1 on a buffer of zeros, its one-pixel state zero too: E_z * E_s and E_f * E_s are not positive, so gamma = 0, theta = 0 and
    q = (1, 0) (tempest_hip_cstack.h, 5. and 6.), gamma_f = 0 (tempest_hip_ctrack.h, 8.); every sum, the state, mag, the scores and
    the matrix are exactly zero, and nothing is NaN"""
    c = CASES["P1"]
    y, x, F, T, n = c["y"], c["x"], c["F"], c["T"], c["n"]
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", np.concatenate([np.zeros(n, C64), NAN_SAMPLE]), 8).ptr
        d_tr = A.input("track", K.track(c), 8)
        zs, mag, info = A.output("zstate", 8, 8), A.output("mag", 4, 4), A.output("info", 64, 8)
        out, gram, st, sc = A.output("out", 8 * (4 * F + 1), 8), A.output("gram", 16 * F * F, 8), A.output("state", 4, 4), A.output("score", 72, 8)
        _fill(ctx, zs, np.zeros(1, C64))
        _case_probe(ctx, c, d_iq, n, d_tr.ptr, zs.ptr, out.ptr)
        _run(ctx, {"cstack_direct", "cstack_lock", "cstack_blend"}, lambda: _case_d(ctx, c, d_iq, n, PHI, 0.25, LOCK, zs.ptr, mag.ptr, info.ptr))
        _gram_d(ctx, d_iq, 0, 1.0, n, c["t0"], T, d_tr.ptr, F, y, x, gram.ptr)
        TC._fold_d(ctx, d_iq, 0, 1.0, n, c["t0"], T, KAPPA, F, y, x, 0.0, st.ptr)
        TC._scan_d(ctx, d_iq, 0, 1.0, n, c["t0"], T, 0.0, 0.125, 9, F, y, x, sc.ptr)
        A.check()
        assert info.get(np.float64).tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        assert np.all(zs.get(F32) == 0.0) and np.all(mag.get(F32) == 0.0) and np.all(st.get(F32) == 0.0) and np.all(sc.get(np.float64) == 0.0)
        assert np.all(out.get(np.float64) == 0.0) and np.all(gram.get(np.float64) == 0.0)
