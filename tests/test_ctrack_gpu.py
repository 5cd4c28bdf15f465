"""GPU tests of carrier tracking (include/tempest_hip_ctrack.h): the stack along a track against tests/ctrack_ref.py within cstack's
bounds, its tie to tsdr_cstack_iq_d bit for bit, the probe against the reference within the header's bounds and against the stack's
own rho, the NULL track, the state that must not be read, repeats and integer formats bit for bit, the host forms, every refusal, and
the two capabilities the feature exists for (a carrier drifting inside a buffer, a retune between buffers) on the inputs of
tests/test_ctrack_host.py.

The shapes, captures and arena offsets are tests/test_cstack_gpu.py's (CASES U, M, D, S, R, X; `zstate` / `zref` at ZS_PHASE, `mag` at
MAG_PHASE, ComplexF32 `iq` at IQ_PHASE); the track and `out` sit at 8 mod 16.  Which case reaches which kernel (asserted by profile
name): U, M, S the tiled kernels (ctrack_stack_tile, ctrack_probe_tile), D, R, X the direct ones.  References are made once per case
(functools caches); nothing modifies them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cstack_ref as CS
import ctrack_ref as R
import dptr_util as D
import test_ctrack_host as H
from test_cstack_gpu import (ALL, CASES, IQ_PHASE, KAPPA_TRUE, KERNEL, MAG_PHASE, MODE_NAME, ZS_PHASE, _capture, _case_of, _check_info, _fill,
                             _null, _pkg, _profiled, _quantised, _report, _stack_d, _zref)

pytestmark = pytest.mark.gpu

F32, C64 = np.float32, np.complex64
GIVEN, LOCK = R.GIVEN, R.LOCK


def _track(name):
    """the test track of a case: a_f = 0.37 + f kappa_true + 0.01 f^2, b_f = 0.02 f - 0.03"""
    f = np.arange(CASES[name]["F"], dtype=np.float64)
    return np.ascontiguousarray(np.stack([0.37 + f * KAPPA_TRUE + 0.01 * f * f, 0.02 * f - 0.03], axis=1))


@functools.lru_cache(maxsize=None)
def _ztrack(name):
    """the reference's Z of a case along its test track, state order, complex128[P]"""
    c = CASES[name]
    Z = R.zmean(CS.samples(_capture(name)[0]), c["t0"], c["T"], _track(name), c["F"], c["y"], c["x"])
    Z.setflags(write=False)
    return Z


def _noisy(Z, level):
    """Z turned by 0.3 turn plus `level` (of its rms) complex noise, complex64 -- as test_cstack_gpu._state_in makes its state"""
    rng = np.random.default_rng(Z.size)
    rms = math.sqrt(float(np.mean(np.abs(Z) ** 2)))
    S = (Z * np.exp(2j * np.pi * 0.3) + level * rms * (rng.normal(size=Z.size) + 1j * rng.normal(size=Z.size)) / math.sqrt(2.0)).astype(C64)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def _state_in(name):
    """the entry state of the stack tests: the case's tracked reference Z turned by 0.3 turn, plus 5 % noise"""
    return _noisy(_ztrack(name), 0.05)


@functools.lru_cache(maxsize=None)
def _probe_ref_picture(name):
    """zref of the probe tests: the case's reference Z (constant kappa, phi = 0) turned by 0.3 turn, plus 30 % noise"""
    return _noisy(_zref(name, 0.0), 0.30)


def _tstack_d(ctx, iq, fmt, scale, n, t0, T, track, F, y, x, alpha, mode, zs, mag, info):
    ctx.call("tsdr_ctrack_stack_iq_d", iq, fmt, C.c_float(scale), n, C.c_double(t0), C.c_double(T), track, F, y, x, C.c_float(alpha), mode,
             zs, mag, info)


def _probe_d(ctx, iq, fmt, scale, n, t0, T, track, F, y, x, zref, out):
    ctx.call("tsdr_ctrack_probe_iq_d", iq, fmt, C.c_float(scale), n, C.c_double(t0), C.c_double(T), track, F, y, x, zref, out)


def _case_stack(ctx, name, d_iq, n, d_track, alpha, mode, zs, mag, info, fmt=0, scale=1.0):
    c = _case_of(name)
    _tstack_d(ctx, d_iq, fmt, scale, n, c["t0"], c["T"], d_track, c["F"], c["y"], c["x"], alpha, mode, zs, mag, info)


def _case_probe(ctx, name, d_iq, n, d_track, zref, out, fmt=0, scale=1.0):
    c = _case_of(name)
    _probe_d(ctx, d_iq, fmt, scale, n, c["t0"], c["T"], d_track, c["F"], c["y"], c["x"], zref, out)


# ---------------------------------------------------------------- 1. the stack against the reference
@pytest.mark.parametrize("alpha", [0.0, 0.25])
@pytest.mark.parametrize("name", ALL)
def test_stack_matches_the_reference(ctx, name, alpha):
    """zstate, mag and info along the test track within tempest_hip_cstack.h's bounds (ACCURACY; tempest_hip_ctrack.h, 5.), both modes.
    alpha = 0 runs on an all-NaN state; alpha = 0.25 on the tracked reference Z turned by 0.3 turn plus 5 % noise."""
    c = CASES[name]
    iq, amax = _capture(name)
    P, F = c["y"] * c["x"], c["F"]
    S_in = np.full(P, np.nan + 1j * np.nan, C64) if alpha == 0 else _state_in(name)
    M = 0.0 if alpha == 0 else float(np.abs(S_in.astype(np.complex128)).max())
    Z = _ztrack(name)
    for mode in (GIVEN, LOCK):
        ref, ref_info = CS.step(Z, alpha, mode, S_in.astype(np.complex128))
        if alpha:
            assert ref_info[5] >= 0.5, ref_info
        with D.Arenas(ctx) as A:
            d_iq, d_tr = A.input("iq", iq, IQ_PHASE[name]), A.input("track", _track(name), 8)
            d_zs, d_mag, d_info = A.output("zstate", 8 * P, ZS_PHASE[name]), A.output("mag", 4 * P, MAG_PHASE[name]), A.output("info", 64, 8)
            _fill(ctx, d_zs, S_in)
            names = _profiled(ctx, lambda: _case_stack(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, alpha, mode, d_zs.ptr, d_mag.ptr, d_info.ptr))
            A.check()
            zs, mag, info = d_zs.get(C64).astype(np.complex128), d_mag.get(F32).astype(np.float64), d_info.get(np.float64)
        want = {"ctrack_stack_" + KERNEL[name], "cstack_lock"} | ({"cstack_blend"} if mode == LOCK else set())
        assert names == want, (names, want)
        assert np.isfinite(zs.view(np.float64)).all() and np.isfinite(mag).all() and np.isfinite(info).all()
        what = f"ctrack stack {name} alpha {alpha} {MODE_NAME[mode]}"
        e_rho, rho_abs = _check_info(what, info, ref_info, F, amax, P)
        if mode == GIVEN:
            b_s, b_m = CS.eps_s(F, amax, M), CS.eps_mag(F, amax, M)
        else:
            b_s, b_m = CS.eps_lock(F, amax, M, e_rho, rho_abs), CS.eps_lock_mag(F, amax, M, e_rho, rho_abs)
        err_s, err_m = float(np.max(np.abs(zs - ref))), float(np.max(np.abs(mag - np.abs(ref))))
        _report(f"{what} zstate", err_s, b_s)
        _report(f"{what} mag", err_m, b_m)
        assert err_s <= b_s and err_m <= b_m, (name, alpha, mode, err_s, b_s, err_m, b_m)
    # the track matters: the constant-kappa picture is somewhere else
    assert float(np.max(np.abs(Z - _zref(name, 0.37)))) > 100.0 * CS.eps_s(F, amax)


# ---------------------------------------------------------------- 2. tied to cstack
@pytest.mark.parametrize("phi", [0.0, 0.37])
@pytest.mark.parametrize("name", ["U", "D", "S", "R"])
def test_constant_track_has_the_bits_of_cstack(ctx, name, phi):
    """with constant_track(F, kappa, phi) -- b_f = 0 -- zstate, mag and info are tsdr_cstack_iq_d's, bit for bit, in both modes"""
    c = CASES[name]
    iq = _capture(name)[0]
    P = c["y"] * c["x"]
    track = _pkg("ctrack").constant_track(c["F"], KAPPA_TRUE, phi)
    S_in = _state_in(name)
    for mode, alpha in ((GIVEN, 0.0), (GIVEN, 0.25), (LOCK, 0.25)):
        with D.Arenas(ctx) as A:
            d_iq, d_tr = A.input("iq", iq, IQ_PHASE[name]), A.input("track", track, 8)
            outs = []
            for tag in ("ctrack", "cstack"):
                o = [A.output("zstate " + tag, 8 * P, ZS_PHASE[name]), A.output("mag " + tag, 4 * P, MAG_PHASE[name]), A.output("info " + tag, 64, 8)]
                _fill(ctx, o[0], S_in)
                outs.append(o)
            _case_stack(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, alpha, mode, outs[0][0].ptr, outs[0][1].ptr, outs[0][2].ptr)
            _stack_d(ctx, d_iq.ptr, 0, 1.0, iq.size, c["t0"], c["T"], KAPPA_TRUE, phi, c["F"], c["y"], c["x"], alpha, mode, outs[1][0].ptr,
                     outs[1][1].ptr, outs[1][2].ptr)
            A.check()
            for a, b in zip(*outs):
                assert np.array_equal(a.get(np.uint32), b.get(np.uint32)), (name, phi, mode, alpha, a.name)
            assert np.all(outs[0][1].get(F32) > 0)


# ---------------------------------------------------------------- 3. the probe against the reference
@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_probe_matches_the_reference(ctx, name, tracked):
    """rho_f, E_f and E_s within the header's bounds (9.), gamma_f consistent with the record's own sums; track NULL and the test track;
    zref: the case's reference Z turned by 0.3 turn plus 30 % noise"""
    c = CASES[name]
    iq, amax = _capture(name)
    P, F = c["y"] * c["x"], c["F"]
    S = _probe_ref_picture(name)
    track = _track(name) if tracked else None
    rho, E_f, gamma, E_s = R.probe(CS.samples(iq), c["t0"], c["T"], track, F, c["y"], c["x"], S.astype(np.complex128))
    with D.Arenas(ctx) as A:
        d_iq, d_zr = A.input("iq", iq, IQ_PHASE[name]), A.input("zref", S, ZS_PHASE[name])
        d_tr = A.input("track", track, 8).ptr if tracked else _null()
        d_out = A.output("out", 8 * (4 * F + 1), 8)
        names = _profiled(ctx, lambda: _case_probe(ctx, name, d_iq.ptr, iq.size, d_tr, d_zr.ptr, d_out.ptr))
        A.check()
        out = d_out.get(np.float64)
    assert names == {"ctrack_probe_" + KERNEL[name], "ctrack_probe_sum"}, names
    assert np.isfinite(out).all()
    g_rho, g_E, g_gamma, g_Es = _pkg("ctrack").probe_record(out, F)
    what = f"ctrack probe {name} {'track' if tracked else 'NULL'}"
    assert abs(g_Es - E_s) <= R.eps_es(E_s), (g_Es, E_s)
    worst = [0.0, 0.0]
    for f in range(F):
        b_rho, b_E = R.eps_rho(amax, P, E_f[f], E_s), R.eps_ef(amax, P, E_f[f])
        worst = [max(worst[0], abs(g_rho[f] - rho[f]) / b_rho), max(worst[1], abs(g_E[f] - E_f[f]) / b_E)]
        assert abs(g_rho[f] - rho[f]) <= b_rho and abs(g_E[f] - E_f[f]) <= b_E, (name, f, abs(g_rho[f] - rho[f]), b_rho, abs(g_E[f] - E_f[f]), b_E)
        assert abs(g_gamma[f] - abs(g_rho[f]) / math.sqrt(g_E[f] * g_Es)) <= 1e-12
        # gamma = |rho| (E_f E_s)^(-1/2): to first order its relative error is rho's plus half of each energy's (1 % for the higher orders)
        b_gamma = 1.01 * gamma[f] * (b_rho / abs(rho[f]) + 0.5 * b_E / E_f[f] + 0.5 * R.eps_es(E_s) / E_s) + 1e-12
        assert abs(g_gamma[f] - gamma[f]) <= b_gamma, (name, f, g_gamma[f], gamma[f], b_gamma)
    print(f"{what}: max |rho_f - ref| / bound {worst[0]:.3f}, max |E_f - ref| / bound {worst[1]:.3f}")
    assert np.all(gamma > 0.05), "the frames are coherent with the picture: the comparison means something"


# ---------------------------------------------------------------- 4. the probe and the stack see the same rho
@pytest.mark.parametrize("name", ["U", "D", "X"])
def test_mean_of_the_probe_is_the_stacks_rho(ctx, name):
    """sum_f rho_f / F of the probe agrees with info[0..1] of a GIVEN stack along the same track onto the same picture, within the sum
    of the two bounds: the stack's eps_rho and the mean of the frames' eps_rho_f"""
    c = CASES[name]
    iq, amax = _capture(name)
    P, F = c["y"] * c["x"], c["F"]
    S = _state_in(name)
    with D.Arenas(ctx) as A:
        d_iq, d_tr, d_zr = A.input("iq", iq, IQ_PHASE[name]), A.input("track", _track(name), 8), A.input("zref", S, ZS_PHASE[name])
        d_out, d_zs, d_info = A.output("out", 8 * (4 * F + 1), 8), A.output("zstate", 8 * P, ZS_PHASE[name]), A.output("info", 64, 8)
        _fill(ctx, d_zs, S)
        _case_probe(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, d_zr.ptr, d_out.ptr)
        _case_stack(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, 0.25, GIVEN, d_zs.ptr, _null(), d_info.ptr)
        A.check()
        rho, E_f, _, E_s = _pkg("ctrack").probe_record(d_out.get(np.float64), F)
        info = d_info.get(np.float64)
    bound = CS.eps_rho(F, amax, P, info[2], info[3]) + float(np.mean([R.eps_rho(amax, P, E_f[f], E_s) for f in range(F)]))
    err = abs(np.sum(rho) / F - complex(info[0], info[1]))
    _report(f"ctrack {name}: mean of the probe's rho_f against the stack's rho", err, bound)
    assert err <= bound and abs(complex(info[0], info[1])) > 100.0 * bound
    assert abs(E_s - info[3]) <= 2.0 * R.eps_es(E_s)


# ---------------------------------------------------------------- 5. the NULL track
@pytest.mark.parametrize("name", ["U", "R"])
def test_null_track_is_the_zero_track(ctx, name):
    c = CASES[name]
    iq = _capture(name)[0]
    F = c["F"]
    S = _probe_ref_picture(name)
    with D.Arenas(ctx) as A:
        d_iq, d_zr, d_tr = A.input("iq", iq, IQ_PHASE[name]), A.input("zref", S, ZS_PHASE[name]), A.input("track", np.zeros((F, 2)), 8)
        a, b = A.output("out NULL", 8 * (4 * F + 1), 8), A.output("out zeros", 8 * (4 * F + 1), 0)
        _case_probe(ctx, name, d_iq.ptr, iq.size, _null(), d_zr.ptr, a.ptr)
        _case_probe(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, d_zr.ptr, b.ptr)
        A.check()
        assert np.array_equal(a.get(np.uint64), b.get(np.uint64))
        assert np.all(a.get(np.float64)[2::4] > 0)


# ---------------------------------------------------------------- 6. alpha = 0 does not read the state
@pytest.mark.parametrize("mode", [GIVEN, LOCK])
@pytest.mark.parametrize("name", ["U", "R"])
def test_alpha_zero_does_not_read_the_state(ctx, name, mode):
    c = CASES[name]
    iq, amax = _capture(name)
    P = c["y"] * c["x"]
    with D.Arenas(ctx) as A:
        d_iq, d_tr = A.input("iq", iq, IQ_PHASE[name]), A.input("track", _track(name), 8)
        d_zs, d_mag, d_info = A.output("zstate", 8 * P, ZS_PHASE[name]), A.output("mag", 4 * P, 4), A.output("info", 64, 8)
        _fill(ctx, d_zs, np.full(2 * P, np.nan, F32))
        _case_stack(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, 0.0, mode, d_zs.ptr, d_mag.ptr, d_info.ptr)
        A.check()
        zs, mag, info = d_zs.get(F32), d_mag.get(F32), d_info.get(np.float64)
    assert np.isfinite(zs).all() and np.isfinite(mag).all() and np.isfinite(info).all()
    assert info[0] == 0.0 and info[1] == 0.0 and info[3] == 0.0 and info[4] == 0.0 and info[5] == 0.0 and info[2] > 0.0
    assert (info[6], info[7]) == (1.0, 0.0)
    assert float(np.max(np.abs(zs.view(C64).astype(np.complex128) - _ztrack(name)))) <= CS.eps_lock(c["F"], amax, 0.0, 0.0, 0.0)


# ---------------------------------------------------------------- 7. repeats
@pytest.mark.parametrize("name", ["U", "D", "X"])
def test_two_calls_leave_identical_bits(ctx, name):
    """the same stack (both modes) and the same probe twice, outputs at other offsets: identical bytes"""
    c = CASES[name]
    iq = _capture(name)[0]
    P, F = c["y"] * c["x"], c["F"]
    S_in = _state_in(name)
    with D.Arenas(ctx) as A:
        d_iq, d_tr, d_zr = A.input("iq", iq, IQ_PHASE[name]), A.input("track", _track(name), 8), A.input("zref", S_in, 8)
        for mode in (GIVEN, LOCK):
            outs = []
            for k in range(2):
                o = [A.output(f"zstate {k}", 8 * P, 8 * k), A.output(f"mag {k}", 4 * P, 4 + 8 * k), A.output(f"info {k}", 64, 8 * k)]
                _fill(ctx, o[0], S_in)
                _case_stack(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, 0.25, mode, o[0].ptr, o[1].ptr, o[2].ptr)
                outs.append(o)
            A.check()
            for a, b in zip(*outs):
                assert np.array_equal(a.get(np.uint32), b.get(np.uint32)), (mode, a.name)
        probes = [A.output(f"out {k}", 8 * (4 * F + 1), 8 * k) for k in range(2)]
        for o in probes:
            _case_probe(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, d_zr.ptr, o.ptr)
        A.check()
        assert np.array_equal(probes[0].get(np.uint64), probes[1].get(np.uint64))
        assert np.isfinite(probes[0].get(np.float64)).all()


# ---------------------------------------------------------------- 8. formats
@pytest.mark.parametrize("fmt", ["sc16", "sc8", "uc8"])
def test_integer_formats_give_the_bits_of_the_expanded_buffer(ctx, fmt):
    """the stack (LOCK, alpha 0.25: zstate, mag, info) and the probe (out), cases U (tiled) and D (direct): sc16 / sc8 / uc8 in, the bits
    of the same call on the host-expanded ComplexF32"""
    code = {"sc16": 1, "sc8": 2, "uc8": 3}[fmt]
    for name in ("U", "D"):
        c = CASES[name]
        raw, scale, z = _quantised(name, fmt)
        n, P, F = z.size, c["y"] * c["x"], c["F"]
        S_in = _state_in(name)
        with D.Arenas(ctx) as A:
            d_raw, d_z = A.input("raw", raw, 0), A.input("expanded", z, 8)
            d_tr, d_zr = A.input("track", _track(name), 8), A.input("zref", S_in, ZS_PHASE[name])
            outs = []
            for tag, ptr, cd, sc in (("raw", d_raw.ptr, code, scale), ("expanded", d_z.ptr, 0, 1.0)):
                o = [A.output("zstate " + tag, 8 * P, 8), A.output("mag " + tag, 4 * P, 4), A.output("info " + tag, 64, 8),
                     A.output("out " + tag, 8 * (4 * F + 1), 8)]
                _fill(ctx, o[0], S_in)
                _case_stack(ctx, name, ptr, n, d_tr.ptr, 0.25, LOCK, o[0].ptr, o[1].ptr, o[2].ptr, fmt=cd, scale=sc)
                _case_probe(ctx, name, ptr, n, d_tr.ptr, d_zr.ptr, o[3].ptr, fmt=cd, scale=sc)
                outs.append(o)
            A.check()
            for a, b in zip(*outs):
                assert np.array_equal(a.get(np.uint32), b.get(np.uint32)), (name, fmt, a.name)
            assert np.isfinite(outs[0][3].get(np.float64)).all() and np.isfinite(outs[0][0].get(F32)).all()


# ---------------------------------------------------------------- 9. the host forms
def test_host_forms_agree_with_the_device_forms(ctx):
    """Context.ctrack_stack / ctrack_probe (host arrays) and the device forms give the same bits; the caller's arrays are inputs"""
    name = "U"
    c = CASES[name]
    iq = _capture(name)[0]
    y, x, P, F = c["y"], c["x"], c["y"] * c["x"], c["F"]
    S_in = _state_in(name)
    st = np.asfortranarray(S_in.reshape((y, x), order="F"))
    keep, track = st.copy(), _track(name)
    for mode, alpha in ((GIVEN, 0.0), (GIVEN, 0.25), (LOCK, 0.25)):
        zs, mag, info = ctx.ctrack_stack(iq, c["t0"], c["T"], track, F, y, x, alpha=alpha, mode=MODE_NAME[mode].lower(),
                                         zstate=st if alpha else None)
        assert zs.shape == (y, x) and zs.dtype == C64 and mag.shape == (y, x) and mag.dtype == F32 and info.shape == (8,)
        assert np.array_equal(st, keep) and np.array_equal(track, _track(name))
        with D.Arenas(ctx) as A:
            d_iq, d_tr = A.input("iq", iq, 8), A.input("track", track, 8)
            d_zs, d_mag, d_info = A.output("zstate", 8 * P, 8), A.output("mag", 4 * P, 12), A.output("info", 64, 8)
            _fill(ctx, d_zs, S_in)
            ctx.ctrack_stack_d(d_iq.addr, "cf32", 1.0, iq.size, c["t0"], c["T"], d_tr.addr, F, y, x, alpha, mode, d_zs.addr, d_mag.addr, d_info.addr)
            A.check()
            assert np.array_equal(zs.reshape(-1, order="F").view(np.uint32), d_zs.get(np.uint32))
            assert np.array_equal(mag.reshape(-1, order="F").view(np.uint32), d_mag.get(np.uint32))
            assert np.array_equal(info.view(np.uint64), d_info.get(np.uint64))
    for tr in (None, track):
        rho, E_f, gamma, E_s = ctx.ctrack_probe(iq, c["t0"], c["T"], tr, F, y, x, st)
        with D.Arenas(ctx) as A:
            d_iq, d_zr = A.input("iq", iq, 8), A.input("zref", S_in, 8)
            d_tr = A.input("track", tr, 8).addr if tr is not None else None
            d_out = A.output("out", 8 * (4 * F + 1), 8)
            ctx.ctrack_probe_d(d_iq.addr, "cf32", 1.0, iq.size, c["t0"], c["T"], d_tr, F, y, x, d_zr.addr, d_out.addr)
            A.check()
            g = _pkg("ctrack").probe_record(d_out.get(np.float64), F)
        assert np.array_equal(rho, g[0]) and np.array_equal(E_f, g[1]) and np.array_equal(gamma, g[2]) and E_s == g[3]
    # the raw symbols with mag = info = NULL, and a NULL track of the probe
    raw = S_in.copy()
    rc = ctx.lib.tsdr_ctrack_stack_iq(ctx.h, C.c_void_p(iq.ctypes.data), 0, 1.0, iq.size, c["t0"], c["T"], C.c_void_p(track.ctypes.data), F, y, x,
                                      0.25, LOCK, C.c_void_p(raw.ctypes.data), None, None)
    assert rc == 0 and np.array_equal(raw.view(np.uint32), zs.reshape(-1, order="F").view(np.uint32))


# ---------------------------------------------------------------- 10. refusals and untouched memory
def test_refusals_leave_everything_untouched(ctx):
    """every TSDR_EINVAL of the header, and F == 0 (TSDR_OK): nothing is launched, and the sentinel-filled outputs are as uploaded"""
    c = CASES["U"]
    iq = _capture("U")[0]
    raw = np.zeros(2 * 4096, np.int16)
    n, P, y, x, F, t0, T = iq.size, c["y"] * c["x"], c["y"], c["x"], c["F"], c["t0"], c["T"]
    nan, inf = float("nan"), float("inf")
    track = _track("U")
    with D.Arenas(ctx) as A:
        d_iq, d_raw, d_tr = A.input("iq", iq, 8), A.input("raw", raw, 0), A.input("track", track, 8)
        d_zs, d_mag, d_info = A.output("zstate", 8 * P, 8), A.output("mag", 4 * P, 4), A.output("info", 64, 8)
        d_zr, d_out = A.input("zref", _state_in("U"), 8), A.output("out", 8 * (4 * F + 1), 8)
        good = dict(iq=d_iq.addr, fmt=0, n=n, t0=t0, T=T, tr=d_tr.addr, F=F, y=y, x=x, alpha=0.0, mode=LOCK, zs=d_zs.addr, mag=d_mag.addr,
                    info=d_info.addr, zr=d_zr.addr, out=d_out.addr)

        def stack(**kw):
            k = dict(good, **kw)
            _tstack_d(ctx, C.c_void_p(k["iq"]), k["fmt"], 1.0, k["n"], k["t0"], k["T"], C.c_void_p(k["tr"]), k["F"], k["y"], k["x"], k["alpha"],
                      k["mode"], C.c_void_p(k["zs"]), C.c_void_p(k["mag"]), C.c_void_p(k["info"]))

        def probe(**kw):
            k = dict(good, **kw)
            _probe_d(ctx, C.c_void_p(k["iq"]), k["fmt"], 1.0, k["n"], k["t0"], k["T"], C.c_void_p(k["tr"]), k["F"], k["y"], k["x"],
                     C.c_void_p(k["zr"]), C.c_void_p(k["out"]))

        geometry = [dict(iq=0), dict(fmt=4), dict(fmt=-1), dict(y=0), dict(x=-3), dict(y=65536, x=32768), dict(n=1), dict(n=1 << 31), dict(F=-1),
                    dict(T=nan), dict(T=inf), dict(t0=nan), dict(t0=inf), dict(T=1.5), dict(t0=-0.5), dict(F=F + 1), dict(t0=t0 + 20.0),
                    dict(n=n - 20), dict(iq=d_iq.addr + 4), dict(iq=d_raw.addr + 8, fmt=1, n=2048, F=1), dict(iq=d_raw.addr + 4, fmt=2, n=2048, F=1),
                    dict(tr=d_tr.addr + 4)]
        bad_stack = geometry + [dict(zs=0), dict(tr=0), dict(mode=2), dict(mode=-1), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan),
                                dict(zs=d_zs.addr + 4), dict(mag=d_mag.addr + 2), dict(info=d_info.addr + 4)]
        bad_probe = geometry + [dict(zr=0), dict(out=0), dict(zr=d_zr.addr + 4), dict(out=d_out.addr + 4)]

        def refused():
            for fn, bad in ((stack, bad_stack), (probe, bad_probe)):
                for kw in bad:
                    with pytest.raises(AssertionError, match="invalid|ctrack"):
                        fn(**kw)
                fn(F=0)
            assert ctx.lib.tsdr_ctrack_stack_iq_d(None, d_iq.ptr, 0, 1.0, n, t0, T, d_tr.ptr, F, y, x, 0.0, LOCK, d_zs.ptr, d_mag.ptr,
                                                  d_info.ptr) == -1
            assert ctx.lib.tsdr_ctrack_probe_iq_d(None, d_iq.ptr, 0, 1.0, n, t0, T, d_tr.ptr, F, y, x, d_zr.ptr, d_out.ptr) == -1

        assert _profiled(ctx, refused) == set(), "nothing is enqueued"
        A.check()
        for a in (d_zs, d_mag, d_info, d_out):
            assert np.array_equal(a.get(np.uint32), D.sentinel_words(a.size // 4)[a.lead // 4: (a.lead + a.payload) // 4]), a.name
        # and the context still serves valid calls afterwards; the probe accepts a NULL track
        stack()
        probe(tr=0)
        A.check()
        assert np.all(np.isfinite(d_zs.get(F32))) and np.all(np.isfinite(d_out.get(np.float64)))
    # host forms: the same refusals and a non-finite track entry, host arrays untouched; F == 0 touches nothing
    zs, mag, info, out = np.full(2 * P, 7.0, F32), np.full(P, 7.0, F32), np.full(8, 7.0), np.full(4 * F + 1, 7.0)
    z, zr = iq.copy(), _state_in("U").copy()
    bad_nan, bad_inf = track.copy(), track.copy()
    bad_nan[F - 1, 0], bad_inf[2, 1] = nan, inf
    host = dict(good, tr=track.ctypes.data, zs=zs.ctypes.data, zr=zr.ctypes.data, out=out.ctypes.data)
    common = [dict(T=nan), dict(F=F + 1), dict(fmt=5), dict(y=0), dict(tr=bad_nan.ctypes.data), dict(tr=bad_inf.ctypes.data), dict(F=0)]
    for kw in common + [dict(mode=3), dict(alpha=2.0), dict(zs=0), dict(tr=0)]:
        k = dict(host, **kw)
        rc = ctx.lib.tsdr_ctrack_stack_iq(ctx.h, C.c_void_p(z.ctypes.data), k["fmt"], 1.0, n, k["t0"], k["T"], C.c_void_p(k["tr"]), k["F"], k["y"],
                                          k["x"], k["alpha"], k["mode"], C.c_void_p(k["zs"]), C.c_void_p(mag.ctypes.data),
                                          C.c_void_p(info.ctypes.data))
        assert rc == (0 if kw == dict(F=0) else -1), kw
    for kw in common + [dict(zr=0), dict(out=0)]:
        k = dict(host, **kw)
        rc = ctx.lib.tsdr_ctrack_probe_iq(ctx.h, C.c_void_p(z.ctypes.data), k["fmt"], 1.0, n, k["t0"], k["T"], C.c_void_p(k["tr"]), k["F"], k["y"],
                                          k["x"], C.c_void_p(k["zr"]), C.c_void_p(k["out"]))
        assert rc == (0 if kw == dict(F=0) else -1), kw
    assert np.all(zs == 7.0) and np.all(mag == 7.0) and np.all(info == 7.0) and np.all(out == 7.0) and np.array_equal(z, iq)


# ---------------------------------------------------------------- 11. the capabilities
def test_capability_a_drifting_carrier_inside_one_buffer(ctx):
    """The inputs of tests/test_ctrack_host.py: 66 x 160, T 9150.37, t0 3.25, -10 dB, 24 frames, a ramp of 0.012 turns/frame per frame,
    start kappa 0.7708.  Correlation with the noiseless card of (a) the constant-kappa picture, (b) refine_track's picture after two
    iterations.  tests/ctrack_ref.py gives (a) 0.314, (b) 0.555 (0.553 after one pass); the capture without drift gives 0.555.
    Asserted: each within 0.01 of the reference, (a) <= 0.36, (b) >= 0.50."""
    y, x, T, t0, F = H.CAP["y"], H.CAP["x"], H.CAP["T"], H.CAP["t0"], H.DRIFT["frames"]
    P = y * x
    iq = H.drift_captures()[1]
    _, ref_const, _, ref_two = H.drift_reference()
    card = H.cap_card()
    ctrack = _pkg("ctrack")
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, 8)
        d_zs, d_mag, d_m0 = A.output("zstate", 8 * P, 8), A.output("mag", 4 * P, 4), A.output("mag constant", 4 * P, 12)
        d_z0, d_tr = A.output("zstate constant", 8 * P, 0), A.input("track", ctrack.constant_track(F, H.DRIFT["kappa"]), 8)
        _tstack_d(ctx, d_iq.ptr, 0, 1.0, iq.size, t0, T, d_tr.ptr, F, y, x, 0.0, GIVEN, d_z0.ptr, d_m0.ptr, _null())
        track, polys, gammas = ctx.refine_track(d_iq.addr, "cf32", 1.0, iq.size, t0, T, F, y, x, H.DRIFT["kappa"], iterations=2, degree=2,
                                                zstate=d_zs.addr, mag=d_mag.addr)
        A.check()
        const, two = H.corr(d_m0.get(F32), card), H.corr(d_mag.get(F32), card)
    print(f"drift: constant kappa {const:.3f} (reference {ref_const:.3f}), tracked after two iterations {two:.3f} (reference {ref_two:.3f}); "
          f"mean gamma per iteration {[round(float(g.mean()), 3) for g in gammas]}; fitted chi {2.0 * polys[0].coeffs[0]:.4f}")
    assert abs(const - ref_const) <= 0.01 and abs(two - ref_two) <= 0.01, (const, ref_const, two, ref_two)
    assert const <= 0.36 and two >= 0.50, (const, two)
    assert track.shape == (F, 2) and len(polys) == 2 and len(gammas) == 2


def test_capability_a_retune_between_buffers(ctx):
    """The inputs of tests/test_ctrack_host.py: two buffers of ceil(13 T) + 7 samples at -10 dB, the second retuned by 200 Hz (3.333
    turns per frame).  LOCK with alpha 0.5 onto the first buffer's picture: tsdr_cstack_iq_d at kappa_B = frac(kappa + 3.333) finds
    gamma 0.068 in the reference, tsdr_ctrack_stack_iq_d along constant_track(F, kappa + 3.333, 0, 3.333) finds 0.646 and a picture
    that scores 0.545.  Asserted: each within 0.01 of the reference, cstack's gamma <= 0.15, the tracked gamma >= 0.55."""
    y, x, T = H.CAP["y"], H.CAP["x"], H.CAP["T"]
    P = y * x
    (a, t0a, Fa), (b, t0b, Fb) = H.retune_buffers()
    _, ref_gp, ref_cp, ref_gt, ref_ct = H.retune_reference()
    card = H.cap_card()
    dk, alpha = H.RETUNE["dkappa"], H.RETUNE["alpha"]
    track = _pkg("ctrack").constant_track(Fb, KAPPA_TRUE + dk, 0.0, dk)
    with D.Arenas(ctx) as A:
        d_a, d_b, d_tr = A.input("iq a", a, 8), A.input("iq b", b, 0), A.input("track", track, 8)
        zs = [A.output("zstate cstack", 8 * P, 8), A.output("zstate ctrack", 8 * P, 0)]
        mag = [A.output("mag cstack", 4 * P, 4), A.output("mag ctrack", 4 * P, 12)]
        info = [A.output("info cstack", 64, 8), A.output("info ctrack", 64, 0)]
        for k in range(2):
            _stack_d(ctx, d_a.ptr, 0, 1.0, a.size, t0a, T, KAPPA_TRUE, 0.0, Fa, y, x, 0.0, GIVEN, zs[k].ptr, _null(), _null())
        _stack_d(ctx, d_b.ptr, 0, 1.0, b.size, t0b, T, CS.frac(KAPPA_TRUE + dk), 0.0, Fb, y, x, alpha, LOCK, zs[0].ptr, mag[0].ptr, info[0].ptr)
        _tstack_d(ctx, d_b.ptr, 0, 1.0, b.size, t0b, T, d_tr.ptr, Fb, y, x, alpha, LOCK, zs[1].ptr, mag[1].ptr, info[1].ptr)
        A.check()
        gp, gt = float(info[0].get(np.float64)[5]), float(info[1].get(np.float64)[5])
        cp, ct = H.corr(mag[0].get(F32), card), H.corr(mag[1].get(F32), card)
    print(f"retune: cstack LOCK gamma {gp:.3f} (reference {ref_gp:.3f}), picture {cp:.3f} ({ref_cp:.3f}); tracked gamma {gt:.3f} ({ref_gt:.3f}), "
          f"picture {ct:.3f} ({ref_ct:.3f})")
    assert abs(gp - ref_gp) <= 0.01 and abs(gt - ref_gt) <= 0.01 and abs(cp - ref_cp) <= 0.01 and abs(ct - ref_ct) <= 0.01
    assert gp <= 0.15 and gt >= 0.55, (gp, gt)
