"""GPU tests of coherent stacking across buffers (include/tempest_hip_cstack.h): both modes against tests/cstack_ref.py within the
contract's error bounds, the tie to the coherent fold bit for bit, what the lock is for, the state that must not be read, the optional
outputs, format invariance and repeatability bit for bit, the capability itself (six buffers at -16 dB, with and without a carrier
phase step), the host form, and every refusal.  Every device pointer sits inside a guarded arena (tests/dptr_util.py): `zstate` at 8
mod 16 (the one-pixel blend) and at 0 mod 16 (the two-pixel blend, with D's odd P for its tail), `mag` at 4, 8 and 12 mod 16,
ComplexF32 `iq` at 0 and 8 mod 16.

The shapes are the coherent fold's suite's (tests/test_cfold_gpu.py): captures synth_leak(60 T, x, y, 60.0, n) at 20 dB, the carrier
advancing by kappa_true = frac(1000 / 60) turns per frame.  Which case reaches which kernel (asserted by profile name):
    U  70 x 150, T 1207.73, F 7, t0 3.25      cstack_tile     partial second line tile, partial pixel tile
    M  66 x 160, T 9150.37, F 5               cstack_tile     W 114
    D  77 x 131, T 11600.61, F 4, t0 11599.9  cstack_direct   odd sizes, odd P
    S  20 x 140, T 2550.3, F 3                cstack_tile     W 120, the widest span the tiled kernel stages
    R  20 x 140, T 2565.3, F 3                cstack_direct   W 121, the narrowest span of the direct kernel
    X   8 x 16,  T 5000.5, F 3                cstack_direct   39 samples per pixel
cstack_lock runs whenever info is asked for or the mode is LOCK; cstack_blend in LOCK mode only.

Captures and references are made once per case (functools caches); nothing modifies them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cstack_ref as R
import dptr_util as D

pytestmark = pytest.mark.gpu

F32, C64 = np.float32, np.complex64
CASES = {
    "U": dict(y=70, x=150, T=1207.73, F=7, t0=3.25),
    "M": dict(y=66, x=160, T=9150.37, F=5, t0=0.0),
    "D": dict(y=77, x=131, T=11600.61, F=4, t0=11599.9),
    "S": dict(y=20, x=140, T=2550.3, F=3, t0=1.5),
    "R": dict(y=20, x=140, T=2565.3, F=3, t0=1.5),
    "X": dict(y=8, x=16, T=5000.5, F=3, t0=0.5),
}
ALL = list(CASES)
KERNEL = {"U": "tile", "M": "tile", "D": "direct", "S": "tile", "R": "direct", "X": "direct"}
ZS_PHASE = {"U": 8, "M": 0, "D": 0, "S": 8, "R": 8, "X": 0}
MAG_PHASE = {"U": 4, "M": 8, "D": 12, "S": 8, "R": 12, "X": 4}
IQ_PHASE = {"U": 0, "M": 8, "D": 0, "S": 0, "R": 8, "X": 8}
KAPPA_TRUE = (1000.0 / 60.0) % 1.0
GIVEN, LOCK = R.GIVEN, R.LOCK
MODE_NAME = {GIVEN: "GIVEN", LOCK: "LOCK"}


def _n(c):
    return int(math.ceil(c["t0"] + c["F"] * (c["T"] + 2.0))) + 5


def _pkg(name):
    import importlib
    from tempest_loader import load_package
    load_package()
    return importlib.import_module("tempestsdr_jl_amd." + name)


@functools.lru_cache(maxsize=None)
def _capture(name):
    """(iq complex64[n], amax) of a case: Fs = 60 T, so one frame of the synthetic leak lasts exactly T samples"""
    c = CASES[name]
    iq = _pkg("synth").synth_leak(60.0 * c["T"], c["x"], c["y"], 60.0, _n(c), snr_db=20.0)
    iq.setflags(write=False)
    return iq, float(np.abs(R.samples(iq)).max())


@functools.lru_cache(maxsize=None)
def _zref(name, phi):
    """the reference's Z of a case in state order, complex128[P]"""
    c = CASES[name]
    Z = R.zmean(R.samples(_capture(name)[0]), c["t0"], c["T"], KAPPA_TRUE, phi, c["F"], c["y"], c["x"])
    Z.setflags(write=False)
    return Z


@functools.lru_cache(maxsize=None)
def _state_in(name):
    """the entry state of a case, complex64[P]: its own reference Z (phi = 0) turned by 0.3 turn, plus 5 % complex noise"""
    Z = _zref(name, 0.0)
    rng = np.random.default_rng(Z.size)
    rms = math.sqrt(float(np.mean(np.abs(Z) ** 2)))
    S = Z * np.exp(2j * np.pi * 0.3) + 0.05 * rms * (rng.normal(size=Z.size) + 1j * rng.normal(size=Z.size)) / math.sqrt(2.0)
    S = S.astype(C64)
    S.setflags(write=False)
    return S


def _fill(ctx, arena, data):
    """put `data` into an OUTPUT arena's payload (a state the call may overwrite)"""
    d = np.ascontiguousarray(data)
    assert d.nbytes == arena.payload
    ctx.call("tsdr_upload", arena.ptr, C.c_void_p(d.ctypes.data), d.nbytes)


def _null():
    return C.c_void_p(0)


def _stack_d(ctx, iq, fmt, scale, n, t0, T, kappa, phi, F, y, x, alpha, mode, zs, mag, info):
    ctx.call("tsdr_cstack_iq_d", iq, fmt, C.c_float(scale), n, C.c_double(t0), C.c_double(T), C.c_double(kappa), C.c_double(phi), F, y, x,
             C.c_float(alpha), mode, zs, mag, info)


def _case_of(case):
    """a case by its name in CASES, or the case itself: a dict with y, x, T, F, t0 (tests/fold_domain_cases.py's rows)"""
    return CASES[case] if isinstance(case, str) else case


def _case_d(ctx, name, d_iq, n, phi, alpha, mode, zs, mag, info, fmt=0, scale=1.0, kappa=KAPPA_TRUE):
    c = _case_of(name)
    _stack_d(ctx, d_iq, fmt, scale, n, c["t0"], c["T"], kappa, phi, c["F"], c["y"], c["x"], alpha, mode, zs, mag, info)


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


def _check_info(what, info, ref, F, amax, P):
    """the info record against the reference's within the header's bounds, and theta, gamma, q against the record's own sums"""
    rho, rho_ref = complex(info[0], info[1]), complex(ref[0], ref[1])
    E_z, E_s = float(ref[2]), float(ref[3])
    if rho_ref == 0:
        assert tuple(info[[0, 1, 3, 4, 5]]) == (0.0, 0.0, 0.0, 0.0, 0.0), info
        assert (info[6], info[7]) == (1.0, 0.0)
        e_rho = 0.0
    else:
        e_rho = R.eps_rho(F, amax, P, E_z, E_s)
        _report(f"{what} rho", abs(rho - rho_ref), e_rho)
        assert abs(rho - rho_ref) <= e_rho
        assert abs(info[3] - E_s) <= R.eps_es(E_s)
        assert e_rho <= abs(rho_ref), "the angle bound's precondition"
        _report(f"{what} theta", R.turn_dist(info[4], ref[4]), R.eps_theta(e_rho, abs(rho_ref)))
        assert R.turn_dist(info[4], ref[4]) <= R.eps_theta(e_rho, abs(rho_ref))
        assert R.turn_dist(info[4], math.atan2(info[1], info[0]) / (2.0 * math.pi)) <= 1e-12
        assert abs(info[5] - abs(rho) / math.sqrt(info[2] * info[3])) <= 1e-12
    _report(f"{what} E_z", abs(info[2] - E_z), R.eps_ez(F, amax, P, E_z))
    assert abs(info[2] - E_z) <= R.eps_ez(F, amax, P, E_z)
    return e_rho, abs(rho_ref)


# ---------------------------------------------------------------- 1. both modes against the reference
@pytest.mark.parametrize("phi", [0.0, 0.37])
@pytest.mark.parametrize("alpha", [0.0, 0.25])
@pytest.mark.parametrize("name", ALL)
def test_both_modes_match_the_reference(ctx, name, alpha, phi):
    """zstate, mag and info within the header's bounds (ACCURACY): GIVEN eps_s = sqrt(2) (F + 16) u M and sqrt(2) (F + 18) u M for mag;
    LOCK sqrt(2) (F + 19) u M + (pi / 2) amax eps_rho / |rho_ref| (F + 21 for mag); rho within eps_rho, E_z, E_s and theta within theirs.
    alpha = 0 runs on an all-NaN state, which must not be read; alpha = 0.25 on the case's own reference Z turned by 0.3 turn plus
    5 % noise, whose coherence with Z is asserted on the reference (gamma_ref >= 0.5).  The kernels are asserted by profile name."""
    c = CASES[name]
    iq, amax = _capture(name)
    P, F = c["y"] * c["x"], c["F"]
    S_in = np.full(P, np.nan + 1j * np.nan, C64) if alpha == 0 else _state_in(name)
    M = 0.0 if alpha == 0 else float(np.abs(S_in.astype(np.complex128)).max())
    Z = _zref(name, phi)
    for mode in (GIVEN, LOCK):
        ref, ref_info = R.step(Z, alpha, mode, S_in.astype(np.complex128))
        if alpha:
            assert ref_info[5] >= 0.5, ref_info
        with D.Arenas(ctx) as A:
            d_iq = A.input("iq", iq, IQ_PHASE[name])
            d_zs, d_mag, d_info = A.output("zstate", 8 * P, ZS_PHASE[name]), A.output("mag", 4 * P, MAG_PHASE[name]), A.output("info", 64, 8)
            _fill(ctx, d_zs, S_in)
            names = _profiled(ctx, lambda: _case_d(ctx, name, d_iq.ptr, iq.size, phi, alpha, mode, d_zs.ptr, d_mag.ptr, d_info.ptr))
            A.check()
            zs, mag, info = d_zs.get(C64).astype(np.complex128), d_mag.get(F32).astype(np.float64), d_info.get(np.float64)
        want = {"cstack_" + KERNEL[name], "cstack_lock"} | ({"cstack_blend"} if mode == LOCK else set())
        assert names == want, (names, want)
        assert np.isfinite(zs.view(np.float64)).all() and np.isfinite(mag).all() and np.isfinite(info).all()
        what = f"cstack {name} alpha {alpha} phi {phi} {MODE_NAME[mode]}"
        e_rho, rho_abs = _check_info(what, info, ref_info, F, amax, P)
        if mode == GIVEN:
            b_s, b_m = R.eps_s(F, amax, M), R.eps_mag(F, amax, M)
            assert (info[6], info[7]) == (1.0, 0.0)
        else:
            b_s, b_m = R.eps_lock(F, amax, M, e_rho, rho_abs), R.eps_lock_mag(F, amax, M, e_rho, rho_abs)
            if rho_abs:
                q = complex(info[0], info[1]) / math.hypot(info[0], info[1])
                assert abs(complex(info[6], info[7]) - q) <= 2.0 ** -23, "q is the direction of the record's own rho, rounded to f32"
        err_s, err_m = float(np.max(np.abs(zs - ref))), float(np.max(np.abs(mag - np.abs(ref))))
        _report(f"{what} zstate", err_s, b_s)
        _report(f"{what} mag", err_m, b_m)
        assert err_s <= b_s and err_m <= b_m, (name, alpha, phi, mode, err_s, b_s, err_m, b_m)


# ---------------------------------------------------------------- 2. tied to the coherent fold
@pytest.mark.parametrize("name", ["U", "D", "S", "R"])
def test_given_phi_zero_alpha_zero_has_the_bits_of_the_coherent_fold(ctx, name):
    """mag of a GIVEN call with phi = 0 and alpha = 0 is tsdr_cfold_iq_d's state at alpha = 0, bit for bit; and zstate's magnitude is it"""
    c = CASES[name]
    iq = _capture(name)[0]
    P = c["y"] * c["x"]
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, IQ_PHASE[name])
        d_zs, d_mag, d_st = A.output("zstate", 8 * P, 8), A.output("mag", 4 * P, MAG_PHASE[name]), A.output("cfold state", 4 * P, 4)
        _case_d(ctx, name, d_iq.ptr, iq.size, 0.0, 0.0, GIVEN, d_zs.ptr, d_mag.ptr, _null())
        ctx.call("tsdr_cfold_iq_d", d_iq.ptr, 0, C.c_float(1.0), iq.size, C.c_double(c["t0"]), C.c_double(c["T"]), C.c_double(KAPPA_TRUE),
                 c["F"], c["y"], c["x"], C.c_float(0.0), d_st.ptr)
        A.check()
        a, b = d_mag.get(np.uint32), d_st.get(np.uint32)
        assert np.array_equal(a, b), (name, int(np.count_nonzero(a != b)))
        assert np.all(d_mag.get(F32) > 0)


# ---------------------------------------------------------------- 3. what LOCK is for
@pytest.mark.parametrize("name", ["U", "D"])
def test_lock_is_blind_to_the_start_phase_and_given_follows_it(ctx, name):
    """LOCK at phi and at phi + 0.25 leave the same zstate within the two calls' LOCK bounds, and their theta differ by a quarter turn
    (Z(phi + 1/4) = -i Z(phi): rho turns by -1/4 turn); GIVEN at alpha = 0 leaves the second Z equal to the first turned by -1/4 turn
    within the two calls' eps_s"""
    c = CASES[name]
    iq, amax = _capture(name)
    P, F, phi, alpha = c["y"] * c["x"], c["F"], 0.11, 0.25
    S_in = _state_in(name)
    M = float(np.abs(S_in.astype(np.complex128)).max())
    out = {}
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, IQ_PHASE[name])
        for key, (ph, al, mode) in dict(l0=(phi, alpha, LOCK), l1=(phi + 0.25, alpha, LOCK), g0=(phi, 0.0, GIVEN),
                                        g1=(phi + 0.25, 0.0, GIVEN)).items():
            d_zs, d_info = A.output("zstate " + key, 8 * P, 8), A.output("info " + key, 64, 0)
            _fill(ctx, d_zs, S_in)
            _case_d(ctx, name, d_iq.ptr, iq.size, ph, al, mode, d_zs.ptr, _null(), d_info.ptr)
            out[key] = (d_zs, d_info)
        A.check()
        zs = {k: v[0].get(C64).astype(np.complex128) for k, v in out.items()}
        info = {k: v[1].get(np.float64) for k, v in out.items()}
    _, ref_info = R.step(_zref(name, phi), alpha, LOCK, S_in.astype(np.complex128))
    e_rho = R.eps_rho(F, amax, P, ref_info[2], ref_info[3])
    rho_abs = math.hypot(ref_info[0], ref_info[1])
    bound = 2.0 * R.eps_lock(F, amax, M, e_rho, rho_abs)
    err = float(np.max(np.abs(zs["l0"] - zs["l1"])))
    _report(f"lock {name}: zstate at phi against phi + 1/4", err, bound)
    assert err <= bound
    d_theta = R.turn_dist(info["l1"][4], info["l0"][4] - 0.25)
    _report(f"lock {name}: theta step", d_theta, 2.0 * R.eps_theta(e_rho, rho_abs))
    assert d_theta <= 2.0 * R.eps_theta(e_rho, rho_abs)
    err = float(np.max(np.abs(zs["g1"] - (-1j) * zs["g0"])))
    _report(f"given {name}: Z at phi + 1/4 against -i Z at phi", err, 2.0 * R.eps_s(F, amax))
    assert err <= 2.0 * R.eps_s(F, amax)
    assert float(np.max(np.abs(zs["g1"] - zs["g0"]))) > 100.0 * R.eps_s(F, amax), "the quarter turn is there"


# ---------------------------------------------------------------- 4. alpha = 0 does not read the state
@pytest.mark.parametrize("mode", [GIVEN, LOCK])
@pytest.mark.parametrize("name", ["U", "R"])
def test_alpha_zero_does_not_read_the_state(ctx, name, mode):
    c = CASES[name]
    iq, amax = _capture(name)
    P = c["y"] * c["x"]
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, IQ_PHASE[name])
        d_zs, d_mag, d_info = A.output("zstate", 8 * P, ZS_PHASE[name]), A.output("mag", 4 * P, 4), A.output("info", 64, 8)
        _fill(ctx, d_zs, np.full(2 * P, np.nan, F32))
        _case_d(ctx, name, d_iq.ptr, iq.size, 0.37, 0.0, mode, d_zs.ptr, d_mag.ptr, d_info.ptr)
        A.check()
        zs, mag, info = d_zs.get(F32), d_mag.get(F32), d_info.get(np.float64)
    assert np.isfinite(zs).all() and np.isfinite(mag).all() and np.isfinite(info).all()
    assert info[0] == 0.0 and info[1] == 0.0 and info[3] == 0.0 and info[4] == 0.0 and info[5] == 0.0 and info[2] > 0.0
    assert (info[6], info[7]) == (1.0, 0.0)
    ref = _zref(name, 0.37)
    assert float(np.max(np.abs(zs.view(C64).astype(np.complex128) - ref))) <= R.eps_lock(c["F"], amax, 0.0, 0.0, 0.0)


# ---------------------------------------------------------------- 5. optional outputs
@pytest.mark.parametrize("name", ["U", "D"])
def test_optional_outputs(ctx, name):
    """mag = NULL and info = NULL are accepted and change no bit of what remains; info = NULL in GIVEN mode launches no cstack_lock"""
    c = CASES[name]
    iq = _capture(name)[0]
    P = c["y"] * c["x"]
    S_in = _state_in(name)
    for mode in (GIVEN, LOCK):
        with D.Arenas(ctx) as A:
            d_iq = A.input("iq", iq, IQ_PHASE[name])
            full = [A.output("zstate", 8 * P, 8), A.output("mag", 4 * P, 12), A.output("info", 64, 8)]
            bare, no_mag, no_info = A.output("zstate alone", 8 * P, 8), A.output("zstate, info", 8 * P, 0), A.output("zstate, mag", 8 * P, 8)
            i2, m3 = A.output("info alone", 64, 0), A.output("mag alone", 4 * P, 4)
            for a in (full[0], bare, no_mag, no_info):
                _fill(ctx, a, S_in)
            _case_d(ctx, name, d_iq.ptr, iq.size, 0.2, 0.25, mode, full[0].ptr, full[1].ptr, full[2].ptr)
            names = _profiled(ctx, lambda: _case_d(ctx, name, d_iq.ptr, iq.size, 0.2, 0.25, mode, bare.ptr, _null(), _null()))
            _case_d(ctx, name, d_iq.ptr, iq.size, 0.2, 0.25, mode, no_mag.ptr, _null(), i2.ptr)
            _case_d(ctx, name, d_iq.ptr, iq.size, 0.2, 0.25, mode, no_info.ptr, m3.ptr, _null())
            A.check()
            want = {"cstack_" + KERNEL[name]} | ({"cstack_lock", "cstack_blend"} if mode == LOCK else set())
            assert names == want, (names, want)
            for a in (bare, no_mag, no_info):
                assert np.array_equal(a.get(np.uint32), full[0].get(np.uint32)), a.name
            assert np.array_equal(m3.get(np.uint32), full[1].get(np.uint32)) and np.array_equal(i2.get(np.uint64), full[2].get(np.uint64))


# ---------------------------------------------------------------- 6. formats and repeats
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
    """zstate, mag and info (cases U: tiled, D: direct; GIVEN at alpha 0, LOCK at alpha 0.25): sc16 / sc8 / uc8 in, the bits of the same
    call on the host-expanded ComplexF32"""
    code = {"sc16": 1, "sc8": 2, "uc8": 3}[fmt]
    for name in ("U", "D"):
        c = CASES[name]
        raw, scale, z = _quantised(name, fmt)
        n, P = z.size, c["y"] * c["x"]
        S_in = _state_in(name)
        for mode, alpha in ((GIVEN, 0.0), (LOCK, 0.25)):
            with D.Arenas(ctx) as A:
                d_raw, d_z = A.input("raw", raw, 0), A.input("expanded", z, 8)
                outs = []
                for tag, ptr, cd, sc in (("raw", d_raw.ptr, code, scale), ("expanded", d_z.ptr, 0, 1.0)):
                    o = [A.output("zstate " + tag, 8 * P, 8), A.output("mag " + tag, 4 * P, 4), A.output("info " + tag, 64, 8)]
                    _fill(ctx, o[0], S_in)
                    _case_d(ctx, name, ptr, n, 0.37, alpha, mode, o[0].ptr, o[1].ptr, o[2].ptr, fmt=cd, scale=sc)
                    outs.append(o)
                A.check()
                for a, b in zip(*outs):
                    assert np.array_equal(a.get(np.uint32), b.get(np.uint32)), (name, fmt, mode, a.name)
                ref, _ = R.step(R.zmean(R.samples(z), c["t0"], c["T"], KAPPA_TRUE, 0.37, c["F"], c["y"], c["x"]), 0.0, GIVEN)
                if mode == GIVEN:
                    err = float(np.max(np.abs(outs[1][0].get(C64).astype(np.complex128) - ref)))
                    assert err <= R.eps_s(c["F"], np.abs(R.samples(z)).max()), "and they are the stack of that buffer"


@pytest.mark.parametrize("mode", [GIVEN, LOCK])
@pytest.mark.parametrize("name", ["U", "D", "X"])
def test_two_calls_leave_identical_bits(ctx, name, mode):
    """the same call twice, zstate at 0 and at 8 mod 16 (in LOCK mode: the two-pixel and the one-pixel blend): identical bytes in
    zstate, mag and info"""
    c = CASES[name]
    iq = _capture(name)[0]
    P = c["y"] * c["x"]
    S_in = _state_in(name)
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, IQ_PHASE[name])
        outs = []
        for k in range(2):
            o = [A.output(f"zstate {k}", 8 * P, 8 * k), A.output(f"mag {k}", 4 * P, 4 + 8 * k), A.output(f"info {k}", 64, 8 * k)]
            _fill(ctx, o[0], S_in)
            _case_d(ctx, name, d_iq.ptr, iq.size, 0.37, 0.25, mode, o[0].ptr, o[1].ptr, o[2].ptr)
            outs.append(o)
        A.check()
        for a, b in zip(*outs):
            assert np.array_equal(a.get(np.uint32), b.get(np.uint32)), a.name
        assert np.isfinite(outs[0][2].get(np.float64)).all() and np.isfinite(outs[0][0].get(F32)).all()


# ---------------------------------------------------------------- 7. the capability
CAP = dict(y=66, x=160, T=9150.37, snr_db=-16.0, buffers=6, step_at=3, step_rad=2.0)


def _corr(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float(np.dot(a, b) / math.sqrt(np.dot(a, a) * np.dot(b, b)))


@functools.lru_cache(maxsize=None)
def _cap_buffers(step):
    """six contiguous buffers of n = ceil(9 T) + 7 samples of one capture at -16 dB; step: the capture's carrier phase is raised by
    2 rad from buffer 3 on (a retune, a dropped buffer)"""
    synth = _pkg("synth")
    y, x, T = CAP["y"], CAP["x"], CAP["T"]
    n = int(math.ceil(9 * T)) + 7
    out = []
    for b in range(CAP["buffers"]):
        phi0 = 0.3 + (CAP["step_rad"] if step and b >= CAP["step_at"] else 0.0)
        iq = synth.synth_leak(60.0 * T, x, y, 60.0, n, n0=b * n, snr_db=CAP["snr_db"], phi0=phi0)
        iq.setflags(write=False)
        out.append(iq)
    return tuple(out)


def _cap_card():
    synth = _pkg("synth")
    b, y, x = synth.BLANK_BOX, CAP["y"], CAP["x"]
    return synth.test_card(x, y, row0=int(round(b["row0_frac"] * y)) % y, col0=int(round(b["col0_frac"] * x)) % x)


def _cap_plan():
    """[(F, t0, phi, alpha)] of the six buffers: chained by cstack_plan, alpha_b = b / (b + 1) (the running mean)"""
    T, n = CAP["T"], int(math.ceil(9 * CAP["T"])) + 7
    t0, phi, out = 0.0, 0.0, []
    for b in range(CAP["buffers"]):
        F, nt0, nphi = R.cstack_plan(n, t0, T, KAPPA_TRUE, phi)
        out.append((F, t0, phi, b / (b + 1.0)))
        t0, phi = nt0, nphi
    return out


def capability_reference(step):
    """(lock, given, magnitudes): the correlations of the three pictures with the noiseless card, from tests/cstack_ref.py alone"""
    import cfold_ref as CR
    y, x, T = CAP["y"], CAP["x"], CAP["T"]
    S = {GIVEN: None, LOCK: None}
    st = None
    for iq, (F, t0, phi, alpha) in zip(_cap_buffers(step), _cap_plan()):
        z = R.samples(iq)
        for mode in (GIVEN, LOCK):
            S[mode], _, _ = R.cstack(z, t0, T, KAPPA_TRUE, phi, F, y, x, alpha, mode, S[mode])
        st = CR.cfold(z, t0, T, KAPPA_TRUE, F, y, x, alpha, st)
    card = _cap_card().reshape(-1, order="F")
    return _corr(np.abs(S[LOCK]), card), _corr(np.abs(S[GIVEN]), card), _corr(st, card)


def _capability_gpu(ctx, step):
    y, x, T = CAP["y"], CAP["x"], CAP["T"]
    P = y * x
    with D.Arenas(ctx) as A:
        zs = {m: A.output("zstate " + MODE_NAME[m], 8 * P, 8) for m in (GIVEN, LOCK)}
        mag = {m: A.output("mag " + MODE_NAME[m], 4 * P, 4) for m in (GIVEN, LOCK)}
        d_st = A.output("cfold state", 4 * P, 12)
        for b, (iq, (F, t0, phi, alpha)) in enumerate(zip(_cap_buffers(step), _cap_plan())):
            d_iq = A.input(f"iq {b}", iq, 8 * (b % 2))
            for m in (GIVEN, LOCK):
                _stack_d(ctx, d_iq.ptr, 0, 1.0, iq.size, t0, T, KAPPA_TRUE, phi, F, y, x, alpha, m, zs[m].ptr, mag[m].ptr, _null())
            ctx.call("tsdr_cfold_iq_d", d_iq.ptr, 0, C.c_float(1.0), iq.size, C.c_double(t0), C.c_double(T), C.c_double(KAPPA_TRUE), F, y, x,
                     C.c_float(alpha), d_st.ptr)
        A.check()
        card = _cap_card().reshape(-1, order="F")
        return _corr(mag[LOCK].get(F32), card), _corr(mag[GIVEN].get(F32), card), _corr(d_st.get(F32), card)


def test_complex_state_keeps_the_picture_magnitude_averaging_loses(ctx):
    """66 x 160, T 9150.37, -16 dB per sample, six contiguous buffers of ceil(9 T) + 7 samples (8 or 9 frames each) chained by
    cstack_plan with alpha_b = b / (b + 1).  Correlation with the noiseless card of (a) LOCK's mag, (b) GIVEN's mag, (c) the state of
    tsdr_cfold_iq_d with the same alphas.  tests/cstack_ref.py gives (capability_reference):
        without a phase step   (a) 0.617  (b) 0.617  (c) 0.470
        the capture's carrier phase raised by 2 rad from buffer 3 on (buffers counted from 0)   (a) 0.620  (b) 0.319  (c) 0.476
    The thresholds take about a third of each gap as margin: without the step (a), (b) >= 0.55 and each >= (c) + 0.08; with it
    (a) >= 0.55 and (b) <= (a) - 0.15."""
    a, b, c = _capability_gpu(ctx, False)
    print(f"capability, no step: lock {a:.3f}, given {b:.3f}, magnitudes {c:.3f}")
    assert a >= 0.55 and b >= 0.55 and a >= c + 0.08 and b >= c + 0.08, (a, b, c)
    a, b, c = _capability_gpu(ctx, True)
    print(f"capability, 2 rad step from buffer 3 on: lock {a:.3f}, given {b:.3f}, magnitudes {c:.3f}")
    assert a >= 0.55 and b <= a - 0.15, (a, b, c)


# ---------------------------------------------------------------- 8. the host form
@pytest.mark.parametrize("mode", [GIVEN, LOCK])
def test_host_form_agrees_with_the_device_form(ctx, mode):
    """Context.cstack (host arrays, tsdr_cstack_iq) and the device form give the same bits; the caller's state is an input"""
    name = "U"
    c = CASES[name]
    iq = _capture(name)[0]
    y, x, P = c["y"], c["x"], c["y"] * c["x"]
    S_in = _state_in(name)
    st = np.asfortranarray(S_in.reshape((y, x), order="F"))
    keep = st.copy()
    for alpha in (0.0, 0.25):
        zs, mag, info = ctx.cstack(iq, c["t0"], c["T"], KAPPA_TRUE, 0.37, c["F"], y, x, alpha=alpha, mode=MODE_NAME[mode].lower(),
                                   zstate=st if alpha else None)
        assert zs.shape == (y, x) and zs.dtype == C64 and mag.shape == (y, x) and mag.dtype == F32 and info.shape == (8,)
        assert np.array_equal(st, keep)
        with D.Arenas(ctx) as A:
            d_iq = A.input("iq", iq, 8)
            d_zs, d_mag, d_info = A.output("zstate", 8 * P, 8), A.output("mag", 4 * P, 12), A.output("info", 64, 8)
            _fill(ctx, d_zs, S_in)
            ctx.cstack_d(d_iq.addr, "cf32", 1.0, iq.size, c["t0"], c["T"], KAPPA_TRUE, 0.37, c["F"], y, x, alpha, mode, d_zs.addr, d_mag.addr,
                         d_info.addr)
            A.check()
            assert np.array_equal(zs.reshape(-1, order="F").view(np.uint32), d_zs.get(np.uint32))
            assert np.array_equal(mag.reshape(-1, order="F").view(np.uint32), d_mag.get(np.uint32))
            assert np.array_equal(info.view(np.uint64), d_info.get(np.uint64))
    # the raw symbol with mag = info = NULL
    raw = S_in.copy()
    rc = ctx.lib.tsdr_cstack_iq(ctx.h, C.c_void_p(iq.ctypes.data), 0, 1.0, iq.size, c["t0"], c["T"], KAPPA_TRUE, 0.37, c["F"], y, x, 0.25, mode,
                                C.c_void_p(raw.ctypes.data), None, None)
    assert rc == 0 and np.array_equal(raw.view(np.uint32), zs.reshape(-1, order="F").view(np.uint32))


# ---------------------------------------------------------------- 9. refusals and untouched memory
def test_refusals_leave_everything_untouched(ctx):
    """every TSDR_EINVAL of the header, and F == 0 (TSDR_OK): nothing is launched, the sentinels around iq, zstate, mag and info and
    the sentinel-filled outputs themselves are as uploaded"""
    c = CASES["U"]
    iq = _capture("U")[0]
    raw = np.zeros(2 * 4096, np.int16)
    n, P, y, x, F, t0, T = iq.size, c["y"] * c["x"], c["y"], c["x"], c["F"], c["t0"], c["T"]
    nan, inf = float("nan"), float("inf")
    with D.Arenas(ctx) as A:
        d_iq, d_raw = A.input("iq", iq, 8), A.input("raw", raw, 0)
        d_zs, d_mag, d_info = A.output("zstate", 8 * P, 8), A.output("mag", 4 * P, 4), A.output("info", 64, 8)
        good = dict(iq=d_iq.addr, fmt=0, n=n, t0=t0, T=T, k=KAPPA_TRUE, phi=0.37, F=F, y=y, x=x, alpha=0.0, mode=LOCK, zs=d_zs.addr,
                    mag=d_mag.addr, info=d_info.addr)

        def stack(**kw):
            k = dict(good, **kw)
            _stack_d(ctx, C.c_void_p(k["iq"]), k["fmt"], 1.0, k["n"], k["t0"], k["T"], k["k"], k["phi"], k["F"], k["y"], k["x"], k["alpha"],
                     k["mode"], C.c_void_p(k["zs"]), C.c_void_p(k["mag"]), C.c_void_p(k["info"]))

        bad = [dict(iq=0), dict(zs=0), dict(fmt=4), dict(fmt=-1), dict(y=0), dict(x=-3), dict(y=65536, x=32768), dict(n=1), dict(n=1 << 31),
               dict(F=-1), dict(T=nan), dict(T=inf), dict(t0=nan), dict(t0=inf), dict(T=1.5), dict(t0=-0.5), dict(k=nan), dict(k=inf),
               dict(phi=nan), dict(phi=inf), dict(phi=-inf), dict(mode=2), dict(mode=-1), dict(F=F + 1), dict(t0=t0 + 20.0), dict(n=n - 20),
               dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan), dict(zs=d_zs.addr + 4), dict(mag=d_mag.addr + 2),
               dict(info=d_info.addr + 4), dict(iq=d_iq.addr + 4), dict(iq=d_raw.addr + 8, fmt=1, n=2048, F=1),
               dict(iq=d_raw.addr + 4, fmt=2, n=2048, F=1)]

        def refused():
            for kw in bad:
                with pytest.raises(AssertionError, match="invalid|cstack"):
                    stack(**kw)
            stack(F=0)
            assert ctx.lib.tsdr_cstack_iq_d(None, d_iq.ptr, 0, 1.0, n, t0, T, KAPPA_TRUE, 0.37, F, y, x, 0.0, LOCK, d_zs.ptr, d_mag.ptr,
                                            d_info.ptr) == -1

        assert _profiled(ctx, refused) == set(), "nothing is enqueued"
        A.check()
        for a in (d_zs, d_mag, d_info):
            assert np.array_equal(a.get(np.uint32), D.sentinel_words(a.size // 4)[a.lead // 4: (a.lead + a.payload) // 4]), a.name
        # and the context still serves valid calls afterwards: negative kappa and phi are accepted
        stack(k=-2.5, phi=-7.25)
        A.check()
        assert np.all(np.isfinite(d_zs.get(F32))) and np.all(np.isfinite(d_mag.get(F32))) and np.all(np.isfinite(d_info.get(np.float64)))
    # host form: the same refusals, host arrays untouched; F == 0 touches nothing
    zs, mag, info = np.full(2 * P, 7.0, F32), np.full(P, 7.0, F32), np.full(8, 7.0)
    z = iq.copy()
    for kw in (dict(T=nan), dict(phi=nan), dict(mode=3), dict(F=F + 1), dict(alpha=2.0), dict(fmt=5), dict(y=0), dict(zs=0), dict(F=0)):
        k = dict(dict(good, zs=zs.ctypes.data), **kw)
        rc = ctx.lib.tsdr_cstack_iq(ctx.h, C.c_void_p(z.ctypes.data), k["fmt"], 1.0, n, k["t0"], k["T"], k["k"], k["phi"], k["F"], k["y"], k["x"],
                                    k["alpha"], k["mode"], C.c_void_p(k["zs"]), C.c_void_p(mag.ctypes.data), C.c_void_p(info.ctypes.data))
        assert rc == (0 if kw == dict(F=0) else -1), kw
    assert np.all(zs == 7.0) and np.all(mag == 7.0) and np.all(info == 7.0) and np.array_equal(z, iq)
