"""Host-side checks of carrier tracking (no GPU): include/tempest_hip_ctrack.h, its ctypes table (_lib._SIGS_CTRACK), its Python module
(ctrack.py) and its Julia shim (julia/TempestHIP_ctrack.jl) agree with each other and with the library; the numpy reference the GPU
tests compare against (tests/ctrack_ref.py) on answers known without it -- fit_track on a known quadratic, constant_track against
cstack_ref's weight, the constant track against cstack_ref.cstack; and the two capabilities the feature exists for, on the CPU: a
carrier that drifts inside a buffer, and a retune between buffers."""
import ctypes as C
import functools
import inspect
import math
import os
import re

import numpy as np

import cfold_ref as CF
import cstack_ref as CS
import ctrack_ref as R
import test_dptr_host as DH
import test_hires_host as HH
import test_julia_shim_static as JS

ROOT = HH.ROOT
CTRACK_H = os.path.join(ROOT, "include", "tempest_hip_ctrack.h")
SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP_ctrack.jl")
CSRC = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc")

SYMS = ["tsdr_ctrack_probe_iq", "tsdr_ctrack_probe_iq_d", "tsdr_ctrack_stack_iq", "tsdr_ctrack_stack_iq_d"]
HEAD = ["tsdr_ctx *ctx", "const void *iq", "int iq_fmt", "float scale", "size_t n", "double t0", "double T", "const double *track",
        "int n_frames", "int y_t", "int x_t"]
STACK = HEAD + ["float alpha", "int mode", "float *zstate", "float *mag", "double *info"]
PROBE = HEAD + ["const float *zref", "double *out"]


# ---------------------------------------------------------------- header, table, library, shims
def test_header_declares_the_four_forms():
    p = HH._protos(CTRACK_H)
    assert sorted(p) == SYMS
    assert p["tsdr_ctrack_stack_iq"] == p["tsdr_ctrack_stack_iq_d"] == STACK
    assert p["tsdr_ctrack_probe_iq"] == p["tsdr_ctrack_probe_iq_d"] == PROBE
    main = open(HH.MAIN_H).read()
    assert main.count('#include "tempest_hip_ctrack.h"') == 1
    assert main.index('#include "tempest_hip_ctrack.h"') > main.index('#include "tempest_hip_cstack.h"')
    assert not re.search(r"tsdr_ctrack", HH._strip(HH.MAIN_H))
    guard = open(CTRACK_H).read()
    assert "#ifndef TEMPEST_HIP_CTRACK_H" in guard and "#ifndef TEMPEST_HIP_CSTACK_H\n#error" in guard


def test_header_states_the_contract():
    src = " ".join(open(CTRACK_H).read().split())
    for phrase in ("INPUT", "TRACK", "SAMPLING", "RESULT", "ACCURACY", "REFUSALS", "COST", "REPRODUCIBILITY", "FORMAT INVARIANCE",
                   "c_l = fl64((l + 1/2) / y_t)", "x = fma(b_f, c_l, a_f)", "r = x - floor(x)", "piecewise constant per line",
                   "at most |b_f| / (2 y_t) turns", "the caller keeps it small", "|a_f| + |b_f| <= 2^20", "With b_f == 0, x = a_f exactly",
                   "a_f = fl64(fl64(f * kappa) + phi) and b_f = 0", "have the bits of tsdr_cstack_iq_d", "the state is NOT READ",
                   "track NULL", "track not 8-byte aligned", "a track entry that is not finite", "NaN pixels",
                   "track may be NULL: the zero track", "re = fsub(fmul(wr, zr), fmul(wi, zi)), im = fadd(fmul(wr, zi), fmul(wi, zr))",
                   "Re += vr*sr + vi*si, Im += vi*sr - vr*si", "out[4f .. 4f+3] = Re rho_f, Im rho_f, E_f, gamma_f",
                   "gamma_f = |rho_f| / sqrt(E_f * E_s), 0 unless that product is > 0", "out[4F] = E_s", "No float atomics",
                   "|v - ref| <= sqrt(2) * 12 * u * amax = eps_t",
                   "|rho_f - ref| <= eps_t * sqrt(P * E_s) + 2^-36 * sqrt(E_f * E_s)",
                   "|E_f - ref| <= 2 * eps_t * sqrt(P * ref) + P * eps_t^2 + 2^-36 * ref", "|E_s - ref| <= 2^-36 * ref",
                   "zref or out NULL", "F == 0 is TSDR_OK and writes nothing", "nothing written and nothing enqueued",
                   '"ctrack_stack_tile"', '"ctrack_stack_direct"', '"ctrack_probe_tile"', '"ctrack_probe_direct"', '"ctrack_probe_sum"',
                   '"cstack_lock"', '"cstack_blend"', "TSDR_CFOLD_STAGE_MAX", '"wait_ms"'):
        assert phrase in src, phrase
    assert R.TERM == 12


def test_header_table_and_library_agree():
    lib = HH._pkg("_lib")
    assert sorted(HH._protos(CTRACK_H)) == SYMS == lib.exported_names_ctrack()
    for other in (lib._SIGS, lib._SIGS_IQ, lib._SIGS_CPLX, lib._SIGS_HIRES, lib._SIGS_REGISTER, lib._SIGS_DISPLAY, lib._SIGS_FOLD,
                  lib._SIGS_CFOLD, lib._SIGS_CSTACK):
        assert not set(other) & set(lib._SIGS_CTRACK)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    ct = {"i32": C.c_int, "i64": C.c_size_t, "f32": C.c_float, "f64": C.c_double}
    for sym, params in HH._protos(CTRACK_H).items():
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_ctrack.h but not exported"
        res, args = lib._SIGS_CTRACK[sym]
        assert getattr(bound, sym).restype is C.c_int and getattr(bound, sym).argtypes == args, sym
        assert res is C.c_int and len(args) == len(params), sym
        for k, (a, p) in enumerate(zip(args, params)):
            cls = JS.c_class(p)
            assert (a is C.c_void_p) if cls == "ptr" else (a is ct[cls]), (sym, k, p, a)


def test_every_ccall_of_the_shim_matches_its_prototype():
    protos = {name: ("i32", [JS.c_class(p) for p in params]) for name, params in HH._protos(CTRACK_H).items()}
    jl = open(SHIM).read()
    seen = []
    for m in re.finditer(r"ccall\(\(:(tsdr_[a-z0-9_]+),\s*LIB\),", jl):
        i = jl.index("(", m.start())
        depth, j = 0, i
        while True:
            depth += jl[j] == "("
            depth -= jl[j] == ")"
            if depth == 0:
                break
            j += 1
        parts = JS.split_args(jl[i + 1:j])
        ret, types = JS.jl_class(parts[1]), [JS.jl_class(t) for t in JS.split_args(parts[2][1:-1]) if t]
        seen.append(m.group(1))
        cret, cparams = protos[m.group(1)]
        assert (ret, types, len(parts) - 3) == (cret, cparams, len(cparams)), (m.group(1), ret, types, cret, cparams)
    assert sorted(seen) == SYMS, "one ccall per symbol"
    main = open(HH.SHIM).read()
    assert main.count('include("TempestHIP_ctrack.jl")') == 1
    assert main.index('include("TempestHIP_ctrack.jl")') > main.index('include("TempestHIP_cstack.jl")')
    for name in ("constant_track", "fit_track", "hip_ctrack_stack!", "hip_ctrack_stack_d!", "hip_ctrack_probe", "hip_ctrack_probe_d!"):
        assert re.search(r"\nfunction " + re.escape(name) + r"\(", jl), name


def test_python_interface_and_delegation():
    api, mod = HH._pkg("api"), HH._pkg("ctrack")
    head = ["iq", "fmt", "scale", "n", "t0", "T", "track", "n_frames", "y_t", "x_t"]
    want = {"ctrack_stack_d": head + ["alpha", "mode", "zstate", "mag", "info"], "ctrack_probe_d": head + ["zref", "out"],
            "ctrack_stack": ["iq", "t0", "T", "track", "n_frames", "y_t", "x_t", "alpha", "mode", "zstate", "fmt", "scale"],
            "ctrack_probe": ["iq", "t0", "T", "track", "n_frames", "y_t", "x_t", "zref", "fmt", "scale"],
            "refine_track": ["iq_d", "fmt", "scale", "n", "t0", "T", "n_frames", "y_t", "x_t", "kappa", "iterations", "degree", "zstate", "mag"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(api.Context, name)).parameters) == ["self"] + params, name
        assert list(inspect.signature(getattr(mod, name)).parameters) == ["ctx"] + params, name
    for fn in (api.Context.constant_track, mod.constant_track):
        p = inspect.signature(fn).parameters
        assert list(p) == ["n_frames", "kappa", "phi", "slope"] and p["phi"].default == 0.0 and p["slope"].default == 0.0
    for fn in (api.Context.fit_track, mod.fit_track):
        p = inspect.signature(fn).parameters
        assert list(p) == ["rho", "track", "degree"] and p["degree"].default == 2
    p = inspect.signature(mod.refine_track).parameters
    assert p["iterations"].default == 2 and p["degree"].default == 2
    called = DH.called_symbols(open(mod.__file__).read())
    assert set(SYMS) <= called
    assert not (DH.called_symbols(open(api.__file__).read()) & set(SYMS)), "api.py delegates; it calls no symbol itself"
    import tempestsdr_jl_amd as T
    for name in ("ctrack_stack", "ctrack_stack_d", "ctrack_probe", "ctrack_probe_d", "constant_track", "fit_track", "refine_track"):
        assert getattr(T, name) is getattr(mod, name), name
    pkg = os.path.dirname(mod.__file__)
    for f in os.listdir(pkg):
        if f.endswith(".py") and f not in ("ctrack.py", "_lib.py"):
            assert "tsdr_ctrack" not in open(os.path.join(pkg, f)).read(), f


def test_every_entry_point_is_called_by_the_gpu_suite():
    text = open(os.path.join(ROOT, "tests", "test_ctrack_gpu.py")).read()
    called = DH.called_symbols(text) | set(re.findall(r"\b(tsdr_ctrack_\w+)", text))
    assert set(SYMS) <= called, sorted(set(SYMS) - called)
    assert "import dptr_util as D" in text and "D.Arenas(" in text and "pytestmark = pytest.mark.gpu" in text
    assert "from test_cstack_gpu import" in text and "CASES" in text


def test_kernel_source_keeps_its_launch_rules():
    src = open(os.path.join(CSRC, "raster_ctrack.hip")).read()
    code = re.sub(r"//.*", "", src)
    for name in ("ctrack_stack_tile", "ctrack_stack_direct", "ctrack_probe_tile", "ctrack_probe_direct", "ctrack_probe_sum"):
        assert f'TSDR_LAUNCH(ctx, "{name}"' in code, name
    assert re.search(r"k_fold_engine<Tracked, kFoldTileP, kFoldTileWaves, 1, true, false>", code)
    assert re.search(r"k_fold_engine<Tracked, kFoldDirectP, kFoldDirectWaves, 1, false, false>", code)
    assert "Stacked::stack(" in code and "stack_finish(" in code and "stack_ws(" in code, "the stack's epilogue, lock and blend are cstack's"
    assert "hipLaunchKernelGGL" not in code and not re.search(r"\batomic\w*\(", code) and not re.search(r"\basm\b", code)
    assert len(re.findall(r"\bHostStage \w+\(ctx\)", code)) == 2 and not re.search(r"scratch\(WS_(IN|OUT|AUX)\b", code)
    assert "line_weights = true" in code
    engine = open(os.path.join(CSRC, "fold_engine.h")).read()
    assert "if constexpr (Fl::line_weights)" in engine
    for f in ("raster_fold.hip", "raster_cfold.hip", "raster_cstack.hip"):
        assert "line_weights = false" in open(os.path.join(CSRC, f)).read(), f
    ops = open(os.path.join(CSRC, "coherent_ops.h")).read()
    assert "fma(b, c, a)" in ops and "coh_line_weight(" in code and "coh_mul(" in code and "coh_blend(" in code


def test_refusals_need_no_device():
    """a NULL context is refused before anything else; nothing is dereferenced"""
    lib = HH._pkg("_lib").load()
    z = np.zeros(16, np.complex64)
    zs, mag, info, out = np.zeros(8, np.float32), np.zeros(4, np.float32), np.zeros(8), np.zeros(5)
    track = np.zeros(2)
    head = (None, z.ctypes.data, 0, 1.0, 16, 0.0, 8.0, track.ctypes.data, 1, 2, 2)
    stack = head + (0.0, 1, zs.ctypes.data, mag.ctypes.data, info.ctypes.data)
    probe = head + (zs.ctypes.data, out.ctypes.data)
    assert lib.tsdr_ctrack_stack_iq(*stack) == -1 and lib.tsdr_ctrack_stack_iq_d(*stack) == -1
    assert lib.tsdr_ctrack_probe_iq(*probe) == -1 and lib.tsdr_ctrack_probe_iq_d(*probe) == -1
    assert not zs.any() and not mag.any() and not info.any() and not out.any()


# ---------------------------------------------------------------- the reference and the fit, on answers known without them
def test_fit_track_recovers_a_known_quadratic_across_a_wrap():
    """rho_f = A_f exp(2 pi i q(f)) with q a quadratic that runs over 2.9 turns in 24 frames: fit_track returns q to 1e-9 turns (up to
    the whole turns of its constant term), in the reference and in the bindings, and the track moves by q(f) - q'(f)/2 and q'(f)"""
    mod = HH._pkg("ctrack")
    F = 24
    f = np.arange(F, dtype=np.float64)
    q = np.poly1d([0.006, -0.02, 0.43])
    assert abs(q(F - 1) - q(0)) > 2.5 and np.max(np.abs(np.diff(q(f)))) < 0.5
    rho = (1.0 + 0.5 * np.cos(f)) * np.exp(2j * np.pi * q(f))
    t0 = R.constant_track(F, 0.3, 0.1, 0.25)
    for fit in (R.fit_track, mod.fit_track):
        t, p = fit(rho, t0, 2)
        d = np.asarray(p.coeffs) - np.asarray(q.coeffs)
        assert abs(d[0]) <= 1e-9 and abs(d[1]) <= 1e-9 and abs(d[2] - round(d[2])) <= 1e-9, d
        k = round(d[2])
        assert np.max(np.abs(t[:, 0] - (t0[:, 0] + q(f) + k - 0.5 * q.deriv()(f)))) <= 1e-9
        assert np.max(np.abs(t[:, 1] - (t0[:, 1] + q.deriv()(f)))) <= 1e-9
    a, b = R.fit_track(rho, t0, 2)[0], mod.fit_track(rho, t0, 2)[0]
    assert np.max(np.abs(a - b)) <= 1e-9, "the bindings' fit is the reference's"


def test_fit_track_ignores_a_frame_without_weight():
    mod = HH._pkg("ctrack")
    F = 12
    f = np.arange(F, dtype=np.float64)
    q = np.poly1d([0.004, 0.11, -0.2])
    rho = np.exp(2j * np.pi * q(f)) * (2.0 + np.sin(f))
    holed = rho.copy()
    holed[[0, 5, 6]] = 0.0
    t0 = np.zeros((F, 2))
    for fit in (R.fit_track, mod.fit_track):
        full, hole = fit(rho, t0, 2), fit(holed, t0, 2)
        assert np.max(np.abs(full[0] - hole[0])) <= 1e-9 and np.max(np.abs(full[1].coeffs - hole[1].coeffs)) <= 1e-9
        none = fit(np.zeros(F, complex), t0, 2)
        assert np.array_equal(none[0], t0)


def test_constant_track_is_the_argument_of_cstacks_weight():
    """a_f == fl64(fl64(f * kappa) + phi) bit for bit -- what cstack_ref.weight passes to frac, what the kernel passes to coh_weight --
    and b_f == slope, in the reference and in the bindings"""
    mod = HH._pkg("ctrack")
    for kappa, phi, slope in ((1000.0 / 60.0 % 1.0, 0.37, 0.0), (-2.5, -7.25, 3.0 + 1.0 / 3.0), (0.7708, 0.0, 0.0), (1e-3, 123.456, -0.125)):
        for make in (R.constant_track, mod.constant_track):
            t = make(40, kappa, phi, slope)
            assert t.shape == (40, 2) and t.dtype == np.float64 and t.flags.c_contiguous
            for f in range(40):
                want = float(f) * float(kappa) + float(phi)
                assert t[f, 0] == want and t[f, 1] == slope, (f, kappa, phi)
                w = CS.weight(f, kappa, phi)
                r = CS.frac(t[f, 0])
                assert w == complex(math.cos(2.0 * math.pi * r), -math.sin(2.0 * math.pi * r))


def test_constant_track_reference_equals_cstack_reference():
    """ctrack_ref with constant_track(F, kappa, phi) is cstack_ref.cstack to 1e-12 (relative to the largest pixel), both modes"""
    y, x, T, F, t0 = 13, 21, 301.7, 5, 2.25
    rng = np.random.default_rng(7)
    n = int(math.ceil(t0 + F * T)) + 3
    z = CF.samples((rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64))
    S = (rng.normal(size=y * x) + 1j * rng.normal(size=y * x)).astype(np.complex64).astype(np.complex128)
    for kappa, phi in ((0.31, 0.0), (0.6667, 0.37)):
        for mode, alpha in ((R.GIVEN, 0.0), (R.GIVEN, 0.25), (R.LOCK, 0.25)):
            a = R.ctrack(z, t0, T, R.constant_track(F, kappa, phi), F, y, x, alpha, mode, S)
            b = CS.cstack(z, t0, T, kappa, phi, F, y, x, alpha, mode, S)
            scale = float(np.abs(b[0]).max())
            assert np.max(np.abs(a[0] - b[0])) <= 1e-12 * scale and np.max(np.abs(a[1] - b[1])) <= 1e-12 * scale
            assert np.max(np.abs(a[2] - b[2])) <= 1e-12 * max(1.0, float(np.abs(b[2]).max()))
    # and the probe of the zero track against S is the frame's plain inner product
    rho, E_f, gamma, E_s = R.probe(z, t0, T, None, F, y, x, S)
    zero = R.probe(z, t0, T, np.zeros((F, 2)), F, y, x, S)
    assert np.max(np.abs(rho - zero[0])) <= 1e-12 * np.abs(rho).max() and E_s == zero[3]
    v0 = CF.to_state(R.frame_samples(z, t0, T, 0, y, x), y, x)
    assert abs(rho[0] - np.sum(v0 * np.conj(S))) <= 1e-12 * abs(rho[0]) and abs(E_f[0] - np.sum(np.abs(v0) ** 2)) <= 1e-12 * E_f[0]
    assert np.all(gamma <= 1.0) and np.all(gamma >= 0.0)


# ---------------------------------------------------------------- the two capabilities, on the CPU
CAP = dict(y=66, x=160, T=9150.37, t0=3.25, snr_db=-10.0)
KAPPA_TRUE = (1000.0 / 60.0) % 1.0
DRIFT = dict(frames=24, chi=0.012, kappa=0.7708)
RETUNE = dict(df=1200.0, dkappa=200.0 / 60.0, alpha=0.5)


def corr(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float(np.dot(a, b) / math.sqrt(np.dot(a, a) * np.dot(b, b)))


def cap_card():
    """the noiseless card of the capability geometry, in state order"""
    synth = HH._pkg("synth")
    b, y, x = synth.BLANK_BOX, CAP["y"], CAP["x"]
    return synth.test_card(x, y, row0=int(round(b["row0_frac"] * y)) % y, col0=int(round(b["col0_frac"] * x)) % x).reshape(-1, order="F")


@functools.lru_cache(maxsize=None)
def drift_captures():
    """(without drift, with drift): n = ceil(25 T) + 7 samples at -10 dB; the second multiplied by exp(2 pi i chi t^2 / 2), t = k / T"""
    synth = HH._pkg("synth")
    T = CAP["T"]
    n = int(math.ceil(25 * T)) + 7
    iq = synth.synth_leak(60.0 * T, CAP["x"], CAP["y"], 60.0, n, snr_db=CAP["snr_db"])
    t = np.arange(n, dtype=np.float64) / T
    drifted = (iq.astype(np.complex128) * np.exp(2j * np.pi * 0.5 * DRIFT["chi"] * t * t)).astype(np.complex64)
    for a in (iq, drifted):
        a.setflags(write=False)
    return iq, drifted


@functools.lru_cache(maxsize=None)
def retune_buffers():
    """two contiguous buffers of n = ceil(13 T) + 7 samples at -10 dB, the second with df = 1200 Hz: [(iq, t0, F)]"""
    synth = HH._pkg("synth")
    T = CAP["T"]
    n = int(math.ceil(13 * T)) + 7
    a = synth.synth_leak(60.0 * T, CAP["x"], CAP["y"], 60.0, n, snr_db=CAP["snr_db"])
    b = synth.synth_leak(60.0 * T, CAP["x"], CAP["y"], 60.0, n, n0=n, snr_db=CAP["snr_db"], df=RETUNE["df"])
    for q in (a, b):
        q.setflags(write=False)
    Fa, t0b = CS.fold_plan(n, CAP["t0"], T)
    Fb, _ = CS.fold_plan(n, t0b, T)
    return (a, CAP["t0"], Fa), (b, t0b, Fb)


@functools.lru_cache(maxsize=None)
def drift_reference():
    """correlations with the card from the references alone: (without drift, the constant kappa, after one pass, after two)"""
    y, x, T, t0, F = CAP["y"], CAP["x"], CAP["T"], CAP["t0"], DRIFT["frames"]
    iq, drifted = drift_captures()
    card = cap_card()
    clean = corr(np.abs(CS.zmean(CF.samples(iq), t0, T, KAPPA_TRUE, 0.0, F, y, x)), card)
    _, Z = R.refine_track(CF.samples(drifted), t0, T, F, y, x, DRIFT["kappa"], 2, 2)
    return (clean,) + tuple(corr(np.abs(z), card) for z in Z)


@functools.lru_cache(maxsize=None)
def retune_reference():
    """(first buffer alone, cstack LOCK gamma, its picture, tracked LOCK gamma, its picture) from the references alone"""
    y, x, T = CAP["y"], CAP["x"], CAP["T"]
    (a, t0a, Fa), (b, t0b, Fb) = retune_buffers()
    card = cap_card()
    S = CS.zmean(CF.samples(a), t0a, T, KAPPA_TRUE, 0.0, Fa, y, x)
    kb = CS.frac(KAPPA_TRUE + RETUNE["dkappa"])
    plain, info_p = CS.step(CS.zmean(CF.samples(b), t0b, T, kb, 0.0, Fb, y, x), RETUNE["alpha"], CS.LOCK, S)
    track = R.constant_track(Fb, KAPPA_TRUE + RETUNE["dkappa"], 0.0, RETUNE["dkappa"])
    _, mag, info_t = R.ctrack(CF.samples(b), t0b, T, track, Fb, y, x, RETUNE["alpha"], CS.LOCK, S)
    return corr(np.abs(S), card), float(info_p[5]), corr(np.abs(plain), card), float(info_t[5]), corr(mag, card)


def test_capability_a_drifting_carrier_inside_one_buffer():
    """66 x 160, T 9150.37, t0 3.25, -10 dB, 24 frames, a frequency ramp of 0.012 turns/frame per frame.  The best constant kappa
    (cfold_ref.ladder: 0.7708) folds to 0.314, below what the capture without drift gives (0.555); probing each frame against that
    blurred picture, fitting a weighted quadratic and refolding along the track gives 0.553 after one pass and 0.555 after two."""
    y, x, T, t0, F = CAP["y"], CAP["x"], CAP["T"], CAP["t0"], DRIFT["frames"]
    kappa_hat = CF.ladder(CF.samples(drift_captures()[1]), t0, T, F, y, x)[0]
    assert abs(kappa_hat - DRIFT["kappa"]) <= 1e-4, kappa_hat
    clean, const, one, two = drift_reference()
    print(f"drift: without 0.555 -> {clean:.3f}; constant kappa 0.314 -> {const:.3f}; one pass 0.553 -> {one:.3f}; two 0.555 -> {two:.3f}")
    assert abs(clean - 0.555) <= 0.002 and abs(const - 0.314) <= 0.002 and abs(one - 0.553) <= 0.002 and abs(two - 0.555) <= 0.002
    assert const <= 0.36 and two >= 0.50


def test_capability_a_retune_between_buffers():
    """two buffers of ceil(13 T) + 7 samples at -10 dB, the second retuned from 1000 to 1200 Hz (3.333 turns per frame more): cstack's
    LOCK at kappa_B = frac(kappa + 3.333) finds gamma 0.068 and its picture (0.392) is worse than the first buffer alone (0.468);
    with the ramp 3.333 (l + 1/2) / y_t removed per line the lock finds 0.646 and the picture scores 0.545"""
    first, g_plain, c_plain, g_track, c_track = retune_reference()
    print(f"retune: first buffer 0.468 -> {first:.3f}; cstack LOCK gamma 0.068 -> {g_plain:.3f}, picture 0.392 -> {c_plain:.3f}; "
          f"tracked gamma 0.646 -> {g_track:.3f}, picture 0.545 -> {c_track:.3f}")
    for got, want in ((first, 0.468), (g_plain, 0.068), (c_plain, 0.392), (g_track, 0.646), (c_track, 0.545)):
        assert abs(got - want) <= 0.002, (got, want)
    assert g_plain <= 0.15 and g_track >= 0.55 and c_plain < first < c_track
