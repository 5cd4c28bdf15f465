"""Host-side checks of the frame Gram matrix (no GPU): include/tempest_hip_gram.h, its ctypes table (_lib._SIGS_GRAM), its Python module
(gram.py) and its Julia shim (julia/TempestHIP_gram.jl) agree with each other and with the library; the host algorithms of gram.py
against tests/gram_ref.py and against answers known without either -- the fold's energy, the ladder's carrier, planted phases, planted
slopes; and the two capabilities the feature exists for, on the CPU reference: a carrier whose ramp no constant kappa can follow, and a
carrier on a random walk, with the inputs of tests/test_ctrack_host.py."""
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
import gram_ref as GR
import test_ctrack_host as TH
import test_dptr_host as DH
import test_hires_host as HH
import test_julia_shim_static as JS

ROOT = HH.ROOT
GRAM_H = os.path.join(ROOT, "include", "tempest_hip_gram.h")
SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP_gram.jl")
CSRC = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc")

SYMS = ["tsdr_ctrack_gram_iq", "tsdr_ctrack_gram_iq_d"]
GRAM = ["tsdr_ctx *ctx", "const void *iq", "int iq_fmt", "float scale", "size_t n", "double t0", "double T", "const double *track",
        "int n_frames", "int y_t", "int x_t", "double *gram"]


# ---------------------------------------------------------------- header, table, library, shims
def test_header_declares_both_forms():
    p = HH._protos(GRAM_H)
    assert sorted(p) == SYMS
    assert p["tsdr_ctrack_gram_iq"] == p["tsdr_ctrack_gram_iq_d"] == GRAM
    main = open(HH.MAIN_H).read()
    assert main.count('#include "tempest_hip_gram.h"') == 1
    assert main.index('#include "tempest_hip_gram.h"') > main.index('#include "tempest_hip_ctrack.h"')
    assert not re.search(r"tsdr_ctrack_gram|TSDR_GRAM", HH._strip(HH.MAIN_H))
    text = open(GRAM_H).read()
    assert "#ifndef TEMPEST_HIP_GRAM_H" in text and "#ifndef TEMPEST_HIP_CTRACK_H\n#error" in text
    assert re.search(r"#define TSDR_GRAM_MAX_FRAMES 64\b", text)
    chunk = int(re.search(r"#define TSDR_GRAM_CHUNK (\d+)\b", text).group(1))
    lib = HH._pkg("_lib")
    assert chunk <= 1024 and (lib.GRAM_MAX_FRAMES, lib.GRAM_CHUNK) == (64, chunk) == (GR.MAX_FRAMES, GR.CHUNK)
    assert re.search(r"#define TSDR_GRAM_MAX_TILES 65536\b", text) and lib.GRAM_MAX_TILES == 65536


def test_header_states_the_contract():
    src = " ".join(open(GRAM_H).read().split())
    for phrase in ("INPUT, TRACK, SAMPLING", "RESULT", "SUMMATION", "ACCURACY", "REPRODUCIBILITY, FORMAT INVARIANCE", "REFUSALS", "COST",
                   "Exactly tempest_hip_ctrack.h, 1. - 3.", "re = fsub(fmul(wr, zr), fmul(wi, zi)), im = fadd(fmul(wr, zi), fmul(wi, zr))",
                   "track may be NULL: the zero track", "gram holds 2*F*F doubles, row-major",
                   "gram[2*(f*F + g)] = Re G[f][g], gram[2*(f*F + g) + 1] = Im G[f][g]", "Both triangles are written",
                   "G[g][f] has the bits of conj(G[f][g])", "Im G[f][f] is +0", "G[f][f] is the probe's E_f",
                   "at most TSDR_GRAM_CHUNK = 1024 pixels", "bit for bit an fmaf chain", "chunks within a tile in chunk order",
                   "the tiles in tile order", "one lane per entry", "No float atomics",
                   "eps_t * (sqrt(P * E_f) + sqrt(P * E_g)) + P * eps_t^2", "c = 3 * TSDR_GRAM_CHUNK + 64 = 3136",
                   "c * u * sqrt(E_f * E_g)", "2^-36 * sqrt(E_f * E_g)",
                   "|G[f][g] - ref| <= eps_t * (sqrt(P * E_f) + sqrt(P * E_g)) + P * eps_t^2 + (c * u + 2^-36) * sqrt(E_f * E_g)",
                   "identical bits", "the bits of the host-expanded ComplexF32 buffer", "the host form has the bits of the device form",
                   "nothing written and nothing enqueued", "gram NULL", "n_frames > TSDR_GRAM_MAX_FRAMES", "TSDR_GRAM_MAX_TILES tiles or more",
                   "fewer than TSDR_GRAM_MAX_TILES = 2^16 tiles deep",
                   "gram or a non-NULL track not 8-byte aligned", "a track entry that is not finite",
                   "F == 0 is TSDR_OK and touches nothing", "Nothing is written outside gram[0 .. 2*F*F)",
                   '"gram_tile"', '"gram_direct"', '"gram_sum"', "TSDR_CFOLD_STAGE_MAX", "profiles/gram.json", '"wait_ms"'):
        assert phrase in src, phrase
    assert GR.CHAIN == 3136


def test_header_table_and_library_agree():
    lib = HH._pkg("_lib")
    assert sorted(HH._protos(GRAM_H)) == SYMS == lib.exported_names_gram() == sorted([lib.GRAM_IQ, lib.GRAM_IQ_D])
    for other in (lib._SIGS, lib._SIGS_IQ, lib._SIGS_CPLX, lib._SIGS_HIRES, lib._SIGS_REGISTER, lib._SIGS_DISPLAY, lib._SIGS_FOLD,
                  lib._SIGS_CFOLD, lib._SIGS_CSTACK, lib._SIGS_CTRACK):
        assert not set(other) & set(lib._SIGS_GRAM)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    ct = {"i32": C.c_int, "i64": C.c_size_t, "f32": C.c_float, "f64": C.c_double}
    for sym, params in HH._protos(GRAM_H).items():
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_gram.h but not exported"
        res, args = lib._SIGS_GRAM[sym]
        assert getattr(bound, sym).restype is C.c_int and getattr(bound, sym).argtypes == args, sym
        assert res is C.c_int and len(args) == len(params), sym
        for k, (a, p) in enumerate(zip(args, params)):
            cls = JS.c_class(p)
            assert (a is C.c_void_p) if cls == "ptr" else (a is ct[cls]), (sym, k, p, a)


def test_every_ccall_of_the_shim_matches_its_prototype():
    protos = {name: ("i32", [JS.c_class(p) for p in params]) for name, params in HH._protos(GRAM_H).items()}
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
    assert main.count('include("TempestHIP_gram.jl")') == 1
    assert main.index('include("TempestHIP_gram.jl")') > main.index('include("TempestHIP_ctrack.jl")')
    for name in ("hip_ctrack_gram", "hip_ctrack_gram_d!", "gram_energy", "gram_carrier", "gram_phases", "gram_track", "track_slopes",
                 "blind_track"):
        assert re.search(r"\nfunction " + re.escape(name) + r"\(", jl), name
    assert "LinearAlgebra.eigen(LinearAlgebra.Hermitian(" in jl
    tests = open(os.path.join(os.path.dirname(SHIM), "runtests.jl")).read()
    assert "TempestHIP.hip_ctrack_gram(" in tests and "TempestHIP.gram_phases(" in tests


def test_python_interface_and_delegation():
    api, mod, lib = HH._pkg("api"), HH._pkg("gram"), HH._pkg("_lib")
    want = {"ctrack_gram_d": ["iq", "fmt", "scale", "n", "t0", "T", "track", "n_frames", "y_t", "x_t", "gram"],
            "ctrack_gram": ["iq", "t0", "T", "track", "n_frames", "y_t", "x_t", "fmt", "scale"],
            "blind_track": ["iq_d", "fmt", "scale", "n", "t0", "T", "n_frames", "y_t", "x_t", "passes", "zstate", "mag"],
            "coherent_period_scan": ["iq_d", "fmt", "scale", "n", "t0", "y_t", "x_t", "periods"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(api.Context, name)).parameters) == ["self"] + params, name
        assert list(inspect.signature(getattr(mod, name)).parameters) == ["ctx"] + params, name
    static = {"gram_energy": ["G", "turns"], "gram_carrier": ["G", "oversample", "steps"], "gram_phases": ["G", "iters"],
              "gram_track": ["G", "track", "v"], "track_slopes": ["track"]}
    for name, params in static.items():
        for fn in (getattr(api.Context, name), getattr(mod, name)):
            assert list(inspect.signature(fn).parameters) == params, name
    p = inspect.signature(mod.blind_track).parameters
    assert p["passes"].default == 2 and p["zstate"].default is None and p["mag"].default is None
    assert inspect.signature(mod.gram_phases).parameters["iters"].default == 50
    assert inspect.signature(mod.gram_carrier).parameters["oversample"].default == 16
    # gram.py names the two symbols through _lib (the tsdr_ctrack prefix is ctrack.py's own in the package: test_ctrack_host); it
    # calls both, and no other module does
    src = open(mod.__file__).read()
    assert re.search(r"ctx\.call\(_lib\.GRAM_IQ_D,", src) and re.search(r"ctx\.call\(_lib\.GRAM_IQ,", src)
    assert (lib.GRAM_IQ_D, lib.GRAM_IQ) == ("tsdr_ctrack_gram_iq_d", "tsdr_ctrack_gram_iq")
    pkg = os.path.dirname(mod.__file__)
    for f in os.listdir(pkg):
        if f.endswith(".py") and f not in ("gram.py", "_lib.py"):
            text = open(os.path.join(pkg, f)).read()
            assert "GRAM_IQ" not in text and "tsdr_ctrack_gram" not in text, f
    import tempestsdr_jl_amd as T
    for name in list(want) + list(static):
        assert getattr(T, name) is getattr(mod, name), name


def test_every_entry_point_is_called_by_the_gpu_suite():
    text = open(os.path.join(ROOT, "tests", "test_gram_gpu.py")).read()
    called = DH.called_symbols(text)
    assert set(SYMS) <= called, sorted(set(SYMS) - called)
    assert "import dptr_util as D" in text and "D.Arenas(" in text and "pytestmark = pytest.mark.gpu" in text
    assert "from test_cstack_gpu import" in text and "from test_ctrack_gpu import" in text and "CASES" in text
    for name in ("ctrack_gram(", "ctrack_gram_d(", "blind_track(", "coherent_period_scan("):
        assert "ctx." + name in text, name


def test_kernel_source_keeps_its_launch_rules():
    src = open(os.path.join(CSRC, "raster_gram.hip")).read()
    code = re.sub(r"//.*", "", src)
    for name in ("gram_tile", "gram_direct", "gram_sum"):
        assert f'TSDR_LAUNCH(ctx, "{name}"' in code, name
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32(" in code
    assert "hipLaunchKernelGGL" not in code and not re.search(r"\batomic\w*\(", code) and not re.search(r"\basm\b", code)
    assert len(re.findall(r"\bHostStage \w+\(ctx\)", code)) == 1 and not re.search(r"scratch\(WS_(IN|OUT|AUX)\b", code)
    for helper in ("fold_check<Gram>(", "fold_launch<Gram>(", "frame_pos(", "fold_s(", "fold_tap(", "coh_blend(", "coh_mul(", "ld_iq(",
                   "track_weight(", "lds_opt_in(", "scratch(WS_GRAM"):
        assert helper in code, helper
    assert "k_fold_engine" not in code, "the kernel has a body of its own"
    assert "WS_GRAM" in open(os.path.join(CSRC, "common.h")).read()
    build = open(os.path.join(ROOT, "tempestsdr.jl_amd", "build.py")).read()
    assert '"raster_gram.hip": ["raster_ctrack.hip", "raster_cstack.hip"]' in build and '"tempest_hip_gram.h"' in build


def test_refusals_need_no_device():
    """a NULL context is refused before anything else; nothing is dereferenced"""
    lib = HH._pkg("_lib").load()
    z, gram, track = np.zeros(16, np.complex64), np.zeros(2), np.zeros(2)
    args = (None, z.ctypes.data, 0, 1.0, 16, 0.0, 8.0, track.ctypes.data, 1, 2, 2, gram.ctypes.data)
    assert lib.tsdr_ctrack_gram_iq(*args) == -1 and lib.tsdr_ctrack_gram_iq_d(*args) == -1
    assert not gram.any()


# ---------------------------------------------------------------- the host algorithms on answers known without them
def _both(name):
    return getattr(GR, name), getattr(HH._pkg("gram"), name)


@functools.lru_cache(maxsize=None)
def clean_gram():
    """(z, G) of the drift-free capability capture, no track, 24 frames"""
    z = CF.samples(TH.drift_captures()[0])
    G = GR.gram(z, TH.CAP["t0"], TH.CAP["T"], None, TH.DRIFT["frames"], TH.CAP["y"], TH.CAP["x"])
    G.setflags(write=False)
    return z, G


def test_gram_energy_is_the_folds_energy():
    """(1/F^2) sum_fg w_f conj(w_g) G[f][g] at a_f = f kappa is sum |Z|^2 of cstack_ref.zmean, at three kappa, to 1e-11"""
    z, G = clean_gram()
    y, x, T, t0, F = TH.CAP["y"], TH.CAP["x"], TH.CAP["T"], TH.CAP["t0"], TH.DRIFT["frames"]
    f = np.arange(F, dtype=np.float64)
    for kappa in (TH.KAPPA_TRUE, 0.25, -1.3):
        want = float(np.sum(np.abs(CS.zmean(z, t0, T, kappa, 0.0, F, y, x)) ** 2))
        for fn in _both("gram_energy"):
            assert abs(fn(G, f * kappa) - want) <= 1e-11 * want, (kappa, fn(G, f * kappa), want)
        assert abs(GR.periodogram(G, kappa) - want) <= 1e-11 * want
    assert np.allclose(HH._pkg("gram").lag_sums(G)[3], sum(G[g + 3][g] for g in range(F - 3)), rtol=1e-13, atol=0)


def test_gram_carrier_finds_the_ladders_kappa():
    """on the drift-free capture gram_carrier is within the ladder's last step of cfold_ref.ladder's kappa, its energy is the
    periodogram's there, and no grid point of the reference's dense search is better by more than 1e-9"""
    z, G = clean_gram()
    y, x, T, t0, F = TH.CAP["y"], TH.CAP["x"], TH.CAP["T"], TH.CAP["t0"], TH.DRIFT["frames"]
    kappa_l, last, _ = CF.ladder(z, t0, T, F, y, x)
    k_ref, e_ref = GR.gram_carrier(G)
    k, e = HH._pkg("gram").gram_carrier(G)
    print(f"ladder {kappa_l:.6f} (last step {last:.6f}); gram_carrier {k:.6f}, dense reference {k_ref:.6f}; energy {e:.6g}")
    assert abs(k - kappa_l) <= last and abs(k_ref - kappa_l) <= last
    assert abs(e - GR.periodogram(G, k)) <= 1e-12 * e and e >= e_ref * (1.0 - 1e-9)
    assert abs(k - TH.KAPPA_TRUE) <= 1e-3
    one = np.array([[2.5 + 0j]])
    assert HH._pkg("gram").gram_carrier(one) == (0.0, 2.5)


def test_gram_phases_recovers_planted_phases():
    """G = A u u^H + noise with |u_f| = 1: v is u turned so that v_0 = 1, within the noise; rho = G0 v; F == 1 gives v = [1]"""
    rng = np.random.default_rng(11)
    F = 24
    u = np.exp(2j * np.pi * rng.uniform(size=F))
    N = rng.normal(size=(F, F)) + 1j * rng.normal(size=(F, F))
    G = 10.0 * np.outer(u, u.conj()) + 0.1 * (N + N.conj().T) + np.diag(rng.uniform(5, 50, F))
    want = u * np.conj(u[0])
    for fn in _both("gram_phases"):
        v, rho = fn(G)
        assert np.max(np.abs(np.abs(v) - 1.0)) <= 1e-12 and abs(v[0] - 1.0) <= 1e-12
        assert np.max(np.abs(v - want)) <= 0.05, np.max(np.abs(v - want))
        G0 = G - np.diag(np.diag(G))
        assert np.max(np.abs(rho - G0 @ v)) <= 1e-9
        assert np.max(np.abs(np.angle(rho * np.conj(v)))) <= 1e-9, "a fixed point: rho_f has the phase of v_f"
        v1, rho1 = fn(np.array([[3.0 + 0j]]))
        assert v1.tolist() == [1.0] and rho1.tolist() == [0.0]
    a, b = GR.gram_phases(G)[0], HH._pkg("gram").gram_phases(G)[0]
    assert np.max(np.abs(a - b)) <= 1e-9, "the bindings' phases are the reference's"
    # an entry without any coupling keeps unit modulus
    G2 = G.copy()
    G2[5, :] = G2[:, 5] = 0.0
    for fn in _both("gram_phases"):
        assert abs(abs(fn(G2)[0][5]) - 1.0) <= 1e-12
    for fn in _both("gram_track"):
        t = fn(G, np.full((F, 2), 0.25))
        assert np.max(np.abs(t[:, 0] - 0.25 - np.angle(GR.gram_phases(G)[0]) / (2 * np.pi))) <= 1e-9 and np.all(t[:, 1] == 0.25)


def test_track_slopes_recovers_planted_slopes_across_a_wrap():
    """mid-frame phases q(f + 1/2) of a quadratic that runs over several turns, given modulo 1: b_f is q'(f + 1/2) to the second
    difference's size, exactly so in the interior, and a_f + b_f / 2 is the given phase"""
    F = 24
    f = np.arange(F, dtype=np.float64)
    q = np.poly1d([0.03, 0.77, 0.1])
    mid = q(f + 0.5)
    assert mid[-1] - mid[0] > 30.0
    given = np.stack([mid % 1.0 - 0.5, np.full(F, 9.0)], axis=1)
    for fn in _both("track_slopes"):
        t = fn(given)
        want = q.deriv()(f + 0.5)
        k = round(t[0, 1] - want[0])
        assert k == -1, "d_0 = 0.83 turns per frame is taken into [-1/2, 1/2): -0.17"
        assert np.max(np.abs(t[1:-1, 1] - (want[1:-1] + k))) <= 1e-9
        assert abs(t[0, 1] - (want[0] + k)) <= 0.0301 and abs(t[-1, 1] - (want[-1] + k)) <= 0.0301
        assert np.max(np.abs(t[:, 0] + 0.5 * t[:, 1] - given[:, 0])) <= 1e-12
        assert fn(np.array([[0.3, 5.0]])).tolist() == [[0.3, 0.0]]
    assert np.max(np.abs(GR.track_slopes(given) - HH._pkg("gram").track_slopes(given))) <= 1e-12


# ---------------------------------------------------------------- the capabilities, on the CPU reference
RAMP = dict(frames=24, chi=0.06)
WALK = dict(frames=24, seed=7, sigma=0.12, steps=40)
SCAN = dict(step=2.0, count=9)


@functools.lru_cache(maxsize=None)
def hard_captures():
    """the drift-free capture of tests/test_ctrack_host.py multiplied by (a ramp of 0.06 turns/frame per frame, a random walk of the
    carrier phase: default_rng(7), steps = cumsum(normal(0, 0.12, 40)), interpolated linearly at k / T)"""
    iq = TH.drift_captures()[0]
    t = np.arange(iq.size, dtype=np.float64) / TH.CAP["T"]
    steps = np.cumsum(np.random.default_rng(WALK["seed"]).normal(0.0, WALK["sigma"], WALK["steps"]))
    ramp = (iq.astype(np.complex128) * np.exp(2j * np.pi * 0.5 * RAMP["chi"] * t * t)).astype(np.complex64)
    walk = (iq.astype(np.complex128) * np.exp(2j * np.pi * np.interp(t, np.arange(WALK["steps"]), steps))).astype(np.complex64)
    for a in (ramp, walk):
        a.setflags(write=False)
    return ramp, walk


@functools.lru_cache(maxsize=None)
def hard_reference(which):
    """(ladder + refine_track after two passes, blind_track with two passes): correlations with the card, from the references alone"""
    y, x, T, t0, F = TH.CAP["y"], TH.CAP["x"], TH.CAP["T"], TH.CAP["t0"], RAMP["frames"]
    z = CF.samples(hard_captures()[which])
    card = TH.cap_card()
    kappa = CF.ladder(z, t0, T, F, y, x)[0]
    _, Z = R.refine_track(z, t0, T, F, y, x, kappa, 2, 2)
    _, _, Zb = GR.blind_track(z, t0, T, F, y, x, 2)
    return TH.corr(np.abs(Z[-1]), card), TH.corr(np.abs(Zb), card)


@functools.lru_cache(maxsize=None)
def scan_periods():
    return tuple(TH.CAP["T"] + (k - SCAN["count"] // 2) * SCAN["step"] for k in range(SCAN["count"]))


@functools.lru_cache(maxsize=None)
def scan_reference():
    """gram_ref.period_scan over the 9 periods around 9150.37 on the drift-free capture"""
    return GR.period_scan(CF.samples(TH.drift_captures()[0]), TH.CAP["t0"], TH.CAP["y"], TH.CAP["x"], scan_periods())


def test_capability_a_ramp_no_constant_kappa_follows():
    """66 x 160, T 9150.37, t0 3.25, -10 dB, 24 frames, a ramp of 0.06 turns/frame per frame: the ladder's constant kappa folds to
    noise and refine_track never locks (0.133 after two passes; the capture without drift gives 0.555); the blind track from the Gram
    matrix, two passes, gives 0.554"""
    tracked, blind = hard_reference(0)
    print(f"ramp 0.06: ladder + refine_track 0.133 -> {tracked:.3f}; blind track 0.554 -> {blind:.3f}")
    assert abs(tracked - 0.133) <= 0.002 and abs(blind - 0.554) <= 0.002
    assert tracked <= 0.20 and blind >= 0.52


def test_capability_a_carrier_on_a_random_walk():
    """the same capture with the carrier phase on a random walk of 0.12 turns per frame: ladder + refine_track reaches 0.475, the blind
    track 0.554"""
    tracked, blind = hard_reference(1)
    print(f"random walk: ladder + refine_track 0.475 -> {tracked:.3f}; blind track 0.554 -> {blind:.3f}")
    assert abs(tracked - 0.475) <= 0.002 and abs(blind - 0.554) <= 0.002
    assert tracked <= 0.50 and blind >= 0.52


def test_period_scan_reference_has_a_clear_maximum():
    """9 periods 2 samples apart around 9150.37 on the drift-free capture: the true period wins, and the runner-up's energy is 0.882
    of the maximum (the noise's own energy, which every trial folds, is most of that floor)"""
    e, kappas, best = scan_reference()
    s = np.sort(e)
    print(f"period scan: best {best}, runner-up / maximum {s[-2] / s[-1]:.3f}, kappa there {kappas[best]:.4f}")
    assert best == SCAN["count"] // 2 and abs(s[-2] / s[-1] - 0.882) <= 0.002
    assert abs(kappas[best] - TH.KAPPA_TRUE) <= 1e-3
