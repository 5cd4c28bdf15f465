"""Host-side checks of coherent stacking across buffers (no GPU): include/tempest_hip_cstack.h, its ctypes table (_lib._SIGS_CSTACK),
its Python module (cstack.py) and its Julia shim (julia/TempestHIP_cstack.jl) agree with each other and with the library, the way
test_cfold_host.py pins tempest_hip_cfold.h; the launch rules of csrc/raster_cstack.hip; and the numpy reference the GPU tests compare
against (tests/cstack_ref.py) on answers known without it."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np

import cfold_ref as CR
import cstack_ref as R
import test_dptr_host as DH
import test_hires_host as HH
import test_julia_shim_static as JS

ROOT = HH.ROOT
MAIN_H = HH.MAIN_H
CSTACK_H = os.path.join(ROOT, "include", "tempest_hip_cstack.h")
CFOLD_H = os.path.join(ROOT, "include", "tempest_hip_cfold.h")
CSTACK_SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP_cstack.jl")
CSRC = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc")
KERNEL = os.path.join(CSRC, "raster_cstack.hip")
ENGINE = os.path.join(CSRC, "fold_engine.h")
OPS = os.path.join(CSRC, "coherent_ops.h")

SYMS = ["tsdr_cstack_iq", "tsdr_cstack_iq_d"]
PROTO = ["tsdr_ctx *ctx", "const void *iq", "int iq_fmt", "float scale", "size_t n", "double t0", "double T", "double kappa", "double phi",
         "int n_frames", "int y_t", "int x_t", "float alpha", "int mode", "float *zstate", "float *mag", "double *info"]


# ---------------------------------------------------------------- header, table, library, shims
def test_header_declares_the_two_forms_and_the_constants():
    p = HH._protos(CSTACK_H)
    assert sorted(p) == SYMS
    assert p["tsdr_cstack_iq"] == p["tsdr_cstack_iq_d"] == PROTO
    text = open(CSTACK_H).read()
    for name, value in (("TSDR_CSTACK_GIVEN", 0), ("TSDR_CSTACK_LOCK", 1), ("TSDR_CSTACK_INFO", 8)):
        assert re.search(rf"^#define {name} {value}$", text, flags=re.M), name
    lib = HH._pkg("_lib")
    assert (lib.CSTACK_GIVEN, lib.CSTACK_LOCK, lib.CSTACK_INFO) == (0, 1, 8) == (R.GIVEN, R.LOCK, 8)
    for s in SYMS:
        assert not s.startswith("tsdr_fold") and not s.startswith("tsdr_cfold")


def test_main_header_includes_it_once_after_the_cfold_header():
    main = open(MAIN_H).read()
    assert main.count('#include "tempest_hip_cstack.h"') == 1
    assert main.index('#include "tempest_hip_cstack.h"') > main.index('#include "tempest_hip_cfold.h"')
    for path in (MAIN_H, CFOLD_H, os.path.join(ROOT, "include", "tempest_hip_fold.h")):
        assert not re.search(r"tsdr_cstack|TSDR_CSTACK_", HH._strip(path)), path
    guard = open(CSTACK_H).read()
    assert "#ifndef TEMPEST_HIP_CSTACK_H" in guard and "#ifndef TEMPEST_HIP_CFOLD_H\n#error" in guard


def test_header_states_the_contract():
    src = " ".join(open(CSTACK_H).read().split())
    for phrase in ("INPUT", "SAMPLING", "WEIGHT", "RESULT", "LOCK", "INFO", "ACCURACY", "REPRODUCIBILITY", "FORMAT INVARIANCE", "REFUSALS",
                   "COST", "the complex state exists", "pair index p*y_t + l", "the state is NOT READ", "iq is never written",
                   "x = fl64(f * kappa)", "x' = fl64(x + phi)", "r_f = x' - floor(x')", "w_f = (f32(cospi(2 r_f)), f32(-sinpi(2 r_f)))",
                   "Only frac(phi) matters", "have the bits of tsdr_cfold_iq_d", "rho = sum_m Z(m) * conj(S(m))",
                   "Re += zr*sr + zi*si, Im += zi*sr - zr*si", "rho = E_s = 0", "re = fadd(fmul(qr, zr), fmul(qi, zi))",
                   "im = fsub(fmul(qr, zi), fmul(qi, zr))", "fadd(fmul(alpha, S), fmul(fsub(1, alpha), Zq))", "No float atomics",
                   "hypot(Re rho, Im rho) is finite and > 0", "otherwise q = (1, 0)", "theta = atan2(Im rho, Re rho) / (2 pi)",
                   "gamma = |rho| / sqrt(E_z * E_s)", "Written in GIVEN mode too", "does not depend on tsdr_set_precision",
                   "|S' - ref| <= sqrt(2) * (F + 16) * u * M = eps_s", "|mag - |ref|| <= sqrt(2) * (F + 18) * u * M",
                   "|rho - ref| <= eps_z * sqrt(P * E_s) + 2^-36 * sqrt(E_z * E_s) = eps_rho",
                   "|E_z - ref| <= 2 * eps_z * sqrt(P * ref) + P * eps_z^2 + 2^-36 * ref",
                   "|theta - ref| <= eps_rho / (4 * |rho_ref|) + 2^-40 turns",
                   "|S' - ref| <= sqrt(2) * (F + 19) * u * M + (pi/2) * amax * eps_rho / |rho_ref| = eps_lock",
                   "a function of |rho_ref|, not a constant", "identical bits in zstate, mag and info", "host-expanded ComplexF32",
                   "nothing written and nothing enqueued", "phi not finite", "mode outside {0, 1}", "zstate NULL",
                   "zstate not 8-byte aligned, mag not 4-byte aligned, info not 8-byte aligned", "mag and info may be NULL",
                   "F == 0 (with everything else valid) is TSDR_OK and touches nothing, info included",
                   "zstate[0 .. 2P), mag[0 .. P), info[0 .. 8)", "Overlapping outputs are undefined", "512-byte segments",
                   '"cstack_tile"', '"cstack_direct"', '"cstack_lock"', '"cstack_blend"', "TSDR_CFOLD_STAGE_MAX", '"wait_ms"'):
        assert phrase in src, phrase
    # the cfold header keeps saying what it said; this header is where the complex state is announced
    assert "a complex state across buffers is out of scope" in " ".join(open(CFOLD_H).read().split())


def test_header_table_and_library_agree():
    lib = HH._pkg("_lib")
    assert sorted(HH._protos(CSTACK_H)) == SYMS == lib.exported_names_cstack()
    for other in (lib._SIGS, lib._SIGS_IQ, lib._SIGS_CPLX, lib._SIGS_HIRES, lib._SIGS_REGISTER, lib._SIGS_DISPLAY, lib._SIGS_FOLD,
                  lib._SIGS_CFOLD):
        assert not set(other) & set(lib._SIGS_CSTACK)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    for sym in SYMS:
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_cstack.h but not exported"
        assert getattr(bound, sym).restype is C.c_int and getattr(bound, sym).argtypes == lib._SIGS_CSTACK[sym][1], sym


def test_table_argtypes_match_the_prototypes():
    lib = HH._pkg("_lib")
    ct = {"i32": C.c_int, "i64": C.c_size_t, "f32": C.c_float, "f64": C.c_double}
    for sym, params in HH._protos(CSTACK_H).items():
        res, args = lib._SIGS_CSTACK[sym]
        assert res is C.c_int and len(args) == len(params), sym
        for k, (a, p) in enumerate(zip(args, params)):
            cls = JS.c_class(p)
            assert (a is C.c_void_p) if cls == "ptr" else (a is ct[cls]), (sym, k, p, a)


def test_every_ccall_of_the_cstack_shim_matches_its_prototype():
    protos = {name: ("i32", [JS.c_class(p) for p in params]) for name, params in HH._protos(CSTACK_H).items()}
    assert sorted(protos) == SYMS and not set(protos) & set(JS.header_protos())
    jl = open(CSTACK_SHIM).read()
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
        name = m.group(1)
        seen.append(name)
        cret, cparams = protos[name]
        assert (ret, types, len(parts) - 3) == (cret, cparams, len(cparams)), (name, ret, types, cret, cparams)
    assert sorted(seen) == SYMS, "one ccall per symbol"


def test_shim_is_included_after_the_cfold_shim_and_the_main_shim_names_nothing():
    main = open(HH.SHIM).read()
    assert main.count('include("TempestHIP_cstack.jl")') == 1
    assert main.index('include("TempestHIP_cstack.jl")') > main.index('include("TempestHIP_cfold.jl")')
    assert main.rstrip().endswith("end # module") and main.index('include("TempestHIP_cstack.jl")') > main.rindex("\nfunction ")
    code = "\n".join(line for line in main.splitlines() if not line.lstrip().startswith("#"))
    assert "tsdr_cstack" not in code and "cstack_plan" not in code
    jl = open(CSTACK_SHIM).read()
    for sig in (r"\nfunction hip_cstack!\(zstate::Matrix\{ComplexF32\}, iq::Vector\{ComplexF32\}, t0::Real, T::Real, κ::Real, φ::Real, F::Integer;",
                r"\nfunction hip_cstack_d!\(d_zstate::Ptr\{Cvoid\}, d_iq::Ptr\{Cvoid\}, fmt::Symbol,",
                r"\nfunction cstack_plan\(n::Integer, t0::Real, T::Real, κ::Real, φ::Real; θ::Real = 0.0\)"):
        assert re.search(sig, jl), sig
    tests = open(os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "runtests.jl")).read()
    assert "hip_cstack!(" in tests and "cstack_plan(" in tests


def test_python_interface_and_delegation():
    api, mod = HH._pkg("api"), HH._pkg("cstack")
    p = inspect.signature(api.Context.cstack_d).parameters
    want = ["iq", "fmt", "scale", "n", "t0", "T", "kappa", "phi", "n_frames", "y_t", "x_t", "alpha", "mode", "zstate", "mag", "info"]
    assert list(p) == ["self"] + want and p["mag"].default is None and p["info"].default is None
    assert list(inspect.signature(mod.cstack_d).parameters) == ["ctx"] + want
    assert list(inspect.signature(api.Context.cstack).parameters)[:9] == ["self", "iq", "t0", "T", "kappa", "phi", "n_frames", "y_t", "x_t"]
    for fn in (api.Context.cstack_plan, mod.cstack_plan):
        p = inspect.signature(fn).parameters
        assert list(p) == ["n", "t0", "T", "kappa", "phi", "theta"] and p["theta"].default == 0.0
    called = DH.called_symbols(open(mod.__file__).read())
    assert set(SYMS) <= called
    assert not (DH.called_symbols(open(api.__file__).read()) & set(SYMS)), "api.py delegates; it calls neither symbol itself"
    import tempestsdr_jl_amd as T
    for name in ("cstack", "cstack_d", "cstack_plan"):
        assert getattr(T, name) is getattr(mod, name), name
    pkg = os.path.dirname(mod.__file__)
    for f in os.listdir(pkg):
        if f.endswith(".py") and f not in ("cstack.py", "_lib.py"):
            assert "tsdr_cstack" not in open(os.path.join(pkg, f)).read(), f
    assert mod.mode_code("given") == 0 and mod.mode_code("lock") == 1 and mod.mode_code(1) == 1
    for bad in ("open", 2, True, None):
        try:
            mod.mode_code(bad)
        except AssertionError:
            continue
        raise AssertionError(f"mode {bad!r} accepted")


def test_both_entry_points_are_called_by_the_gpu_suite():
    text = open(os.path.join(ROOT, "tests", "test_cstack_gpu.py")).read()
    called = DH.called_symbols(text)
    assert set(SYMS) <= called, sorted(set(SYMS) - called)
    assert 'ctx.call("tsdr_cstack_iq_d"' in text
    assert "import dptr_util as D" in text and "D.Arenas(" in text and "pytestmark = pytest.mark.gpu" in text


def test_kernel_source_keeps_its_launch_rules():
    src = open(KERNEL).read()
    code = re.sub(r"//.*", "", src)
    for name in ("cstack_tile", "cstack_direct", "cstack_lock", "cstack_blend"):
        assert f'TSDR_LAUNCH(ctx, "{name}"' in src, name
    assert '#include "fold_engine.h"' in code and '#include "coherent_ops.h"' in code
    assert re.search(r'"cstack_tile", \(k_fold_engine<Stacked, kFoldTileP, kFoldTileWaves, 1, true, false>\)', code)
    assert re.search(r'"cstack_direct", \(k_fold_engine<Stacked, kFoldDirectP, kFoldDirectWaves, 1, false, false>\)', code)
    assert "stream_grid(" not in code and "stream_blocks(" not in code and "ceil_div(" in code, "exact grids"
    assert "hipLaunchKernelGGL" not in code, "every launch goes through TSDR_LAUNCH"
    assert not re.search(r"\batomic\w*\(", code), "no atomics at all: partial sums are combined in a fixed order"
    assert not re.search(r"\basm\b", code), "no inline assembly"
    assert "static_assert(" in code and "TSDR_CFOLD_STAGE_MAX" in code and "WS_CSTACK" in code
    assert "kStageMax = TSDR_CFOLD_STAGE_MAX" in code, "the staged / direct choice is the coherent fold's"
    # the engine's third epilogue is a compile-time branch on the flavour, and both coherent flavours share their arithmetic
    engine = open(ENGINE).read()
    assert "if constexpr (!SCAN && !Fl::stacks)" in engine and "Fl::stack(A, st[0]," in engine
    for f in ("raster_fold.hip", "raster_cfold.hip"):
        assert "stacks = false" in open(os.path.join(CSRC, f)).read(), f
    assert "stacks = true" in code
    ops = open(OPS).read()
    for fn in ("coh_weight(", "coh_blend(", "coh_add(", "coh_mean("):
        assert fn in ops and fn in code and fn in open(os.path.join(CSRC, "raster_cfold.hip")).read(), fn


def test_workspace_and_build_know_the_feature():
    common = open(os.path.join(CSRC, "common.h")).read()
    slots = re.search(r"enum Slot \{(.*?)\}", common, flags=re.S).group(1)
    names = re.findall(r"^\s*(WS_\w+)", slots, flags=re.M)
    assert names.index("WS_CSTACK") == names.index("WS_CFOLD") + 1, "directly after WS_CFOLD"
    build = open(os.path.join(ROOT, "tempestsdr.jl_amd", "build.py")).read()
    assert '"tempest_hip_cstack.h"' in build and '"tempest_hip_cfold.h"' in build
    assert os.path.exists(KERNEL), "picked up by build.py's directory scan"


def test_refusals_need_no_device():
    """a NULL context is refused before anything else; nothing is dereferenced"""
    lib = HH._pkg("_lib").load()
    z = np.zeros(16, np.complex64)
    zs, mag, info = np.zeros(8, np.float32), np.zeros(4, np.float32), np.zeros(8, np.float64)
    args = (None, z.ctypes.data, 0, 1.0, 16, 0.0, 8.0, 0.25, 0.1, 1, 2, 2, 0.0, 1, zs.ctypes.data, mag.ctypes.data, info.ctypes.data)
    assert lib.tsdr_cstack_iq(*args) == -1 and lib.tsdr_cstack_iq_d(*args) == -1
    assert not zs.any() and not mag.any() and not info.any()


# ---------------------------------------------------------------- the reference's own known answers
GEOMS = ((0.0, 1000.0, 5, 10, 30), (3.25, 701.3, 7, 9, 14), (0.0, 40.5, 12, 4, 4))


def test_constant_sample_against_a_turned_state():
    """z = z0, kappa = 0, S = c z0: rho = P z0 conj(c z0), theta = -arg(c) / 2 pi, gamma = 1; in LOCK mode S' has the phase of S"""
    z0, c = 0.3 - 0.4j, 0.8 * complex(math.cos(1.1), math.sin(1.1))
    z = np.full(5000, z0, np.complex128)
    for t0, T, F, y, x in GEOMS:
        P = y * x
        S = np.full(P, c * z0)
        for mode in (R.GIVEN, R.LOCK):
            out, mag, info = R.cstack(z, t0, T, 0.0, 0.0, F, y, x, 0.25, mode, S)
            rho = P * z0 * np.conj(c * z0)
            assert abs(complex(info[0], info[1]) - rho) <= 1e-12 * abs(rho)
            assert abs(info[2] - P * 0.25) < 1e-12 and abs(info[3] - P * 0.25 * 0.64) < 1e-12
            assert R.turn_dist(info[4], -1.1 / (2.0 * math.pi)) < 1e-12 and abs(info[5] - 1.0) < 1e-12
            if mode == R.LOCK:
                assert abs(complex(info[6], info[7]) - np.conj(c) / abs(c)) < 1e-12
                assert np.allclose(out, (0.25 * 0.8 + 0.75) * (c / abs(c)) * z0, rtol=0, atol=1e-15), "the phase of S, exactly"
                assert np.allclose(np.angle(out / S), 0.0, rtol=0, atol=1e-14)
            else:
                assert (info[6], info[7]) == (1.0, 0.0)
                assert np.allclose(out, 0.25 * c * z0 + 0.75 * z0, rtol=0, atol=1e-15)
            assert np.allclose(mag, np.abs(out), rtol=0, atol=0)
        out, mag, info = R.cstack(z, t0, T, 0.0, 0.0, F, y, x, 0.0, R.LOCK, np.full(P, np.nan))
        assert np.allclose(out, z0, rtol=0, atol=1e-15) and info[0] == info[1] == info[3] == info[4] == info[5] == 0.0
        assert (info[6], info[7]) == (1.0, 0.0), "alpha == 0: the state is not read, rho = E_s = 0, q = (1, 0)"


def test_pure_tone_over_two_buffers_keeps_its_amplitude_with_the_planned_phase():
    """z[k] = A exp(2 pi i nu k) over two buffers, kappa = nu T: with cstack_plan's carried t0 and phi both buffers fold pixel m to
    A exp(i psi(m)) g, g a mean of chord points turned back onto the arc: |g - 1| <= 1 - cos(pi nu), the chord's sagitta.  So GIVEN at
    alpha = 0.5 keeps |S'| >= A cos(pi nu); with the phase off by half a turn S' = (S - Z) / 2 and |S'| <= A (1 - cos(pi nu))"""
    A, nu = 0.75, 0.0137
    T, y, x = 1207.73, 11, 23
    P, n1, n2 = y * x, 6200, 5000
    kappa = nu * T
    z = A * np.exp(2j * np.pi * nu * np.arange(n1 + n2))
    phi0 = -nu * 5.5          # so that the first frame (t0 = 5.5) folds to a real positive picture: any value would do
    F1, t1, phi1 = R.cstack_plan(n1, 5.5, T, kappa, phi0)
    F2, _, _ = R.cstack_plan(n2, t1, T, kappa, phi1)
    assert (F1, F2) == (5, 3)
    S1, _, _ = R.cstack(z[:n1], 5.5, T, kappa, phi0, F1, y, x)
    S2, mag, info = R.cstack(z[n1:], t1, T, kappa, phi1, F2, y, x, 0.5, R.GIVEN, S1)
    lo = A * math.cos(math.pi * nu) - 1e-9
    assert np.all(np.abs(S1) >= lo) and np.all(np.abs(S1) <= A)
    assert np.all(mag >= lo) and np.all(mag <= A), (float(mag.min()), lo)
    assert R.turn_dist(info[4], 0.0) < 1e-3 and info[5] > 0.9999, "the planned phase leaves no residual"
    _, mag_off, info_off = R.cstack(z[n1:], t1, T, kappa, phi1 + 0.5, F2, y, x, 0.5, R.GIVEN, S1)
    assert R.turn_dist(info_off[4], 0.5) < 1e-3
    assert np.all(mag_off <= A * (1.0 - math.cos(math.pi * nu)) + 1e-9), float(mag_off.max())
    # LOCK undoes the half turn
    _, mag_lock, _ = R.cstack(z[n1:], t1, T, kappa, phi1 + 0.5, F2, y, x, 0.5, R.LOCK, S1)
    assert np.all(mag_lock >= lo)


def test_phi_and_phi_plus_one_agree():
    rng = np.random.default_rng(5)
    z = (rng.normal(size=5000) + 1j * rng.normal(size=5000)).astype(np.complex64)
    for t0, T, F, y, x in GEOMS:
        a = R.zmean(CR.samples(z), t0, T, 0.3, 0.37, F, y, x)
        b = R.zmean(CR.samples(z), t0, T, 0.3, 1.37, F, y, x)
        c = R.zmean(CR.samples(z), t0, T, 0.3, -2.63, F, y, x)
        assert np.max(np.abs(a - b)) <= 1e-14 * 5 and np.max(np.abs(a - c)) <= 1e-14 * 5
        # and the factor is the weight's: frame by frame
        w = (np.arange(y * x) + 0.5) * (T / (y * x)) - 0.5
        acc = np.zeros(y * x, np.complex128)
        zz = CR.samples(z)
        for f in range(F):
            u = np.clip((t0 + f * T) + w, 0.0, zz.size - 1.0)
            k = np.minimum(np.floor(u), zz.size - 2.0).astype(np.int64)
            acc += R.weight(f, 0.3, 0.37) * (zz[k] + (u - k) * (zz[k + 1] - zz[k]))
        assert np.max(np.abs(R.to_state(acc / F, y, x) - a)) <= 1e-13


def test_cstack_plan_by_hand_and_past_the_buffer():
    mod = HH._pkg("cstack")
    for plan in (R.cstack_plan, mod.cstack_plan):
        # 600 samples, T = 40.5: frames start at 0, 40.5, ..., 567 (14 whole ones); the 15th straddles; 15 * 40.5 - 600 = 7.5
        assert plan(600, 0.0, 40.5, 0.125, 0.5) == (14, 7.5, 0.375)            # frac(0.5 + 15 / 8) = 0.375
        assert plan(600, 0.0, 40.5, 0.125, 0.5, 0.25) == (14, 7.5, 0.625)      # a measured residual joins the carried phase
        assert plan(600, 7.5, 40.5, -0.25, 0.0) == (14, 15.0, 0.25)            # frac(-15 / 4) = 0.25
        assert plan(100, 130.0, 40.5, 0.125, 0.7) == (0, 30.0, 0.7)            # no frame starts here: the phase is kept
        F, t1, p1 = plan(600, 0.0, 40.5, 0.3, 0.0)
        assert 0.0 <= p1 < 1.0 and 0.0 < t1 <= 40.5
    assert R.fold_plan(600, 0.0, 40.5) == HH._pkg("fold").fold_plan(600, 0.0, 40.5)


def test_bounds_helpers():
    u = 2.0 ** -24
    assert R.eps_s(4, 0.5) == math.sqrt(2.0) * 20 * u * 0.5 and R.eps_s(4, 0.5, 3.0) == math.sqrt(2.0) * 20 * u * 3.0
    assert R.eps_mag(4, 0.5) == math.sqrt(2.0) * 22 * u * 0.5
    assert CR.eps_z(7, 1.0) + 4 * math.sqrt(2.0) * u <= R.eps_s(7, 1.0), "eps_s covers eps_z and the blend's four roundings"
    e = R.eps_rho(5, 0.01, 1000, 2.0, 3.0)
    assert e == CR.eps_z(5, 0.01) * math.sqrt(3000.0) + 2.0 ** -36 * math.sqrt(6.0)
    assert R.eps_lock(5, 0.01, 0.02, e, 4.0) == math.sqrt(2.0) * 24 * u * 0.02 + 0.5 * math.pi * 0.01 * e / 4.0
    assert R.eps_lock(5, 0.01, 0.0, 0.0, 0.0) == math.sqrt(2.0) * 24 * u * 0.01, "rho_ref == 0: no angle term"
    assert abs(R.eps_lock_mag(5, 0.01, 0.02, e, 4.0) - R.eps_lock(5, 0.01, 0.02, e, 4.0) - math.sqrt(2.0) * 2 * u * 0.02) < 1e-20
    assert R.eps_theta(e, 4.0) == e / 16.0 + 2.0 ** -40
    assert R.turn_dist(0.99, 0.01) < 0.0200001 and R.turn_dist(-0.25, 0.75) == 0.0
