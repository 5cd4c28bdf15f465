"""Host-side checks of phase-coherent frame folding (no GPU): include/tempest_hip_cfold.h, its ctypes table (_lib._SIGS_CFOLD), its
Python module (cfold.py) and its Julia shim (julia/TempestHIP_cfold.jl) agree with each other and with the library, the way
test_fold_host.py pins tempest_hip_fold.h; the launch rules of csrc/raster_cfold.hip; the engine shared with
csrc/raster_fold.hip (csrc/fold_engine.h); and the numpy reference the GPU tests compare against (tests/cfold_ref.py) on answers known without it."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np

import cfold_ref as R
import fold_ref as FR
import test_dptr_host as DH
import test_hires_host as HH
import test_julia_shim_static as JS

ROOT = HH.ROOT
MAIN_H = HH.MAIN_H
CFOLD_H = os.path.join(ROOT, "include", "tempest_hip_cfold.h")
FOLD_H = os.path.join(ROOT, "include", "tempest_hip_fold.h")
CFOLD_SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP_cfold.jl")
CSRC = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc")
KERNEL = os.path.join(CSRC, "raster_cfold.hip")
ENGINE = os.path.join(CSRC, "fold_engine.h")   # the kernels and the host path, shared with raster_fold.hip

SYMS = ["tsdr_cfold_iq", "tsdr_cfold_iq_d", "tsdr_cfold_scan_iq", "tsdr_cfold_scan_iq_d"]
HEAD = ["tsdr_ctx *ctx", "const void *iq", "int iq_fmt", "float scale", "size_t n", "double t0", "double T"]
FOLD = HEAD + ["double kappa", "int n_frames", "int y_t", "int x_t", "float alpha", "float *state"]
SCAN = HEAD + ["double kappa0", "double dkappa", "int n_trials", "int n_frames", "int y_t", "int x_t", "double *score"]


# ---------------------------------------------------------------- header, table, library, shims
def test_header_declares_the_four_forms_and_the_constants():
    p = HH._protos(CFOLD_H)
    assert sorted(p) == SYMS
    assert p["tsdr_cfold_iq"] == p["tsdr_cfold_iq_d"] == FOLD
    assert p["tsdr_cfold_scan_iq_d"] == SCAN and p["tsdr_cfold_scan_iq"] == SCAN + ["int *best"]
    text = open(CFOLD_H).read()
    assert re.search(r"^#define TSDR_CFOLD_MAX_TRIALS 4096$", text, flags=re.M)
    assert re.search(r"^#define TSDR_CFOLD_STAGE_MAX 120$", text, flags=re.M)
    lib = HH._pkg("_lib")
    assert (lib.CFOLD_MAX_TRIALS, lib.CFOLD_STAGE_MAX) == (4096, 120)
    kernel = open(KERNEL).read()
    assert "TSDR_CFOLD_STAGE_MAX" in kernel and "TSDR_CFOLD_MAX_TRIALS" in kernel, "the kernel file builds with the header's constants"


def test_main_header_includes_it_once_after_the_fold_header():
    main = open(MAIN_H).read()
    assert main.count('#include "tempest_hip_cfold.h"') == 1
    assert main.index('#include "tempest_hip_cfold.h"') > main.index('#include "tempest_hip_fold.h"')
    for path in (MAIN_H, FOLD_H, HH.HIRES_H, os.path.join(ROOT, "include", "tempest_hip_display.h")):
        assert not re.search(r"tsdr_cfold|TSDR_CFOLD_", HH._strip(path)), path
    guard = open(CFOLD_H).read()
    assert "#ifndef TEMPEST_HIP_CFOLD_H" in guard and "#ifndef TEMPEST_HIP_FOLD_H\n#error" in guard


def test_header_states_the_contract():
    src = " ".join(open(CFOLD_H).read().split())
    for phrase in ("INPUT", "SAMPLING", "WEIGHT", "RESULT", "ACCURACY", "REPRODUCIBILITY", "FORMAT INVARIANCE", "SCORE", "REFUSALS", "COST",
                   "not its magnitude", "amax = max_k |z[k]|", "u_f(m) = (t0 + f*T) + ((m + 1/2)*(T/P) - 1/2)", "k = min(floor(u), n-2)",
                   "d may be 1", "z_f(m) = z[k] + d*(z[k+1] - z[k])", "2^-26 samples", "x = fl64(f * kappa)", "r_f = x - floor(x)",
                   "w_f = (f32(cospi(2 r_f)), f32(-sinpi(2 r_f)))", "rounded once", "Only frac(kappa) matters", "negative ones included",
                   "Z(m) = (1/F) * sum_f w_f * z_f(m)", "accumulated in complex f32", "c(m) = |Z(m)| as f32", "state[p*y_t + l]",
                   "the state is NOT READ", "averaged, non-coherently", "a complex state across buffers is out of scope",
                   "the envelope fold of the same data within the two bounds", "does not depend on tsdr_set_precision",
                   "|Z - Zref| <= sqrt(2) * (F + 12) * u * amax = eps_z",
                   "|state - ref| <= 1.5 * (F + 16) * u * max(amax, max|state_in|) = eps_c", "no floating-point atomics",
                   "host-expanded ComplexF32", "kappa_k = fl64(kappa0 + k*dkappa) at the one period T",
                   "score_k = sum_m ((double)Re Z_k(m))^2 + ((double)Im Z_k(m))^2", "No square root is taken and no raster is written",
                   "2*eps_z*sqrt(P*ref) + P*eps_z^2", "a NaN never wins", "nothing written and nothing enqueued", "P >= 2^31", "n >= 2^31",
                   "kappa, kappa0 or dkappa not finite", "t0 + F*T > n, evaluated in f64 at the one T", "alpha outside [0, 1] or NaN",
                   "n_trials < 1 or > TSDR_CFOLD_MAX_TRIALS", "16-byte aligned",
                   "F == 0 (with everything else valid) is TSDR_OK and touches nothing", "iq is never written", "8n + 8P",
                   "W = ceil(128*T/P) + 3", "TSDR_CFOLD_STAGE_MAX = 120", "ceil(K/8) times", '"cfold_tile"', '"cfold_direct"',
                   '"cfold_scan_tile"', '"cfold_scan_direct"', '"cfold_score"', '"wait_ms"'):
        assert phrase in src, phrase


def test_header_table_and_library_agree():
    lib = HH._pkg("_lib")
    assert sorted(HH._protos(CFOLD_H)) == SYMS == lib.exported_names_cfold()
    for other in (lib._SIGS, lib._SIGS_IQ, lib._SIGS_CPLX, lib._SIGS_HIRES, lib._SIGS_REGISTER, lib._SIGS_DISPLAY, lib._SIGS_FOLD):
        assert not set(other) & set(lib._SIGS_CFOLD)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    for sym in SYMS:
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_cfold.h but not exported"
        assert getattr(bound, sym).restype is C.c_int and getattr(bound, sym).argtypes == lib._SIGS_CFOLD[sym][1], sym


def test_table_argtypes_match_the_prototypes():
    lib = HH._pkg("_lib")
    ct = {"i32": C.c_int, "i64": C.c_size_t, "f32": C.c_float, "f64": C.c_double}
    for sym, params in HH._protos(CFOLD_H).items():
        res, args = lib._SIGS_CFOLD[sym]
        assert res is C.c_int and len(args) == len(params), sym
        for k, (a, p) in enumerate(zip(args, params)):
            cls = JS.c_class(p)
            assert (a is C.c_void_p) if cls == "ptr" else (a is ct[cls]), (sym, k, p, a)


def test_every_ccall_of_the_cfold_shim_matches_its_prototype():
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(tsdr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", HH._strip(CFOLD_H), flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        protos[name] = ("ptr" if "*" in ret else JS.c_class(ret + " x"), [JS.c_class(p) for p in JS.split_args(args)])
    assert sorted(protos) == SYMS and not set(protos) & set(JS.header_protos())
    jl = open(CFOLD_SHIM).read()
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
        assert name in protos, name
        cret, cparams = protos[name]
        assert (ret, types, len(parts) - 3) == (cret, cparams, len(cparams)), (name, ret, types, cret, cparams)
    assert sorted(seen) == SYMS, "one ccall per symbol"


def test_shim_is_included_after_the_fold_shim_and_the_main_shim_names_nothing():
    main = open(HH.SHIM).read()
    assert main.count('include("TempestHIP_cfold.jl")') == 1
    assert main.index('include("TempestHIP_cfold.jl")') > main.index('include("TempestHIP_fold.jl")')
    assert main.rstrip().endswith("end # module") and main.index('include("TempestHIP_cfold.jl")') > main.rindex("\nfunction ")
    code = "\n".join(line for line in main.splitlines() if not line.lstrip().startswith("#"))
    assert "tsdr_cfold" not in code
    jl = open(CFOLD_SHIM).read()
    for sig in (r"\nfunction hip_cfold!\(state::Matrix\{Float32\}, iq::Vector\{ComplexF32\}, t0::Real, T::Real, κ::Real, F::Integer;",
                r"\nfunction hip_cfold_d!\(d_state::Ptr\{Cvoid\}, d_iq::Ptr\{Cvoid\}, fmt::Symbol,",
                r"\nfunction hip_cfold_scan\(iq::Vector\{ComplexF32\},",
                r"\nfunction hip_cfold_scan_d!\(d_score::Ptr\{Cvoid\}, d_iq::Ptr\{Cvoid\}, fmt::Symbol,",
                r"\nfunction refine_carrier\(iq::Vector\{ComplexF32\}, t0::Real, T::Real, F::Integer,"):
        assert re.search(sig, jl), sig


def test_python_interface_and_delegation():
    api, mod = HH._pkg("api"), HH._pkg("cfold")
    p = inspect.signature(api.Context.cfold_d).parameters
    assert list(p) == ["self", "iq", "fmt", "scale", "n", "t0", "T", "kappa", "n_frames", "y_t", "x_t", "alpha", "state"]
    p = inspect.signature(api.Context.cfold_scan_d).parameters
    assert list(p) == ["self", "iq", "fmt", "scale", "n", "t0", "T", "kappa0", "dkappa", "n_trials", "n_frames", "y_t", "x_t", "score"]
    want = ["iq_d", "fmt", "scale", "n", "t0", "T", "n_frames", "y_t", "x_t", "oversample", "half", "levels", "shrink"]
    for fn, first in ((api.Context.refine_carrier, "self"), (mod.refine_carrier, "ctx")):
        p = inspect.signature(fn).parameters
        assert list(p) == [first] + want
        assert (p["oversample"].default, p["half"].default, p["levels"].default, p["shrink"].default) == (4, 8, 2, 4)
    assert list(inspect.signature(api.Context.cfold).parameters)[:8] == ["self", "iq", "t0", "T", "kappa", "n_frames", "y_t", "x_t"]
    assert list(inspect.signature(api.Context.cfold_scan).parameters)[:10] == ["self", "iq", "t0", "T", "kappa0", "dkappa", "n_trials",
                                                                              "n_frames", "y_t", "x_t"]
    called = DH.called_symbols(open(mod.__file__).read())
    assert set(SYMS) <= called
    assert not (DH.called_symbols(open(api.__file__).read()) & set(SYMS)), "api.py delegates; it calls none of the symbols itself"
    assert not any("fold" in s for syms in DH.api_wrappers().values() for s in syms)
    import tempestsdr_jl_amd as T
    for name in ("cfold", "cfold_d", "cfold_scan", "cfold_scan_d", "refine_carrier"):
        assert getattr(T, name) is getattr(mod, name), name
    # every call of the symbols is in cfold.py
    pkg = os.path.dirname(mod.__file__)
    for f in os.listdir(pkg):
        if f.endswith(".py") and f not in ("cfold.py", "_lib.py"):
            assert "tsdr_cfold" not in open(os.path.join(pkg, f)).read(), f


def test_every_new_entry_point_is_called_by_the_gpu_suite():
    text = open(os.path.join(ROOT, "tests", "test_cfold_gpu.py")).read()
    called = DH.called_symbols(text)
    assert set(SYMS) <= called, sorted(set(SYMS) - called)
    assert "import dptr_util as D" in text and "D.Arenas(" in text and "pytestmark = pytest.mark.gpu" in text


def test_kernel_source_keeps_its_launch_rules():
    src = open(KERNEL).read()
    code = re.sub(r"//.*", "", src)
    engine = re.sub(r"//.*", "", open(ENGINE).read())
    for name in ("cfold_tile", "cfold_direct", "cfold_scan_tile", "cfold_scan_direct", "cfold_score"):
        assert f'TSDR_LAUNCH(ctx, "{name}"' in src, name
    assert len(re.findall(r"\bTSDR_LAUNCH\(", code)) == 5 and "TSDR_LAUNCH(" not in engine, "the launches stay in the flavour's file"
    assert "ceil_div(" in code and "ceil_div(" in engine
    for text in (code, engine):
        assert "stream_grid(" not in text and "stream_blocks(" not in text, "exact grids"
        assert "hipLaunchKernelGGL" not in text, "every launch goes through TSDR_LAUNCH"
        assert not re.search(r"\batomic\w*\(", text), "no atomics at all: partial sums are combined in a fixed order"
        assert not re.search(r"\basm\b", text), "no inline assembly"
    assert "blockIdx.y * KB" in engine and re.search(r"constexpr int kBatch = (\d+);", code), "the trial batch rides in blockIdx.y"
    assert int(re.search(r"constexpr int kBatch = (\d+);", code).group(1)) >= 8
    assert re.search(r'"cfold_scan_tile", \(k_fold_engine<Coherent, kScanP, kFoldTileWaves, kBatch,', code), "the scan kernels get the batch"
    assert re.search(r'"cfold_scan_direct", \(k_fold_engine<Coherent, kFoldDirectP, kFoldDirectWaves, kBatch,', code)


def test_coordinate_helpers_are_shared_with_the_envelope_fold():
    shared = open(ENGINE).read()
    for name in ("struct FramePos", "frame_pos(", "fold_s(", "fold_tap(", "__umulhi(", "__fmul_rn(alpha, *o)", "__shfl_down(", "__syncthreads()"):
        assert name in shared, name
    assert not os.path.exists(os.path.join(CSRC, "fold_pos.h")), "the coordinate helpers moved into the engine"
    for f in ("raster_fold.hip", "raster_cfold.hip"):
        code = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        assert '#include "fold_engine.h"' in code, f
        assert "struct FramePos" not in code and not re.search(r"inline \w+ (frame_pos|fold_s|fold_tap)\(", code), f
        # ... nor the staging loop, the walk, the IIR epilogue, the reductions or a kernel of its own
        for piece in (r"frame_pos\(", r"fold_s\(", r"fold_tap\(", r"__umulhi\(", r"\bld_iq\(", r"__syncthreads\(", "__shfl", "__shared__",
                      "__global__", r"\bbeta\b", r"\*o\b", "hipMemcpyAsync", r"scratch\("):
            assert not re.search(piece, code), (f, piece)
        assert "k_fold_engine<" in code and "k_fold_score<" in code and code.count("fold_entry<") == 4, f


def test_workspace_and_build_know_the_feature():
    common = open(os.path.join(CSRC, "common.h")).read()
    slots = re.search(r"enum Slot \{(.*?)\}", common, flags=re.S).group(1)
    assert re.search(r"^\s*WS_CFOLD\b", slots, flags=re.M)
    assert slots.index("WS_COUNT") > slots.index("WS_CFOLD")
    build = open(os.path.join(ROOT, "tempestsdr.jl_amd", "build.py")).read()
    assert '"tempest_hip_cfold.h"' in build and '"tempest_hip_fold.h"' in build
    assert os.path.exists(KERNEL), "picked up by build.py's directory scan"


def test_refusals_need_no_device():
    """a NULL context is refused before anything else; nothing is dereferenced"""
    lib = HH._pkg("_lib").load()
    z = np.zeros(16, np.complex64)
    st = np.zeros(4, np.float32)
    sc = np.zeros(2, np.float64)
    args = (None, z.ctypes.data, 0, 1.0, 16, 0.0, 8.0, 0.25, 1, 2, 2)
    assert lib.tsdr_cfold_iq(*args, 0.0, st.ctypes.data) == -1 and lib.tsdr_cfold_iq_d(*args, 0.0, st.ctypes.data) == -1
    args = (None, z.ctypes.data, 0, 1.0, 16, 0.0, 8.0, 0.0, 0.125, 1, 1, 2, 2)
    assert lib.tsdr_cfold_scan_iq_d(*args, sc.ctypes.data) == -1 and lib.tsdr_cfold_scan_iq(*args, sc.ctypes.data, None) == -1
    assert not st.any() and not sc.any()


# ---------------------------------------------------------------- the reference's own known answers
GEOMS = ((0.0, 1000.0, 5, 10, 30), (3.25, 701.3, 7, 9, 14), (0.0, 40.5, 12, 4, 4))


def test_constant_sample_with_kappa_zero_folds_to_its_magnitude():
    z0 = 0.3 - 0.4j
    z = np.full(5000, z0, np.complex128)
    for t0, T, F, y, x in GEOMS:
        Z = R.zfold_mean(z, t0, T, 0.0, F, y, x)
        assert np.allclose(Z, z0, rtol=0, atol=1e-15), (t0, T, F)
        assert np.allclose(R.cfold(z, t0, T, 0.0, F, y, x), 0.5, rtol=0, atol=1e-15)
        assert abs(R.energy(Z) - y * x * 0.25) < 1e-12
    st = np.full(16, 2.0)
    assert np.allclose(R.cfold(z, 0.0, 40.5, 0.0, 12, 4, 4, 0.25, st), 0.25 * 2.0 + 0.75 * 0.5, rtol=0, atol=1e-15)


def test_constant_sample_cancels_at_the_other_roots_of_unity():
    z0 = 0.3 - 0.4j
    z = np.full(5000, z0, np.complex64)
    for t0, T, F, y, x in GEOMS:
        for j in (1, 2, F - 1, F + 1, -1):
            c = R.cfold(R.samples(z), t0, T, j / F, F, y, x)
            assert np.max(c) <= R.eps_c(F, abs(z0)), (F, j, float(np.max(c)))
        for j in (0, F, -2 * F):   # ... and comes back at every multiple of F
            assert np.allclose(R.cfold(R.samples(z), t0, T, j / F, F, y, x), abs(complex(np.complex64(z0))), rtol=0, atol=1e-12)


def test_pure_tone_folds_to_its_amplitude_times_the_interpolation_loss():
    """z[k] = A exp(2 pi i nu k), kappa = nu T: frame f's sample at u = k + d is A exp(2 pi i nu k) (1 + d (exp(2 pi i nu) - 1)), the
    de-rotation leaves exp(2 pi i nu (u - f T - d)), so |Z(m)| = A |mean_f g(d_f(m))|, g(d) = exp(-2 pi i nu d) (1 + d (exp(2 pi i nu) - 1))"""
    A, nu = 0.75, 0.0137
    t0, T, F, y, x = 5.5, 1207.73, 7, 11, 23
    P, n = y * x, 9000
    z = A * np.exp(2j * np.pi * nu * np.arange(n))
    u = np.array([(t0 + f * T) + ((np.arange(P) + 0.5) * (T / P) - 0.5) for f in range(F)])
    assert u.min() > 0 and u.max() < n - 1, "no clamp acts"
    d = u - np.floor(u)
    g = np.exp(-2j * np.pi * nu * d) * (1.0 + d * (np.exp(2j * np.pi * nu) - 1.0))
    want = A * np.abs(g.mean(axis=0))
    got = np.abs(R.zfold_mean(z, t0, T, nu * T, F, y, x))
    assert np.allclose(got, want, rtol=0, atol=1e-9), float(np.max(np.abs(got - want)))
    assert np.all(want < A) and np.all(want > A * math.cos(math.pi * nu) - 1e-12), "the loss is the chord's: at most 1 - cos(pi nu)"
    # and one turn per frame more is the same picture within the rounding of f * kappa
    assert np.allclose(np.abs(R.zfold_mean(z, t0, T, nu * T + 1.0, F, y, x)), want, rtol=0, atol=1e-9)


def test_kappa_zero_on_real_data_is_the_envelope_fold():
    rng = np.random.default_rng(3)
    for t0, T, F, y, x in GEOMS:
        a = np.abs(rng.normal(1.0, 0.3, 5000)).astype(np.float32)
        Z = R.zfold_mean(a.astype(np.complex64), t0, T, 0.0, F, y, x)
        m = FR.fold_mean(a, t0, T, F, y, x)
        assert np.allclose(Z.imag, 0.0, rtol=0, atol=0) and np.allclose(np.abs(Z), m, rtol=0, atol=1e-15)
        assert np.allclose(R.cfold(a.astype(np.complex64), t0, T, 0.0, F, y, x), FR.fold(a, t0, T, F, y, x), rtol=0, atol=1e-15)


def test_bounds_and_ladder_helpers():
    u = 2.0 ** -24
    assert R.eps_z(4, 0.5) == math.sqrt(2.0) * 16 * u * 0.5
    assert R.eps_c(4, 0.5) == 1.5 * 20 * u * 0.5 and R.eps_c(4, 0.5, 3.0) == 1.5 * 20 * u * 3.0
    assert R.eps_z(7, 1.0) + 6 * u <= R.eps_c(7, 1.0), "eps_c covers eps_z, the square root (2u) and the IIR (4u)"
    assert R.energy(np.array([3 + 4j, 1j])) == 26.0
    assert R.samples(np.array([1 + 2j], np.complex64)).dtype == np.complex128
    # the ladder on a noiseless tone finds kappa = frac(nu T) to its last step
    nu, T, F, y, x = 0.0137, 1207.73, 8, 11, 23
    z = 0.5 * np.exp(2j * np.pi * nu * np.arange(F * 1210 + 10))
    k_hat, last, scores = R.ladder(z, 0.0, T, F, y, x)
    assert [len(s) for s in scores] == [32, 17] and last == 1.0 / 128
    true = (nu * T) % 1.0
    assert abs((k_hat - true + 0.5) % 1.0 - 0.5) <= last, (k_hat, true)
    assert HH._pkg("cfold").first_max is HH._pkg("fold").first_max
