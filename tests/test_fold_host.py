"""Host-side checks of coherent frame folding (no GPU): include/tempest_hip_fold.h, its ctypes table (_lib._SIGS_FOLD), its Python
module (fold.py) and its Julia shim (julia/TempestHIP_fold.jl) agree with each other and with the library, the way
test_display_host.py pins tempest_hip_display.h; fold_plan's known answers; the launch rules of csrc/raster_fold.hip; and the numpy
reference the GPU tests compare against (tests/fold_ref.py) on answers known without it."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import fold_ref as R
import test_dptr_host as DH
import test_hires_host as HH
import test_julia_shim_static as JS

ROOT = HH.ROOT
MAIN_H = HH.MAIN_H
FOLD_H = os.path.join(ROOT, "include", "tempest_hip_fold.h")
DISP_H = os.path.join(ROOT, "include", "tempest_hip_display.h")
FOLD_SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP_fold.jl")
KERNEL = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "raster_fold.hip")
ENGINE = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "fold_engine.h")   # the kernels and the host path, shared with raster_cfold.hip

SYMS = ["tsdr_fold_iq", "tsdr_fold_iq_d", "tsdr_fold_scan_iq", "tsdr_fold_scan_iq_d"]
HEAD = ["tsdr_ctx *ctx", "const void *iq", "int iq_fmt", "float scale", "size_t n", "double t0"]
FOLD = HEAD + ["double T", "int n_frames", "int y_t", "int x_t", "float alpha", "float *state"]
SCAN = HEAD + ["double T0", "double dT", "int n_trials", "int n_frames", "int y_t", "int x_t", "double *score"]


# ---------------------------------------------------------------- header, table, library, shims
def test_header_declares_the_four_forms_and_the_constants():
    p = HH._protos(FOLD_H)
    assert sorted(p) == SYMS
    assert p["tsdr_fold_iq"] == p["tsdr_fold_iq_d"] == FOLD
    assert p["tsdr_fold_scan_iq_d"] == SCAN and p["tsdr_fold_scan_iq"] == SCAN + ["int *best"]
    text = open(FOLD_H).read()
    assert re.search(r"^#define TSDR_FOLD_MAX_TRIALS 4096$", text, flags=re.M)
    assert re.search(r"^#define TSDR_FOLD_STAGE_MAX 240$", text, flags=re.M)
    lib = HH._pkg("_lib")
    assert (lib.FOLD_MAX_TRIALS, lib.FOLD_STAGE_MAX) == (4096, 240)


def test_main_header_includes_it_once_after_the_display_header():
    main = open(MAIN_H).read()
    assert main.count('#include "tempest_hip_fold.h"') == 1
    assert main.index('#include "tempest_hip_fold.h"') > main.index('#include "tempest_hip_display.h"')
    for path in (MAIN_H, HH.HIRES_H, DISP_H, os.path.join(ROOT, "include", "tempest_hip_register.h")):
        assert not re.search(r"tsdr_fold|TSDR_FOLD_", HH._strip(path)), path
    guard = open(FOLD_H).read()
    assert "#ifndef TEMPEST_HIP_FOLD_H" in guard and "#ifndef TEMPEST_HIP_DISPLAY_H\n#error" in guard


def test_header_states_the_contract():
    src = " ".join(open(FOLD_H).read().split())
    for phrase in ("INPUT", "SAMPLING", "ACCURACY", "REPRODUCIBILITY", "FORMAT INVARIANCE", "SCORE", "REFUSALS", "COST",
                   "GUI.jl:103-109,137,166", "u_f(m) = (t0 + f*T) + ((m + 1/2)*(T/P) - 1/2)", "k = min(floor(u), n-2)", "d may be 1",
                   "state[p*y_t + l]", "the state is NOT READ", "sig_to_image(amDemod(iq))", "instead of clamping", "POINT-SAMPLES",
                   "does not depend on tsdr_set_precision", "2^-26 samples", "eps = (F + 8) * 2^-24 * max(amax, max|state_in|)",
                   "no floating-point atomics", "host-expanded ComplexF32", "score = sum_m x_m^2 - (sum_m x_m)^2 / P",
                   "2*eps*sqrt(P*ref) + P*eps^2", "a NaN never wins", "nothing written and nothing enqueued", "P >= 2^31", "n >= 2^31",
                   "t0 + F*T > n", "at the largest trial period", "alpha outside [0, 1] or NaN", "16-byte aligned",
                   "F == 0 (with everything else valid) is TSDR_OK and touches nothing", "iq is never written", "8n + 8P",
                   "W = ceil(128*T/P) + 3", "TSDR_FOLD_STAGE_MAX = 240", '"fold_tile"', '"fold_direct"', '"fold_scan_tile"',
                   '"fold_scan_direct"', '"fold_score"', '"wait_ms"'):
        assert phrase in src, phrase


def test_header_table_and_library_agree():
    lib = HH._pkg("_lib")
    assert sorted(HH._protos(FOLD_H)) == SYMS == lib.exported_names_fold()
    for other in (lib._SIGS, lib._SIGS_IQ, lib._SIGS_CPLX, lib._SIGS_HIRES, lib._SIGS_REGISTER, lib._SIGS_DISPLAY):
        assert not set(other) & set(lib._SIGS_FOLD)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    for sym in SYMS:
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_fold.h but not exported"
        assert getattr(bound, sym).restype is C.c_int and getattr(bound, sym).argtypes == lib._SIGS_FOLD[sym][1], sym


def test_table_argtypes_match_the_prototypes():
    lib = HH._pkg("_lib")
    ct = {"i32": C.c_int, "i64": C.c_size_t, "f32": C.c_float, "f64": C.c_double}
    for sym, params in HH._protos(FOLD_H).items():
        res, args = lib._SIGS_FOLD[sym]
        assert res is C.c_int and len(args) == len(params), sym
        for k, (a, p) in enumerate(zip(args, params)):
            cls = JS.c_class(p)
            assert (a is C.c_void_p) if cls == "ptr" else (a is ct[cls]), (sym, k, p, a)


def test_every_ccall_of_the_fold_shim_matches_its_prototype():
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(tsdr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", HH._strip(FOLD_H), flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        protos[name] = ("ptr" if "*" in ret else JS.c_class(ret + " x"), [JS.c_class(p) for p in JS.split_args(args)])
    assert sorted(protos) == SYMS and not set(protos) & set(JS.header_protos())
    jl = open(FOLD_SHIM).read()
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


def test_shim_is_included_after_the_display_shim_and_the_main_shim_names_nothing():
    main = open(HH.SHIM).read()
    assert main.count('include("TempestHIP_fold.jl")') == 1
    assert main.index('include("TempestHIP_fold.jl")') > main.index('include("TempestHIP_display.jl")')
    assert main.rstrip().endswith("end # module") and main.index('include("TempestHIP_fold.jl")') > main.rindex("\nfunction ")
    code = "\n".join(line for line in main.splitlines() if not line.lstrip().startswith("#"))
    assert "tsdr_fold" not in code
    jl = open(FOLD_SHIM).read()
    for sig in (r"\nfunction fold_plan\(n::Integer, t0::Real, T::Real\)",
                r"\nfunction hip_fold!\(state::Matrix\{Float32\}, iq::Vector\{ComplexF32\}, t0::Real, T::Real, F::Integer;",
                r"\nfunction hip_fold_d!\(d_state::Ptr\{Cvoid\}, d_iq::Ptr\{Cvoid\}, fmt::Symbol,",
                r"\nfunction hip_fold_scan\(iq::Vector\{ComplexF32\},",
                r"\nfunction hip_fold_scan_d!\(d_score::Ptr\{Cvoid\}, d_iq::Ptr\{Cvoid\}, fmt::Symbol,"):
        assert re.search(sig, jl), sig
    assert "t + (F + 1) * p - n64" in jl, "fold_plan keeps the phase"


def test_python_interface_and_delegation():
    api, mod = HH._pkg("api"), HH._pkg("fold")
    p = inspect.signature(api.Context.fold_d).parameters
    assert list(p) == ["self", "iq", "fmt", "scale", "n", "t0", "T", "n_frames", "y_t", "x_t", "alpha", "state"]
    p = inspect.signature(api.Context.fold_scan_d).parameters
    assert list(p) == ["self", "iq", "fmt", "scale", "n", "t0", "T0", "dT", "n_trials", "n_frames", "y_t", "x_t", "score"]
    p = inspect.signature(api.Context.refine_period).parameters
    assert list(p) == ["self", "iq_d", "fmt", "scale", "n", "T_guess", "n_frames", "y_t", "x_t", "dT", "half", "levels", "shrink"]
    assert (p["dT"].default, p["half"].default, p["levels"].default, p["shrink"].default) == (0.125, 8, 2, 4)
    p = inspect.signature(mod.refine_period).parameters
    assert list(p)[:13] == ["ctx", "iq_d", "fmt", "scale", "n", "T_guess", "n_frames", "y_t", "x_t", "dT", "half", "levels", "shrink"]
    assert (p["dT"].default, p["half"].default, p["levels"].default, p["shrink"].default) == (0.125, 8, 2, 4)
    assert list(inspect.signature(api.Context.fold).parameters)[:7] == ["self", "iq", "t0", "T", "n_frames", "y_t", "x_t"]
    assert list(inspect.signature(api.Context.fold_scan).parameters)[:9] == ["self", "iq", "t0", "T0", "dT", "n_trials", "n_frames", "y_t", "x_t"]
    called = DH.called_symbols(open(mod.__file__).read())
    assert set(SYMS) <= called
    assert not (DH.called_symbols(open(api.__file__).read()) & set(SYMS)), "api.py delegates; it calls none of the symbols itself"
    assert not any("fold" in s for syms in DH.api_wrappers().values() for s in syms)
    import tempestsdr_jl_amd as T
    for name in ("fold", "fold_d", "fold_scan", "fold_scan_d", "fold_plan", "refine_period"):
        assert getattr(T, name) is getattr(mod, name), name
    # every call of the symbols is in fold.py
    pkg = os.path.dirname(mod.__file__)
    for f in os.listdir(pkg):
        if f.endswith(".py") and f not in ("fold.py", "_lib.py"):
            assert "tsdr_fold" not in open(os.path.join(pkg, f)).read(), f


def test_every_new_entry_point_is_called_by_the_gpu_suite():
    text = open(os.path.join(ROOT, "tests", "test_fold_gpu.py")).read()
    called = DH.called_symbols(text)
    assert set(SYMS) <= called, sorted(set(SYMS) - called)
    assert "import dptr_util as D" in text and "D.Arenas(" in text and "pytestmark = pytest.mark.gpu" in text


def test_kernel_source_keeps_its_launch_rules():
    src = open(KERNEL).read()
    code = re.sub(r"//.*", "", src)
    engine = re.sub(r"//.*", "", open(ENGINE).read())
    assert '#include "fold_engine.h"' in code, "the kernels are the engine's"
    for name in ("fold_tile", "fold_direct", "fold_scan_tile", "fold_scan_direct", "fold_score"):
        assert f'TSDR_LAUNCH(ctx, "{name}"' in src, name
    assert len(re.findall(r"\bTSDR_LAUNCH\(", code)) == 5 and "TSDR_LAUNCH(" not in engine, "the launches stay in the flavour's file"
    assert "ceil_div(" in code and "ceil_div(" in engine
    for text in (code, engine):
        assert "stream_grid(" not in text and "stream_blocks(" not in text, "exact grids"
        assert "hipLaunchKernelGGL" not in text, "every launch goes through TSDR_LAUNCH"
        assert not re.search(r"\batomic\w*\(", text), "no atomics at all: partial sums are combined in a fixed order"
        assert not re.search(r"atomic\w*\([^;]*float", text)
        assert not re.search(r"\basm\b", text), "no inline assembly"


def test_workspace_and_build_know_the_feature():
    common = open(os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "common.h")).read()
    slots = re.search(r"enum Slot \{(.*?)\}", common, flags=re.S).group(1)
    assert re.search(r"^\s*WS_FOLD\b", slots, flags=re.M)
    assert slots.index("WS_COUNT") > slots.index("WS_FOLD")
    build = open(os.path.join(ROOT, "tempestsdr.jl_amd", "build.py")).read()
    assert '"tempest_hip_fold.h"' in build and '"tempest_hip_display.h"' in build
    assert os.path.exists(KERNEL), "picked up by build.py's directory scan"


def test_refusals_need_no_device():
    """a NULL context is refused before anything else; nothing is dereferenced"""
    lib = HH._pkg("_lib").load()
    z = np.zeros(16, np.complex64)
    st = np.zeros(4, np.float32)
    sc = np.zeros(2, np.float64)
    args = (None, z.ctypes.data, 0, 1.0, 16, 0.0, 8.0, 1, 2, 2)
    assert lib.tsdr_fold_iq(*args, 0.0, st.ctypes.data) == -1 and lib.tsdr_fold_iq_d(*args, 0.0, st.ctypes.data) == -1
    args = (None, z.ctypes.data, 0, 1.0, 16, 0.0, 8.0, 0.0, 1, 1, 2, 2)
    assert lib.tsdr_fold_scan_iq_d(*args, sc.ctypes.data) == -1 and lib.tsdr_fold_scan_iq(*args, sc.ctypes.data, None) == -1
    assert not st.any() and not sc.any()


# ---------------------------------------------------------------- fold_plan
def _plan():
    return HH._pkg("fold").fold_plan


def test_fold_plan_known_answers():
    plan = _plan()
    assert plan(100, 0.0, 10.0) == (10, 10.0), "t0 + F*T == n exactly: all ten frames, and the next buffer starts a whole period in"
    assert plan(100, 0.5, 10.0) == (9, 0.5)
    assert plan(100, 5.0, 9.5) == (10, 9.5), "5 + 10 * 9.5 == 100 exactly"
    assert plan(1000, 3.25, 100.5) == (9, 3.25 + 10 * 100.5 - 1000)
    assert plan(10, 3.0, 20.0) == (0, 13.0), "no whole frame: the phase still moves on"
    assert plan(10, 12.0, 20.0) == (0, 2.0), "no frame starts in this buffer"
    F, nxt = plan(2_000_000, 123.456, 333_333.333)
    assert F == 5 and nxt == pytest.approx(123.456 + 6 * 333_333.333 - 2_000_000, abs=1e-9)
    for bad in ((100, -1.0, 10.0), (100, 0.0, 0.0), (100, 0.0, float("nan")), (100, float("inf"), 10.0)):
        with pytest.raises(AssertionError):
            plan(*bad)


def test_fold_plan_next_t0_lies_in_0_T():
    plan = _plan()
    rng = np.random.default_rng(7)
    for _ in range(2000):
        T = float(rng.uniform(2.0, 5000.0))
        n = int(rng.integers(int(T) + 1, 200_000))
        t0 = float(rng.uniform(0.0, T))
        F, nxt = plan(n, t0, T)
        assert F >= 0 and t0 + F * T <= n < t0 + (F + 1) * T, (n, t0, T, F)
        assert 0.0 < nxt <= T, (n, t0, T, F, nxt)
    for n, T in ((1000, 10.0), (4096, 2.0), (333, 111.0)):
        assert plan(n, 0.0, T) == (int(n // T), T)


def test_fold_plan_chains_buffers_like_one_long_buffer():
    plan = _plan()
    T, t0 = 9150.37, 17.25
    sizes = (40_000, 55_001, 47_123)
    long_starts = [t0 + f * T for f in range(plan(sum(sizes), t0, T)[0])]
    starts, base, t = [], 0, t0
    for n in sizes:
        F, nxt = plan(n, t, T)
        starts += [base + t + f * T for f in range(F)]
        base, t = base + n, nxt
    # every chained start is a start of the long buffer, to 1e-9; the frames that straddle a seam are the ones left out
    grid = np.array(long_starts)
    for s in starts:
        assert np.min(np.abs(grid - s)) <= 1e-9, s
    assert len(starts) == len(long_starts) - 2 and len(set(np.round((np.array(starts) - t0) / T).astype(int))) == len(starts)


# ---------------------------------------------------------------- the reference's own known answers
def test_constant_amplitude_folds_to_the_constant():
    a = np.full(5000, 0.375, np.float32)
    for t0, T, F, y, x in ((0.0, 1000.0, 5, 10, 30), (3.25, 701.3, 7, 9, 14), (0.0, 40.5, 100, 4, 4)):
        m = R.fold_mean(a, t0, T, F, y, x)
        assert np.all(m == 0.375), (t0, T, F)
        assert R.score_of(m) == 0.0
    st = np.full(16, 2.0)
    assert np.all(R.fold(a, 0.0, 40.5, 100, 4, 4, 0.25, st) == 0.25 * 2.0 + 0.75 * 0.375)


def test_ramp_folds_to_the_mean_coordinate():
    c, n = 0.001, 20_000
    a = (c * np.arange(n)).astype(np.float64)   # exact f64 ramp: interpolation of a line is the line
    t0, T, F, y, x = 5.5, 1207.73, 7, 11, 23
    P = y * x
    m = R.fold_mean(a, t0, T, F, y, x)
    u = np.array([(t0 + f * T) + ((np.arange(P) + 0.5) * (T / P) - 0.5) for f in range(F)])
    assert u.min() > 0 and u.max() < n - 1, "no clamp acts"
    assert np.allclose(m, c * u.mean(axis=0), rtol=0, atol=1e-12 * c * n)
    # and where the lower clamp acts (t0 = 0, fewer samples than pixels): the first pixels sit at a[0]
    m = R.fold_mean(a, 0.0, 100.0, 1, 20, 20)
    assert m[0] == 0.0 and m[1] == 0.0 and m[2] > 0.0


def test_one_frame_from_zero_is_sig_to_image():
    rng = np.random.default_rng(3)
    for S, y, x in ((1208, 70, 150), (5000, 8, 16), (300, 17, 23), (391, 17, 23)):
        a = np.abs(rng.normal(1.0, 0.3, S)).astype(np.float32)
        m = R.fold_mean(a, 0.0, float(S), 1, y, x)
        assert np.allclose(m, R.sig_to_image_1d(a, y, x), rtol=0, atol=1e-12), (S, y, x)
        # state order: element (l, p) at p * y_t + l
        st = R.to_state(m, y, x)
        assert st[3 * y + 2] == m[2 * x + 3]


def test_score_bound_and_margin_helpers():
    x = np.array([1.0, 2.0, 3.0, 6.0])
    assert R.score_of(x) == pytest.approx(4 * np.var(x))
    assert R.first_max([1.0, float("nan"), 3.0, 3.0, 2.0]) == 2 and R.first_max([float("nan")] * 3) == -1
    assert HH._pkg("fold").first_max([1.0, float("nan"), 3.0, 3.0, 2.0]) == 2
    assert R.top2_margin([1.0, 4.0, 3.0]) == 0.25
    assert R.eps(7, 0.5) == 15 * 2.0 ** -24 * 0.5 and R.eps(1, 0.5, 3.0) == 9 * 2.0 ** -24 * 3.0
    e = 1e-6
    assert R.score_bound(e, 100, 4.0) == pytest.approx(2 * e * 20.0 + 100 * e * e)


def test_amplitudes_round_once():
    z = np.array([3 + 4j, 1e-20 + 0j, 0j, 1 + 1j], np.complex64)
    a = R.amplitudes(z)
    assert a.dtype == np.float32 and a[0] == 5.0 and a[2] == 0.0 and a[1] == np.float32(1e-20) and a[3] == np.float32(np.sqrt(2.0))
