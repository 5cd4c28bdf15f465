"""Host-side checks of the registration to the raster pixel (no GPU): include/tempest_hip_register.h, its ctypes table
(_lib._SIGS_REGISTER), its Python module (register.py) and its Julia shim (julia/TempestHIP_register.jl) agree with each other and
with the library, the way test_hires_host.py pins tempest_hip_hires.h; the numpy reference the GPU tests compare against
(tests/register_ref.py) is checked against its brute-force form, on a constructed tie, on known displacements, and -- on the CPU
oracle's rasters -- for what the feature is for: the refined average is sharper than the coarse one."""
import ctypes as C
import functools
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import hires_ref as H
import oracle_lib as O
import register_ref as R
import test_dptr_host as DH
import test_hires_host as HH
import test_julia_shim_static as JS

ROOT = HH.ROOT
MAIN_H, HIRES_H = HH.MAIN_H, HH.HIRES_H
REG_H = os.path.join(ROOT, "include", "tempest_hip_register.h")
REG_SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP_register.jl")
KERNEL = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "raster_register.hip")

SYMS = sorted(["tsdr_raster_profiles_d", "tsdr_raster_register_d", "tsdr_raster_register", "tsdr_frames_hires_shifts"])
REGISTER = ["tsdr_ctx *ctx", "const float *rasters", "int n_frames", "int y_t", "int x_t", "const float *ref", "const int *shifts",
            "int shift_units", "int img_h", "int img_w", "int d_y", "int d_x", "int *shifts_out", "double *scores"]
GRID = (600, 800)


# ---------------------------------------------------------------- header, table, library, shims
def test_header_declares_the_four_entry_points():
    p = HH._protos(REG_H)
    assert sorted(p) == SYMS
    assert p["tsdr_raster_register"] == p["tsdr_raster_register_d"] == REGISTER
    assert p["tsdr_raster_profiles_d"] == ["tsdr_ctx *ctx", "const float *rasters", "int n_frames", "int y_t", "int x_t", "double *col",
                                           "double *row"]
    assert p["tsdr_frames_hires_shifts"] == ["tsdr_ctx *ctx", "int max_frames", "int *shifts", "int *n_frames"]


def test_other_headers_declare_none_of_it():
    main = open(MAIN_H).read()
    assert main.count('#include "tempest_hip_register.h"') == 1
    assert main.index('#include "tempest_hip_register.h"') > main.index('#include "tempest_hip_hires.h"')
    for path in (MAIN_H, HIRES_H):
        code = HH._strip(path)
        assert not re.search(r"raster_profiles|raster_register|hires_shifts", code), path
    guard = open(REG_H).read()
    assert "#ifndef TEMPEST_HIP_REGISTER_H" in guard and "#ifndef TEMPEST_HIP_HIRES_H\n#error" in guard


def test_header_states_the_contract():
    src = " ".join(open(REG_H).read().split())
    for phrase in ("PROFILES", "COARSE SHIFT", "REFERENCE PROFILES", "SCORES", "CHOICE", "OUTPUT", "INDEPENDENCE", "REFUSALS", "COST",
                   "THE LOOP", "FIXED", "no floating-point atomics", "FLAT", "IEEE-equal", "NO FMA", "0, -1, +1, -2, +2", "strict >",
                   "A NaN score never wins", "(r0_y + d*_y) mod y_t", "index d + D", "2*d_y + 1 > y_t", "nothing written",
                   "never written", '"hires_refine"', "0 .. 8", "no environment preset", "min(ceil(k*y_t/600), (y_t-1)/2)",
                   "min(ceil(k*x_t/800), (x_t-1)/2)", "do_align == 0", "tsdr_sync_guard_margins"):
        assert phrase in src, phrase


def test_header_table_and_library_agree():
    lib = HH._pkg("_lib")
    assert sorted(HH._protos(REG_H)) == SYMS == lib.exported_names_register()
    for other in (lib._SIGS, lib._SIGS_IQ, lib._SIGS_CPLX, lib._SIGS_HIRES):
        assert not set(other) & set(lib._SIGS_REGISTER)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    for sym in SYMS:
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_register.h but not exported"
        assert getattr(bound, sym).restype is C.c_int and getattr(bound, sym).argtypes == lib._SIGS_REGISTER[sym][1], sym


def test_table_argtypes_match_the_prototypes():
    lib = HH._pkg("_lib")
    ct = {"i32": C.c_int, "i64": C.c_size_t, "f32": C.c_float, "f64": C.c_double}
    for sym, params in HH._protos(REG_H).items():
        res, args = lib._SIGS_REGISTER[sym]
        assert res is C.c_int and len(args) == len(params), sym
        for k, (a, p) in enumerate(zip(args, params)):
            cls = JS.c_class(p)
            if cls == "ptr":
                assert a is C.c_void_p or (isinstance(a, type) and issubclass(a, C._Pointer)), (sym, k, p, a)
                if a is not C.c_void_p:
                    want = {"int": C.c_int, "float": C.c_float, "double": C.c_double}[re.sub(r"\bconst\b", "", p).split()[0]]
                    assert a._type_ is want, (sym, k, p, a)
            else:
                assert a is ct[cls], (sym, k, p, a)


def test_every_ccall_of_the_register_shim_matches_its_prototype():
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(tsdr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", HH._strip(REG_H), flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        protos[name] = ("ptr" if "*" in ret else JS.c_class(ret + " x"), [JS.c_class(p) for p in JS.split_args(args)])
    assert sorted(protos) == SYMS and not set(protos) & set(JS.header_protos())
    jl = open(REG_SHIM).read()
    seen = set()
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
        seen.add(name)
        assert name in protos, name
        cret, cparams = protos[name]
        assert (ret, types, len(parts) - 3) == (cret, cparams, len(cparams)), (name, ret, types, cret, cparams)
    assert seen == {"tsdr_raster_register"}, "hip_raster_register! binds the host form"


def test_shim_is_included_after_the_hires_shim_and_the_main_shim_names_nothing():
    main = open(HH.SHIM).read()
    assert main.count('include("TempestHIP_register.jl")') == 1
    assert main.index('include("TempestHIP_register.jl")') > main.index('include("TempestHIP_hires.jl")')
    code = "\n".join(line for line in main.splitlines() if not line.lstrip().startswith("#"))
    assert not re.search(r"tsdr_raster_profiles|tsdr_raster_register|tsdr_frames_hires_shifts", code)
    jl = open(REG_SHIM).read()
    m = re.search(r"\nfunction hip_raster_register!\(shifts_out::Matrix\{Cint\}, rasters::Array\{Float32,3\},(.*?)\nend", jl, flags=re.S)
    assert m and "ccall((:tsdr_raster_register, LIB)" in m.group(1) and "SHIFT_UNITS[units]" in m.group(1)
    assert 'hip_set_option("hires_refine", k)' in jl


def test_python_interface_and_delegation():
    api, mod = HH._pkg("api"), HH._pkg("register")
    p = inspect.signature(api.Context.raster_register).parameters
    assert list(p) == ["self", "rasters", "d_y", "d_x", "ref", "shifts", "units", "grid", "want_scores"]
    assert (p["ref"].default, p["shifts"].default, p["units"].default, p["grid"].default) == (None, None, "raster", GRID)
    assert list(inspect.signature(api.Context.raster_profiles).parameters) == ["self", "rasters"]
    assert hasattr(api.Context, "raster_register_d") and hasattr(api.Context, "hires_shifts")
    called = DH.called_symbols(open(mod.__file__).read())
    assert set(SYMS) <= called
    assert not (DH.called_symbols(open(api.__file__).read()) & set(SYMS)), "api.py delegates; it calls none of the symbols itself"
    assert not any("register" in s or "profiles" in s for syms in DH.api_wrappers().values() for s in syms)
    assert mod.n_scores(2, 3) == 12


def test_every_new_entry_point_is_called_by_the_gpu_suite():
    text = open(os.path.join(ROOT, "tests", "test_register_gpu.py")).read()
    called = DH.called_symbols(text)
    missing = [s for s in SYMS if s not in called]
    assert not missing, missing
    assert "import dptr_util as D" in text and "D.Arenas(" in text and "pytestmark = pytest.mark.gpu" in text


def test_kernel_source_keeps_its_launch_rules():
    src = open(KERNEL).read()
    assert "stream_grid(" not in src and "stream_blocks(" not in src and "ceil_div(" in src
    assert "atomic" not in re.sub(r"//.*", "", src), "sums are reproducible: per-tile partials, no atomics"
    for name in ("raster_profiles", "raster_profile_sum", "raster_register", "raster_shifts"):
        assert f'TSDR_LAUNCH(ctx, "{name}"' in src, name
    assert "__dadd_rn(s[q], __dmul_rn(a, pf[k]))" in src, "product then sum, separately rounded"
    accum = open(HH.KERNEL).read()
    assert "register_launch(" in accum and "TSDR_SHIFT_RASTER, 0, 0, alpha_hires" in accum


def test_option_workspace_and_build_know_the_feature():
    ctx_src = open(os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "ctx.hip")).read()
    assert '"hires_refine"' in ctx_src and "HIRES_REFINE" not in ctx_src, "an option without an environment preset"
    common = open(os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "common.h")).read()
    slots = re.search(r"enum Slot \{(.*?)\}", common, flags=re.S).group(1)
    names = re.findall(r"^\s*(WS_[A-Z0-9_]+)\b", slots, flags=re.M)
    k = names.index("WS_HIRES_IDX")
    assert names[k + 1:] == ["WS_HIRES_SHIFTS", "WS_REG_PART", "WS_REG_PROF", "WS_REG_SCORES", "WS_COUNT"], "appended to the enum"
    build = open(os.path.join(ROOT, "tempestsdr.jl_amd", "build.py")).read()
    assert '"tempest_hip_register.h"' in build and '"tempest_hip_hires.h"' in build


# ---------------------------------------------------------------- the reference against its definition
def _ints(rng, shape, lo=0, hi=41):
    return np.asfortranarray(rng.integers(lo, hi, shape).astype(np.float32))


def _same(a, b):
    sa, ca = a[0], a[1]
    sb, cb = b[0], b[1]
    return np.array_equal(sa, sb) and np.array_equal(ca, cb, equal_nan=True)


def test_reference_equals_the_brute_force_loop():
    rng = np.random.default_rng(3)
    y_t, x_t, n = 7, 10, 3
    rasters = [_ints(rng, (y_t, x_t)) for _ in range(n)]
    ref = _ints(rng, (y_t, x_t))
    big = 2 ** 31 - 1
    cases = [(None, "raster", GRID), ([(0, 0)] * n, "raster", GRID), ([(6, 4), (-1, -9), (7, 12)], "raster", GRID),
             ([(big, -big - 1), (-big - 1, big), (3, 3)], "raster", GRID), ([(1, 1), (599, 799), (-300, 1000)], "image", GRID),
             ([(big, -big - 1), (-big - 1, big), (-5, 7)], "image", GRID), ([(3, 2), (7, 5), (-1, 0)], "image", (7, 5))]
    for shifts, units, grid in cases:
        for d_y, d_x in ((0, 0), (1, 2), (3, 4)):
            for rf in (ref, None, np.full((y_t, x_t), 3.0, np.float32)):   # a picture, none, a flat one
                got = R.register(rasters, rf, d_y, d_x, shifts, units, grid)
                want = R.brute(rasters, rf, d_y, d_x, shifts, units, grid)
                assert _same(got, want), (shifts, units, d_y, d_x)
                assert got[0].dtype == np.int32 and np.all(got[0] >= 0) and np.all(got[0] < [y_t, x_t])
    # no ref, or a flat one: the reference is frame 0 under its own coarse shift, so frame 0 gets d = 0
    sh = [(2, 3), (1, 1), (0, 5)]
    a, b = R.register(rasters, None, 3, 4, sh), R.register(rasters, np.zeros((y_t, x_t), np.float32), 3, 4, sh)
    assert _same(a, b) and tuple(a[2][0]) == (0, 0) and tuple(a[0][0]) == (2, 3)
    # flat on ONE axis only: ref constant along x has a flat column profile but not a flat row profile
    half = np.asfortranarray(np.tile(np.arange(y_t, dtype=np.float32)[:, None], (1, x_t)))
    got, want = R.register(rasters, half, 2, 2, sh), R.brute(rasters, half, 2, 2, sh)
    assert _same(got, want)
    assert np.array_equal(got[1][:, 5:], a[1][:, 7 + 2: 7 + 2 + 5]), "the x block falls back to frame 0 (d_x = 2 inside the d_x = 4 block)"


def test_a_nan_frame_gets_no_refinement_and_leaves_the_others_alone():
    rng = np.random.default_rng(4)
    y_t, x_t = 6, 9
    rasters = [_ints(rng, (y_t, x_t)) for _ in range(3)]
    ref = _ints(rng, (y_t, x_t))
    clean = R.register(rasters, ref, 2, 3, [(1, 2), (3, 4), (5, 6)])
    bad = [r.copy() for r in rasters]
    bad[1][2, 3] = np.nan
    got = R.register(bad, ref, 2, 3, [(1, 2), (3, 4), (5, 6)])
    assert _same(got, R.brute(bad, ref, 2, 3, [(1, 2), (3, 4), (5, 6)]))
    assert tuple(got[0][1]) == (3, 4) and np.all(np.isnan(got[1][1])), "every score of the frame is NaN: the running best stays d = 0"
    assert np.array_equal(got[0][[0, 2]], clean[0][[0, 2]]) and np.array_equal(got[1][[0, 2]], clean[1][[0, 2]])
    # a NaN in ref: its profiles are not flat (NaN != NaN), every score is NaN, every frame keeps its coarse shift
    nref = ref.copy()
    nref[0, 0] = np.nan
    assert not R.is_flat(R.profiles(nref)[0])
    got = R.register(rasters, nref, 2, 3, [(1, 2), (3, 4), (5, 6)])
    assert np.array_equal(got[0], [(1, 2), (3, 4), (5, 6)]) and np.all(np.isnan(got[1]))


def tie_case(y_t=4, x_t=8):
    """a period-2 column pattern and the same picture one column on: s(-1) == s(+1) > s(0) -> (rasters, ref)"""
    col = np.where(np.arange(x_t) % 2 == 0, 5.0, 1.0).astype(np.float32)
    ref = np.asfortranarray(np.tile(col, (y_t, 1)) + np.arange(y_t, dtype=np.float32)[:, None])
    return [np.asfortranarray(np.roll(ref, 1, axis=1))], ref


def test_constructed_tie_goes_to_the_negative_candidate():
    rasters, ref = tie_case()
    out, sc, d = R.register(rasters, ref, 1, 1)
    sx = sc[0][3:]
    assert sx[0] == sx[2] > sx[1], sx
    assert d[0][1] == -1 and out[0][1] == 8 - 1
    assert _same((out, sc), R.brute(rasters, ref, 1, 1))
    # with a wider window the same tie at every odd |d|: the smallest |d| wins, the negative one first
    assert R.register(rasters, ref, 1, 3)[2][0][1] == -1


# ---------------------------------------------------------------- known displacement
DISP = dict(y_t=48, x_t=160, grid=(12, 20), sigmas=(0, 4, 16))


def displacement_case(sigma, seed=0, trials=12):
    """ref: small integers (0..40) with a bright band; every frame is roll(ref, t) plus integer noise; the coarse index is the
    nearest index of the 12x20 grid.  -> (rasters, ref, coarse indices, true shifts t, (D_y, D_x))"""
    y_t, x_t, grid = DISP["y_t"], DISP["x_t"], DISP["grid"]
    rng = np.random.default_rng(100 + 7 * seed + sigma)
    ref = rng.integers(0, 11, (y_t, x_t)).astype(np.float32)
    ref[:, 30:41] += 30.0          # a bright vertical band
    ref[9:14, :] += 25.0           # and a horizontal one
    ref = np.asfortranarray(ref)
    ts = np.stack([rng.integers(0, y_t, trials), rng.integers(0, x_t, trials)], axis=1)
    rasters = []
    for ty, tx in ts:
        noise = np.round(rng.normal(0.0, sigma, (y_t, x_t))) if sigma else 0.0
        rasters.append(np.asfortranarray((np.roll(ref, (ty, tx), axis=(0, 1)) + noise).astype(np.float32)))
    idx = np.stack([np.round(ts[:, 0] * grid[0] / y_t), np.round(ts[:, 1] * grid[1] / x_t)], axis=1).astype(np.int32)
    D = (-(-y_t // grid[0]), -(-x_t // grid[1]))     # k = 1: one grid cell
    return rasters, ref, idx, ts, D


@pytest.mark.parametrize("sigma", DISP["sigmas"])
def test_known_displacement_is_recovered_exactly(sigma):
    rasters, ref, idx, ts, D = displacement_case(sigma)
    y_t, x_t, grid = DISP["y_t"], DISP["x_t"], DISP["grid"]
    out, _, _ = R.register(rasters, ref, D[0], D[1], [tuple(map(int, r)) for r in idx], "image", grid)
    assert np.array_equal(out, ts % [y_t, x_t]), (sigma, out.tolist(), ts.tolist())
    coarse = np.array([R.coarse(idx, f, y_t, x_t, "image", grid) for f in range(len(rasters))])
    off = np.abs((coarse - ts + [y_t // 2, x_t // 2]) % [y_t, x_t] - [y_t // 2, x_t // 2])
    assert off.max() >= 2 and off[:, 1].max() <= 4, "the nearest grid index alone is pixels off, within half a cell"


# ---------------------------------------------------------------- sharpening, on the CPU oracle's rasters
# 3 raster pixels per grid column; S = round(Fs/fv) = 49917 against 49916.8: the picture drifts 1.4 pixels per frame
GEOMS = {"150x2400": dict(Fs=3.0e6, x_t=2400, y_t=150, fv=60.1, nfr=6, extra=555),
         "628x1056": dict(Fs=2.0e6, x_t=1056, y_t=628, fv=60.0, nfr=3, extra=777)}   # (of tests/test_hires_gpu.py)
ALPHA, ALPHA_H = np.float32(0.1), np.float32(0.1)


@functools.lru_cache(maxsize=None)
def capture(name):
    from tempest_loader import load_package
    load_package()
    synth = importlib.import_module("tempestsdr_jl_amd.synth")
    g = GEOMS[name]
    S = synth.samples_per_frame(g["Fs"], g["fv"])
    iq = synth.synth_leak(g["Fs"], g["x_t"], g["y_t"], g["fv"], S * g["nfr"] + g["extra"])
    iq.setflags(write=False)
    return iq, S


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the CPU oracle's rasters, sync indices, 600x800 frames and state of a capture"""
    g = GEOMS[name]
    iq, S = capture(name)
    st = np.zeros(GRID, np.float32, order="F")
    o = O.frames(O.SyncXY(*GRID), iq, S, g["y_t"], g["x_t"], ALPHA, st, want_raster=True)
    assert o["n_frames"] == g["nfr"]
    assert all(float(r.min()) > 0.0 for r in o["raster"]), "the FAST tolerance is relative: the rasters must be strictly positive"
    return dict(raster=o["raster"], frames=o["frames"], state=st, sync_idx=np.asarray(o["sync_idx"], np.int32))


def residual(rasters, shifts, state):
    """mean squared distance between each aligned raster and the state"""
    st = np.asarray(state, np.float64)
    return float(np.mean([np.mean((np.roll(np.asarray(r, np.float64), (-int(s[0]), -int(s[1])), axis=(0, 1)) - st) ** 2)
                          for r, s in zip(rasters, shifts)]))


def test_refinement_sharpens_the_average_on_the_oracle_rasters():
    name = "150x2400"
    g, o = GEOMS[name], oracle(name)
    zero = np.zeros((g["y_t"], g["x_t"]), np.float32, order="F")
    st_c, sh_c, _, _ = R.refined_loop(o["raster"], o["sync_idx"], zero, ALPHA_H, 1, refine=False)
    st_r, sh_r, scores, (d_y, d_x) = R.refined_loop(o["raster"], o["sync_idx"], zero, ALPHA_H, 1)
    assert (d_y, d_x) == (1, 3)
    assert np.any(sh_c != sh_r), "at least one frame's refined shift differs from its coarse one"
    res_c, res_r = residual(o["raster"], sh_c, st_c), residual(o["raster"], sh_r, st_r)
    print(f"{name}: residual coarse {res_c:.6e}, refined {res_r:.6e}, ratio {res_r / res_c:.4f}; shifts coarse {sh_c.tolist()} refined {sh_r.tolist()}")
    assert res_r < res_c
    # every choice is clear of rounding: the GPU loop (any summation order, TSDR_FAST rasters) must reproduce the shifts
    for chunk in (0, 1, 2):
        for nm in GEOMS:
            gg, oo = GEOMS[nm], oracle(nm)
            z = np.zeros((gg["y_t"], gg["x_t"]), np.float32, order="F")
            _, _, sc, (dy, dx) = R.refined_loop(oo["raster"], oo["sync_idx"], z, ALPHA_H, 1, chunk=chunk)
            m = np.concatenate([R.margins(s, dy, dx) for s in sc])
            print(f"{nm} chunk {chunk}: smallest top-2 margin {m.min():.3e}")
            assert m.min() > 1e-9, (nm, chunk, m.tolist())
