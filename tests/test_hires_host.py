"""Host-side checks of the full-resolution frame average (no GPU): include/tempest_hip_hires.h, its ctypes table
(_lib._SIGS_HIRES), its Python module (hires.py) and its Julia shim (julia/TempestHIP_hires.jl) agree with each other and with the
library, the way test_autocorr_complex_host.py pins tempest_hip_cplx.h; the shift rule of the contract and the numpy reference
the GPU tests compare against (tests/hires_ref.py) are checked against their definitions."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import hires_ref as R
import test_dptr_host as DH
import test_julia_shim_static as JS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN_H = os.path.join(ROOT, "include", "tempest_hip.h")
HIRES_H = os.path.join(ROOT, "include", "tempest_hip_hires.h")
SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP.jl")
HIRES_SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP_hires.jl")
KERNEL = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "raster_accum.hip")

SYMS = sorted(["tsdr_raster_accum", "tsdr_raster_accum_d", "tsdr_frames_hires_iq_d"])
ACCUM = ["tsdr_ctx *ctx", "const float *rasters", "int n_frames", "int y_t", "int x_t", "const int *shifts", "int shift_units",
         "int img_h", "int img_w", "float alpha", "float *state"]


def _pkg(name):
    from tempest_loader import load_package
    load_package()
    return importlib.import_module("tempestsdr_jl_amd." + name)


def _strip(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return re.sub(r"^#.*$", "", src, flags=re.M)


def _protos(path=HIRES_H):
    out = {}
    for m in re.finditer(r"\bint\s+(tsdr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _strip(path), flags=re.S):
        out[m.group(1)] = [" ".join(p.split()) for p in m.group(2).split(",")]
    return out


# ---------------------------------------------------------------- header, table, library, shims
def test_header_declares_the_three_forms():
    p = _protos()
    assert sorted(p) == SYMS
    assert p["tsdr_raster_accum"] == p["tsdr_raster_accum_d"] == ACCUM
    # the whole loop: tsdr_frames_iq_d's list with raster_out replaced by (alpha_hires, hires_state)
    loop = _protos(MAIN_H)["tsdr_frames_iq_d"]
    k = loop.index("float *raster_out")
    assert p["tsdr_frames_hires_iq_d"] == loop[:k] + ["float alpha_hires", "float *hires_state"] + loop[k + 1:]
    code = _strip(HIRES_H)
    assert re.search(r"enum\s*\{\s*TSDR_SHIFT_RASTER\s*=\s*0\s*,\s*TSDR_SHIFT_IMAGE\s*=\s*1\s*\}\s*;", code)


def test_main_header_includes_it_once_and_declares_none_of_it():
    main = open(MAIN_H).read()
    assert main.count('#include "tempest_hip_hires.h"') == 1
    assert main.index('#include "tempest_hip_hires.h"') > main.index("enum { TSDR_IQ_CF32"), "after the TSDR_IQ_* enum"
    assert main.index('#include "tempest_hip_hires.h"') > main.index("typedef struct tsdr_sync"), "the loop's prototype uses tsdr_sync"
    code = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert not re.search(r"raster_accum|frames_hires|TSDR_SHIFT_", code), "the new names live in the new header only"
    guard = open(HIRES_H).read()
    assert "#ifndef TEMPEST_HIP_HIRES_H" in guard and '#error "include tempest_hip.h' in guard


def test_header_states_the_contract():
    src = " ".join(open(HIRES_H).read().split())
    for phrase in ("SEMANTICS", "SHIFT UNITS", "EDGE CASES", "COST", "THE WHOLE LOOP", "GUI.jl:172,175", "NO FMA", "FLOORED",
                   "floor((2*a*y_t + img_h) / (2*img_h)) mod y_t", "64-bit", "n_frames == 0", "P >= 2^31", "TSDR_EINVAL",
                   "nothing written", "never written", "n_frames*4P + 8P", "hires_chunk_frames", "k*4P bytes", "one chunk", "TSDR_FAST",
                   "NOT bit identity", "NaN / Inf propagate"):
        assert phrase in src, phrase


def test_header_table_and_library_agree():
    lib = _pkg("_lib")
    assert sorted(_protos()) == SYMS == lib.exported_names_hires()
    for other in (lib._SIGS, lib._SIGS_IQ, lib._SIGS_CPLX):
        assert not set(other) & set(lib._SIGS_HIRES)
    assert (lib.SHIFT_RASTER, lib.SHIFT_IMAGE) == (0, 1)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    for sym in SYMS:
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_hires.h but not exported"
        assert getattr(bound, sym).restype is C.c_int and getattr(bound, sym).argtypes == lib._SIGS_HIRES[sym][1], sym


def test_table_argtypes_match_the_prototypes():
    lib = _pkg("_lib")
    ct = {"i32": C.c_int, "i64": C.c_size_t, "f32": C.c_float, "f64": C.c_double}
    for sym, params in _protos().items():
        res, args = lib._SIGS_HIRES[sym]
        assert res is C.c_int and len(args) == len(params), sym
        for k, (a, p) in enumerate(zip(args, params)):
            cls = JS.c_class(p)
            if cls == "ptr":
                assert a is C.c_void_p or (isinstance(a, type) and issubclass(a, C._Pointer)), (sym, k, p, a)
                if a is not C.c_void_p:   # a typed pointer points to what the prototype says
                    want = {"int": C.c_int, "float": C.c_float}[re.sub(r"\bconst\b", "", p).split()[0]]
                    assert a._type_ is want, (sym, k, p, a)
            else:
                assert a is ct[cls], (sym, k, p, a)


def test_every_ccall_of_the_hires_shim_matches_its_prototype():
    """as test_julia_shim_static.py, for julia/TempestHIP_hires.jl against the new header (the main shim may only name symbols of
    tempest_hip.h, hence the separate file)"""
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(tsdr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _strip(HIRES_H), flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        protos[name] = ("ptr" if "*" in ret else JS.c_class(ret + " x"), [JS.c_class(p) for p in JS.split_args(args)])
    assert sorted(protos) == SYMS and not set(protos) & set(JS.header_protos())
    jl = open(HIRES_SHIM).read()
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
    assert seen == set(SYMS)


def test_shim_has_the_two_functions():
    main = open(SHIM).read()
    assert main.count('include("TempestHIP_hires.jl")') == 1
    assert main.index('include("TempestHIP_hires.jl")') > main.index('include("TempestHIP_cplx.jl")')
    code = "\n".join(line for line in main.splitlines() if not line.lstrip().startswith("#"))
    assert "tsdr_raster_accum" not in code and "tsdr_frames_hires" not in code
    jl = open(HIRES_SHIM).read()
    m = re.search(r"\nfunction hip_raster_accumulate!\(state::Matrix\{Float32\}, rasters::Array\{Float32,3\}, α::Float32;(.*?)\nend", jl, flags=re.S)
    assert m and "ccall((:tsdr_raster_accum, LIB)" in m.group(1) and "SHIFT_UNITS[units]" in m.group(1)
    m = re.search(r"\nfunction hip_frames_hires!\((.*?)\nend", jl, flags=re.S)
    assert m and "ccall((:tsdr_frames_hires_iq_d, LIB)" in m.group(1) and "IQ_FORMATS[fmt]" in m.group(1)


def test_python_interface_and_delegation():
    api, mod = _pkg("api"), _pkg("hires")
    p = inspect.signature(api.Context.raster_accumulate).parameters
    assert list(p) == ["self", "rasters", "state", "alpha", "shifts", "units", "grid"]
    assert (p["shifts"].default, p["units"].default, p["grid"].default) == (None, "raster", (600, 800))
    p = inspect.signature(api.Context.frames_hires).parameters
    assert list(p)[:11] == ["self", "sync", "iq", "S", "y_t", "x_t", "alpha", "imageOut", "alpha_hires", "hires_state", "iq_fmt"]
    assert p["iq_fmt"].default is None
    assert hasattr(api.Context, "raster_accumulate_d") and hasattr(api.Context, "frames_hires_d")
    # every call of the new symbols is in the new module; api.py calls none of them itself
    called = DH.called_symbols(open(mod.__file__).read())
    assert set(SYMS) <= called
    src = open(api.__file__).read()
    assert not (DH.called_symbols(src) & set(SYMS))
    assert not any("hires" in s or "raster_accum" in s for syms in DH.api_wrappers().values() for s in syms)
    with pytest.raises(AssertionError):
        mod._units("pixels")


def test_every_new_entry_point_is_called_by_the_gpu_suite():
    text = open(os.path.join(ROOT, "tests", "test_hires_gpu.py")).read()
    called = DH.called_symbols(text)
    missing = [s for s in SYMS if s not in called]
    assert not missing, missing
    assert "import dptr_util as D" in text and "D.Arenas(" in text and "pytestmark = pytest.mark.gpu" in text


def test_kernel_source_keeps_its_launch_rules():
    """an exact, uncapped grid under the profile name "raster_accum"; the capped-grid helpers (which tests/test_grid_cap_host.py
    tracks through tests/grid_cap_cases.py) are not used"""
    src = open(KERNEL).read()
    assert "stream_grid(" not in src and "stream_blocks(" not in src
    assert src.count('TSDR_LAUNCH(ctx, "raster_accum"') == 2 and "ceil_div(" in src
    assert frames_in_flight() >= 2
    assert all(op in src for op in ("__fsub_rn(1.0f, alpha)", "__fmul_rn(alpha, acc)", "__fmul_rn(oma, v", "__fadd_rn("))


def frames_in_flight():
    """U: the frames whose loads one lane of k_raster_accum issues back to back (test_hires_gpu.py walks n around its multiples)"""
    m = re.search(r"constexpr int kRasterAccumU = (\d+);", open(KERNEL).read())
    assert m, "kRasterAccumU not found in raster_accum.hip"
    return int(m.group(1))


def test_option_is_known_and_build_tracks_the_header():
    assert '"hires_chunk_frames"' in open(os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "ctx.hip")).read()
    assert '"tempest_hip_hires.h"' in open(os.path.join(ROOT, "tempestsdr.jl_amd", "build.py")).read()


# ---------------------------------------------------------------- the shift rule
@pytest.mark.parametrize("H,y_t", [(600, 125), (600, 628), (600, 1125), (7, 3)])
def test_image_shift_rule(H, y_t):
    a = np.arange(-2 * H, 2 * H + 1, dtype=np.int64)
    u = np.array([int(R.unreduced(int(v), y_t, "image", H)) for v in a], np.int64)
    r = np.array([R.resolve(int(v), y_t, "image", H) for v in a], np.int64)
    assert R.unreduced(0, y_t, "image", H) == 0 and R.resolve(0, y_t, "image", H) == 0
    for k in (-2, -1, 1, 2):
        assert R.unreduced(k * H, y_t, "image", H) == k * y_t and R.resolve(k * H, y_t, "image", H) == 0   # r(H) = 0 mod y_t
    # |r - a*y_t/H| <= 1/2 before the reduction, in exact integers: |2*H*u - 2*a*y_t| <= H
    assert np.all(np.abs(2 * H * u - 2 * a * y_t) <= H)
    # round half UP: an exact half goes to the larger integer
    half = (2 * a * y_t) % (2 * H) == H
    assert np.all(2 * H * u[half] - 2 * a[half] * y_t == H)
    assert np.all(np.diff(u) >= 0), "monotone"
    assert np.all((r >= 0) & (r < y_t)) and np.array_equal(r, np.mod(u, y_t))
    # Python's unbounded integers agree (floored // and %)
    assert [int(v) for v in r] == [((2 * int(v) * y_t + H) // (2 * H)) % y_t for v in a]


def test_raster_shift_rule_and_int_extremes():
    for size in (1, 3, 125, 1125):
        for a in (-2 * size - 1, -size, -1, 0, 1, size - 1, size, 2 * size + 1, -2 ** 31, 2 ** 31 - 1):
            assert R.resolve(a, size, "raster") == a % size
    # the image rule stays inside int64 for every int a and every size, img below 2^31
    for a in (-2 ** 31, 2 ** 31 - 1):
        for size, img in ((2 ** 31 - 1, 1), (2 ** 31 - 1, 2 ** 31 - 1), (1125, 600)):
            assert R.resolve(a, size, "image", img) == ((2 * a * size + img) // (2 * img)) % size


def test_reference_equals_the_brute_force_loop():
    rng = np.random.default_rng(5)
    y_t, x_t, n = 7, 5, 3
    rasters = [np.asfortranarray(rng.standard_normal((y_t, x_t)).astype(np.float32)) for _ in range(n)]
    state = np.asfortranarray(rng.standard_normal((y_t, x_t)).astype(np.float32))
    keep = [r.copy() for r in rasters], state.copy()
    cases = [(None, "raster", (600, 800)), ([(0, 0)] * n, "raster", (600, 800)), ([(6, 4), (-1, -9), (7, 12)], "raster", (600, 800)),
             ([(1, 1), (599, 799), (-300, 1000)], "image", (600, 800)), ([(3, 2), (7, 5), (-1, 0)], "image", (7, 5))]
    for shifts, units, grid in cases:
        for alpha in (0.0, 1.0, 0.1, 0.95):
            got = R.accumulate(rasters, state, alpha, shifts, units, grid)
            want = R.brute(rasters, state, alpha, shifts, units, grid)
            assert got.dtype == np.float32 and got.flags.f_contiguous
            assert np.array_equal(got.view(np.uint32), np.asfortranarray(want).view(np.uint32)), (shifts, units, alpha)
    assert all(np.array_equal(a, b) for a, b in zip(rasters, keep[0])) and np.array_equal(state, keep[1]), "inputs unchanged"
    # a shift really moves the picture: frame 0 alone, alpha = 0, shift (2, 1) in raster units
    one = R.accumulate(rasters[:1], state, 0.0, [(2, 1)], "raster")
    assert one[0, 0] == rasters[0][2, 1] and one[y_t - 1, x_t - 1] == rasters[0][1, 0]
