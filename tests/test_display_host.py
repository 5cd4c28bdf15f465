"""Host-side checks of the display export (no GPU): include/tempest_hip_display.h, its ctypes table (_lib._SIGS_DISPLAY), its Python
module (display.py) and its Julia shim (julia/TempestHIP_display.jl) agree with each other and with the library, the way
test_register_host.py pins tempest_hip_register.h; the numpy reference the GPU tests compare against (tests/display_ref.py) is
checked on answers known without it."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import display_ref as R
import test_dptr_host as DH
import test_hires_host as HH
import test_julia_shim_static as JS

ROOT = HH.ROOT
MAIN_H = HH.MAIN_H
DISP_H = os.path.join(ROOT, "include", "tempest_hip_display.h")
DISP_SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP_display.jl")
KERNEL = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "display.hip")

SYMS = ["tsdr_display_u8", "tsdr_display_u8_d"]
PROTO = ["tsdr_ctx *ctx", "const float *images", "int n_images", "int h", "int w", "int i0", "int j0", "int rh", "int rw", "int range_mode",
         "float lo", "float hi", "double p_lo", "double p_hi", "int flags", "uint8_t *out", "float *ranges_out"]
F = np.float32


# ---------------------------------------------------------------- header, table, library, shims
def test_header_declares_the_two_forms_and_the_constants():
    p = HH._protos(DISP_H)
    assert sorted(p) == SYMS
    assert p["tsdr_display_u8"] == p["tsdr_display_u8_d"] == PROTO
    code = HH._strip(DISP_H)
    assert re.search(r"enum\s*\{\s*TSDR_RANGE_FIXED\s*=\s*0\s*,\s*TSDR_RANGE_MINMAX\s*=\s*1\s*,\s*TSDR_RANGE_PERCENTILE\s*=\s*2\s*\}\s*;", code)
    assert re.search(r"enum\s*\{\s*TSDR_DISPLAY_INVERT\s*=\s*1\s*,\s*TSDR_DISPLAY_SHARED\s*=\s*2\s*\}\s*;", code)
    assert re.search(r"^#define TSDR_DISPLAY_BINS 4096$", open(DISP_H).read(), flags=re.M)
    lib = HH._pkg("_lib")
    assert (lib.RANGE_FIXED, lib.RANGE_MINMAX, lib.RANGE_PERCENTILE, lib.DISPLAY_INVERT, lib.DISPLAY_SHARED, lib.DISPLAY_BINS) == (0, 1, 2, 1, 2, 4096)
    assert (R.FIXED, R.MINMAX, R.PERCENTILE, R.INVERT, R.SHARED, R.B) == (0, 1, 2, 1, 2, 4096)


def test_main_header_includes_it_once_after_the_register_header():
    main = open(MAIN_H).read()
    assert main.count('#include "tempest_hip_display.h"') == 1
    assert main.index('#include "tempest_hip_display.h"') > main.index('#include "tempest_hip_register.h"')
    for path in (MAIN_H, HH.HIRES_H, os.path.join(ROOT, "include", "tempest_hip_register.h")):
        assert not re.search(r"display_u8|TSDR_RANGE_|TSDR_DISPLAY_", HH._strip(path)), path
    guard = open(DISP_H).read()
    assert "#ifndef TEMPEST_HIP_DISPLAY_H" in guard and "#ifndef TEMPEST_HIP_REGISTER_H\n#error" in guard


def test_header_states_the_contract():
    src = " ".join(open(DISP_H).read().split())
    for phrase in ("INPUT", "ROI", "OUTPUT", "GROUP", "RANGE", "MAPPING", "REFUSALS", "REPEATABILITY", "STATE", "COST", "NO WRAP", "NO FMA",
                   "ANY byte alignment", "fullScale!", "ScreenRenderer.jl:35-39", "FINITE", "N == 0: mn = mx = 0",
                   "invw = fdiv((float)B, d)", "min(B-1, (int)floorf(fmul(fsub(v, mn), invw)))", "k_lo = floor(p_lo*(N-1))",
                   "k_hi = ceil(p_hi*(N-1))", "b_lo = the smallest b with cum(b) > k_lo","b == B ? mx : fadd(mn, fmul((float)b, wd))",
                   "hi = edge(b_hi + 1)", "p = (0, 1) gives exactly (mn, mx)", "s = fdiv(255.0f, dd)", "EVERY byte of the group is 0",
                   "round half to even", "255 - q", "A NaN pixel is 0 either way", "n_images == 0 is TSDR_OK", "nothing written",
                   "h*w >= 2^31", "0 <= p_lo <= p_hi <= 1", "not 4-byte aligned", "never written", "no floating-point atomics",
                   "ON THE STREAM BY EVERY CALL", "reads 4*R, writes R", "reads 8*R, writes R", "reads 12*R, writes R", '"wait_ms"'):
        assert phrase in src, phrase


def test_header_table_and_library_agree():
    lib = HH._pkg("_lib")
    assert sorted(HH._protos(DISP_H)) == SYMS == lib.exported_names_display()
    for other in (lib._SIGS, lib._SIGS_IQ, lib._SIGS_CPLX, lib._SIGS_HIRES, lib._SIGS_REGISTER):
        assert not set(other) & set(lib._SIGS_DISPLAY)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    for sym in SYMS:
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_display.h but not exported"
        assert getattr(bound, sym).restype is C.c_int and getattr(bound, sym).argtypes == lib._SIGS_DISPLAY[sym][1], sym


def test_table_argtypes_match_the_prototypes():
    lib = HH._pkg("_lib")
    ct = {"i32": C.c_int, "i64": C.c_size_t, "f32": C.c_float, "f64": C.c_double}
    for sym, params in HH._protos(DISP_H).items():
        res, args = lib._SIGS_DISPLAY[sym]
        assert res is C.c_int and len(args) == len(params) == 17, sym
        for k, (a, p) in enumerate(zip(args, params)):
            cls = JS.c_class(p)
            assert (a is C.c_void_p) if cls == "ptr" else (a is ct[cls]), (sym, k, p, a)


def test_every_ccall_of_the_display_shim_matches_its_prototype():
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(tsdr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", HH._strip(DISP_H), flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        protos[name] = ("ptr" if "*" in ret else JS.c_class(ret + " x"), [JS.c_class(p) for p in JS.split_args(args)])
    assert sorted(protos) == SYMS and not set(protos) & set(JS.header_protos())
    jl = open(DISP_SHIM).read()
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
    assert seen == set(SYMS), "hip_display_u8! binds the host form, hip_display_u8_d! the device form"


def test_shim_is_included_after_the_register_shim_and_the_main_shim_names_nothing():
    main = open(HH.SHIM).read()
    assert main.count('include("TempestHIP_display.jl")') == 1
    assert main.index('include("TempestHIP_display.jl")') > main.index('include("TempestHIP_register.jl")')
    code = "\n".join(line for line in main.splitlines() if not line.lstrip().startswith("#"))
    assert "tsdr_display_u8" not in code
    jl = open(DISP_SHIM).read()
    assert re.search(r"\nfunction hip_display_u8!\(out::Array\{UInt8,3\}, images::Array\{Float32,3\};", jl)
    assert re.search(r"\nfunction hip_display_u8_d!\(d_out::Ptr\{Cvoid\}, d_images::Ptr\{Cvoid\},", jl)
    assert "Dict(:fixed => 0, :minmax => 1, :percentile => 2)" in jl and "(invert ? 1 : 0) | (shared ? 2 : 0)" in jl


def test_python_interface_and_delegation():
    api, mod = HH._pkg("api"), HH._pkg("display")
    p = inspect.signature(api.Context.display_u8).parameters
    assert list(p) == ["self", "images", "roi", "mode", "lo", "hi", "p", "invert", "shared"]
    assert (p["roi"].default, p["mode"].default, p["invert"].default, p["shared"].default) == (None, "minmax", False, False)
    p = inspect.signature(api.Context.display_u8_d).parameters
    assert list(p) == ["self", "images", "n_images", "h", "w", "out", "roi", "mode", "lo", "hi", "p", "invert", "shared", "ranges_out"]
    called = DH.called_symbols(open(mod.__file__).read())
    assert set(SYMS) <= called
    assert not (DH.called_symbols(open(api.__file__).read()) & set(SYMS)), "api.py delegates; it calls none of the symbols itself"
    assert not any("display" in s for syms in DH.api_wrappers().values() for s in syms)
    assert mod.MODES == {"fixed": 0, "minmax": 1, "percentile": 2}
    import tempestsdr_jl_amd as T
    assert T.display_u8 is mod.display_u8 and T.display_u8_d is mod.display_u8_d


def test_every_new_entry_point_is_called_by_the_gpu_suite():
    text = open(os.path.join(ROOT, "tests", "test_display_gpu.py")).read()
    called = DH.called_symbols(text)
    assert set(SYMS) <= called, sorted(set(SYMS) - called)
    assert "import dptr_util as D" in text and "D.Arenas(" in text and "pytestmark = pytest.mark.gpu" in text


def test_kernel_source_keeps_its_launch_rules():
    src = open(KERNEL).read()
    code = re.sub(r"//.*", "", src)
    assert "stream_grid(" not in code and "stream_blocks(" not in code and "ceil_div(" in code, "exact grids"
    for name in ("display_stats", "display_hist", "display_pick", "display_map"):
        assert f'TSDR_LAUNCH(ctx, "{name}"' in src, name
    # integer atomics only: every atomic's operand is an integer word (keys, counts, counters, bin indices)
    assert len(re.findall(r"\batomic(Add|Max|Min)\(", code)) >= 6 and not re.search(r"atomic\w*\([^;]*float", code)
    assert "hipMemsetAsync(gs, 0, bytes" in code, "the scratch is cleared on the stream by every call"
    assert "__fmul_rn(__fsub_rn(v, lo), s)" in code and "__fdiv_rn(255.0f, dd)" in code, "separately rounded, as the contract states"


def test_workspace_and_build_know_the_feature():
    common = open(os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "common.h")).read()
    slots = re.search(r"enum Slot \{(.*?)\}", common, flags=re.S).group(1)
    assert re.search(r"^\s*WS_DISPLAY\b", slots, flags=re.M)
    build = open(os.path.join(ROOT, "tempestsdr.jl_amd", "build.py")).read()
    assert '"tempest_hip_display.h"' in build and '"tempest_hip_register.h"' in build
    assert os.path.exists(KERNEL), "picked up by build.py's directory scan"


# ---------------------------------------------------------------- the reference's own known answers
def _pic(seed=1, shape=(9, 14)):
    return np.asfortranarray(np.random.default_rng(seed).normal(3.0, 2.0, shape).astype(F))


def test_minmax_is_full_scale_times_255_rounded():
    for seed in range(4):
        img = _pic(seed)
        out, rng = R.display([img], mode=R.MINMAX)
        assert np.array_equal(out[0], R.full_scale_255(img))
        assert rng[0, 0] == img.min() and rng[0, 1] == img.max()
        assert out[0].min() == 0 and out[0].max() == 255
        # within one level of the reference's own order, (v - min) / (max - min) * 255 in f64
        exact = (img.astype(np.float64) - float(img.min())) / (float(img.max()) - float(img.min())) * 255.0
        assert np.max(np.abs(out[0].astype(np.float64) - exact)) <= 0.5 + 1e-3


def test_percentile_zero_one_is_minmax():
    for seed in range(4):
        img = _pic(seed, (31, 17))
        a, ra = R.display([img], mode=R.PERCENTILE, p=(0.0, 1.0))
        b, rb = R.display([img], mode=R.MINMAX)
        assert np.array_equal(a, b) and np.array_equal(ra, rb)


def test_ramp_of_integers_has_the_edges_one_expects():
    """0 .. 4095 repeated k times, shuffled: N = 4096 k, the order statistic of rank r is the integer r // k.  The edges are bin
    edges mn + b * wd (wd = 4095/4096, mn = 0) that bracket the order statistics of ranks k_lo and k_hi within one bin width;
    p = (0, 1) gives exactly (0, 4095); every bin holds k or 2k values (4096 integers over a span of 4095 bin widths... of
    4095/4096: exactly one pair of neighbours shares a bin)."""
    wd = F(4095) / F(4096)
    for k in (1, 3):
        v = np.tile(np.arange(4096, dtype=F), k)
        img = np.asfortranarray(np.random.default_rng(k).permutation(v).reshape(64, 64 * k))
        counts = np.bincount(R.bins(img, F(0), F(4096) / F(4095)), minlength=4096)
        assert counts.sum() == 4096 * k and sorted(set(counts.tolist())) == [0, k, 2 * k] and (counts == 2 * k).sum() == 1
        N = v.size
        assert R.group_range(img, R.PERCENTILE, p=(0.0, 1.0)) == (F(0), F(4095))
        for p in ((0.02, 0.98), (0.5, 0.5), (0.0, 1.0), (0.25, 0.25), (0.001, 0.999)):
            lo, hi = R.group_range(img, R.PERCENTILE, p=p)
            v_lo, v_hi = int(np.floor(p[0] * (N - 1))) // k, int(np.ceil(p[1] * (N - 1))) // k
            assert lo <= v_lo < float(lo) + 2 * float(wd), (k, p, lo, v_lo)
            assert float(hi) - 2 * float(wd) < v_hi <= hi, (k, p, hi, v_hi)
            assert lo == F(round(float(lo) / float(wd))) * wd and (hi == F(4095) or hi == F(round(float(hi) / float(wd))) * wd), "bin edges"
            assert lo < hi


def test_degenerate_pictures_give_zeros():
    nan = np.full((5, 7), np.nan, F)
    const = np.full((5, 7), 2.5, F)
    inf = np.full((5, 7), np.inf, F)
    for img in (nan, const, inf):
        for mode in (R.MINMAX, R.PERCENTILE):
            for inv in (False, True):
                out, rng = R.display([img], mode=mode, p=(0.1, 0.9), invert=inv)
                assert not out.any(), (mode, inv)
    assert np.array_equal(R.display([nan], mode=R.MINMAX)[1], [[0, 0]]) and np.array_equal(R.display([const], mode=R.MINMAX)[1], [[2.5, 2.5]])
    # FIXED with hi <= lo, or an infinite bound: zeros as well
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (-np.inf, 1.0), (0.0, np.inf)):
        assert not R.display([_pic()], mode=R.FIXED, lo=lo, hi=hi)[0].any()


def test_invert_nan_inf_and_rounding():
    img = np.asfortranarray(np.array([[0.0, 1.0, 2.0, 3.0], [np.nan, np.inf, -np.inf, 255.0]], F))
    out, rng = R.display([img], mode=R.FIXED, lo=0.0, hi=255.0)
    assert out[0].tolist() == [[0, 1, 2, 3], [0, 255, 0, 255]] and rng.tolist() == [[0.0, 255.0]]
    inv, _ = R.display([img], mode=R.FIXED, lo=0.0, hi=255.0, invert=True)
    assert inv[0].tolist() == [[255, 254, 253, 252], [0, 0, 255, 0]], "255 - q, a NaN pixel 0 either way"
    # halves round to even: s = 255 / 510 = 0.5
    half = np.asfortranarray(np.array([[1.0, 3.0, 5.0, 7.0]], F))
    assert R.display([half], mode=R.FIXED, lo=0.0, hi=510.0)[0][0].tolist() == [[0, 2, 2, 4]]
    # the infinities never enter the statistics
    assert R.display([img], mode=R.MINMAX)[1].tolist() == [[0.0, 255.0]]
    x = _pic(5)
    a, _ = R.display([x], mode=R.PERCENTILE, p=(0.05, 0.95))
    b, _ = R.display([x], mode=R.PERCENTILE, p=(0.05, 0.95), invert=True)
    assert np.array_equal(b, 255 - a)


def test_roi_and_shared_groups():
    imgs = [_pic(s, (12, 10)) * F(s + 1) for s in range(3)]
    roi = (2, 3, 7, 4)
    out, rng = R.display(imgs, roi, R.MINMAX)
    for f, m in enumerate(imgs):
        c = m[2:9, 3:7]
        assert out.shape == (3, 7, 4) and rng[f].tolist() == [c.min(), c.max()]
    out, rng = R.display(imgs, roi, R.MINMAX, shared=True)
    allc = np.stack([m[2:9, 3:7] for m in imgs])
    assert np.all(rng == [allc.min(), allc.max()])
    lo, hi = R.group_range(allc, R.PERCENTILE, p=(0.1, 0.9))
    _, rng = R.display(imgs, roi, R.PERCENTILE, p=(0.1, 0.9), shared=True)
    assert np.all(rng == [lo, hi]) and allc.min() <= lo < hi <= allc.max()
