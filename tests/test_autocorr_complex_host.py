"""Host-side checks of calculate_autocorrelation on complex input (no GPU): include/tempest_hip_cplx.h, its ctypes table
(_lib._SIGS_CPLX), its Python module (autocorr_cplx.py) and its Julia shim (julia/TempestHIP_cplx.jl) agree with each other and
with the library, the way test_abi.py, test_iq_spectra_host.py, test_julia_shim_static.py and test_dptr_host.py pin the other two
headers."""
import ctypes as C
import importlib
import inspect
import os
import re

import test_dptr_host as DH
import test_julia_shim_static as JS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN_H = os.path.join(ROOT, "include", "tempest_hip.h")
CPLX_H = os.path.join(ROOT, "include", "tempest_hip_cplx.h")
SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP.jl")
CPLX_SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP_cplx.jl")

SYMS = sorted(["tsdr_autocorr_cplx", "tsdr_autocorr_cplx_d", "tsdr_autocorr_cplx_iq", "tsdr_autocorr_cplx_search_iq_d",
               "tsdr_autocorr_cplx_f64", "tsdr_autocorr_cplx_f64_d"])
TAIL = ["size_t len", "double Fs", "double minDelay", "double maxDelay", "int log_scale"]
IQ_HEAD = ["tsdr_ctx *ctx", "const void *iq", "int iq_fmt", "float scale"]


def _pkg(name):
    from tempest_loader import load_package
    load_package()
    return importlib.import_module("tempestsdr_jl_amd." + name)


def _strip(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return re.sub(r"^#.*$", "", src, flags=re.M)


def _protos():
    out = {}
    for m in re.finditer(r"\bint\s+(tsdr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _strip(CPLX_H), flags=re.S):
        out[m.group(1)] = [" ".join(p.split()) for p in m.group(2).split(",")]
    return out


def test_header_declares_the_six_forms():
    p = _protos()
    assert sorted(p) == SYMS
    f32 = ["float *out", "size_t *n_out"]
    assert p["tsdr_autocorr_cplx"] == p["tsdr_autocorr_cplx_d"] == ["tsdr_ctx *ctx", "const float *z"] + TAIL + f32
    assert p["tsdr_autocorr_cplx_f64"] == p["tsdr_autocorr_cplx_f64_d"] == ["tsdr_ctx *ctx", "const double *z"] + TAIL + ["double *out", "size_t *n_out"]
    assert p["tsdr_autocorr_cplx_iq"] == IQ_HEAD + TAIL + f32
    assert p["tsdr_autocorr_cplx_search_iq_d"] == IQ_HEAD + TAIL + f32 + ["size_t win_lo", "size_t win_cnt", "size_t *idx", "float *val"]
    # the search twin has the argument list of the power search it mirrors
    main = re.sub(r"/\*.*?\*/", "", open(MAIN_H).read(), flags=re.S)
    m = re.search(r"\bint\s+tsdr_autocorr_search_iq_d\s*\(([^;{]*?)\)\s*;", main, flags=re.S)
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == p["tsdr_autocorr_cplx_search_iq_d"]


def test_main_header_includes_it_once_and_declares_none_of_it():
    main = open(MAIN_H).read()
    assert main.count('#include "tempest_hip_cplx.h"') == 1
    assert main.index('#include "tempest_hip_cplx.h"') > main.index("enum { TSDR_IQ_CF32"), "the prototypes use TSDR_IQ_*"
    code = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert not re.search(r"tsdr_autocorr_cplx", code), "the new symbols live in the new header only (test_abi.py, test_dptr_host.py)"
    guard = open(CPLX_H).read()
    assert "#ifndef TEMPEST_HIP_CPLX_H" in guard and '#error "include tempest_hip.h' in guard


def test_header_states_the_contract():
    src = " ".join(open(CPLX_H).read().split())
    for phrase in ("SEMANTICS", "BIT IDENTITY", "ROUTES", "ALIGNMENT", "EDGE CASES", "Autocorrelations.jl:23-37", "Bluestein",
                   "(q.astype(float32) - offset) * float32(scale)", "n alone", "TSDR_EINVAL", "TSDR_EBOUNDS", "never written",
                   "tsdr_fft_plan", "first maximum", "tsdr_argmax_d", "RAW bytes"):
        assert phrase in src, phrase


def test_header_table_and_library_agree():
    lib = _pkg("_lib")
    assert sorted(_protos()) == SYMS == lib.exported_names_cplx()
    assert not set(lib._SIGS) & set(lib._SIGS_CPLX) and not set(lib._SIGS_IQ) & set(lib._SIGS_CPLX) and not set(lib._SIGS) & set(lib._SIGS_IQ)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    for sym in SYMS:
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_cplx.h but not exported"
        assert getattr(bound, sym).restype is C.c_int and getattr(bound, sym).argtypes == lib._SIGS_CPLX[sym][1], sym


def test_table_argtypes_match_the_prototypes():
    lib = _pkg("_lib")
    ct = {"i32": C.c_int, "i64": C.c_size_t, "f32": C.c_float, "f64": C.c_double}
    for sym, params in _protos().items():
        res, args = lib._SIGS_CPLX[sym]
        assert res is C.c_int and len(args) == len(params), sym
        for k, (a, p) in enumerate(zip(args, params)):
            cls = JS.c_class(p)
            if cls == "ptr":
                assert a is C.c_void_p or (isinstance(a, type) and issubclass(a, C._Pointer)), (sym, k, p, a)
                if a is not C.c_void_p:   # a typed pointer points to what the prototype says
                    want = {"size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}[re.sub(r"\bconst\b", "", p).split()[0]]
                    assert a._type_ is want, (sym, k, p, a)
            else:
                assert a is ct[cls], (sym, k, p, a)


def test_every_ccall_of_the_cplx_shim_matches_its_prototype():
    """as test_julia_shim_static.py, for julia/TempestHIP_cplx.jl against the new header (the main shim may only name symbols of
    tempest_hip.h, hence the separate file)"""
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(tsdr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _strip(CPLX_H), flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        protos[name] = ("ptr" if "*" in ret else JS.c_class(ret + " x"), [JS.c_class(p) for p in JS.split_args(args)])
    assert sorted(protos) == SYMS and not set(protos) & set(JS.header_protos())
    jl = open(CPLX_SHIM).read()
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
    assert seen == {"tsdr_autocorr_cplx", "tsdr_autocorr_cplx_f64", "tsdr_autocorr_cplx_iq"}, "each method binds the host-pointer symbol"


def test_shim_has_the_three_methods():
    main = open(SHIM).read()
    assert main.count('include("TempestHIP_cplx.jl")') == 1
    assert main.index('include("TempestHIP_cplx.jl")') > main.index('include("TempestHIP_iq.jl")')
    assert "tsdr_autocorr_cplx" not in main
    jl = open(CPLX_SHIM).read()
    for T, sym in (("ComplexF32", "tsdr_autocorr_cplx"), ("ComplexF64", "tsdr_autocorr_cplx_f64")):
        m = re.search(r"function calculate_autocorrelation\(x::AbstractVector\{" + T + r"\}, Fs, minDelay, maxDelay, scale = :log\)(.*?)\nend", jl, flags=re.S)
        assert m, T
        assert f"ccall((:{sym}, LIB)" in m.group(1) and "resize!(out, n[]), lags" in m.group(1), T
    m = re.search(r"function calculate_autocorrelation\(x::AbstractVector\{<:IntIQ\}, Fs, minDelay, maxDelay,[^;)]*;\s*scale::Float32[^)]*\)(.*?)\nend",
                  jl, flags=re.S)
    assert m and "ccall((:tsdr_autocorr_cplx_iq, LIB)" in m.group(1) and "_iq_code(" in m.group(1)


def test_python_keywords_and_delegation():
    api, mod, search = _pkg("api"), _pkg("autocorr_cplx"), _pkg("search")
    for fn in (api.Context.calculate_autocorrelation, api.calculate_autocorrelation):
        p = inspect.signature(fn).parameters
        assert p["iq_fmt"].kind is inspect.Parameter.KEYWORD_ONLY and p["iq_fmt"].default is None
        assert p["iq_scale"].kind is inspect.Parameter.KEYWORD_ONLY and p["iq_scale"].default == 1.0
        assert p["dtype"].kind is inspect.Parameter.KEYWORD_ONLY and p["dtype"].default is None
    p = inspect.signature(api.Context.autocorr_search_complex).parameters
    assert list(p)[:8] == ["self", "sig", "Fs", "minDelay", "maxDelay", "rate_min", "rate_max", "scale"]
    assert (p["rate_min"].default, p["rate_max"].default, p["scale"].default) == (50, 90, "log")
    for k, d in (("iq_fmt", None), ("iq_scale", 1.0), ("n_samples", None)):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default == d, k
    p = inspect.signature(search.extract_configuration).parameters
    assert p["domain"].kind is inspect.Parameter.KEYWORD_ONLY and p["domain"].default == "power"
    # every call of the new `_d` symbols is in the new module; api.py calls none of them itself
    called = DH.called_symbols(open(mod.__file__).read())
    assert {s for s in SYMS if s.endswith("_d")} <= called and set(SYMS) <= called
    assert not any("cplx" in s for syms in DH.api_wrappers().values() for s in syms)
    assert "tsdr_autocorr_cplx" not in open(api.__file__).read()


def test_every_new_device_pointer_entry_point_is_called_by_the_gpu_suite():
    text = open(os.path.join(ROOT, "tests", "test_autocorr_complex_gpu.py")).read()
    called = DH.called_symbols(text)
    missing = [s for s in SYMS if s not in called]
    assert not missing, missing
    assert "import dptr_util as D" in text and "D.Arenas(" in text and "pytestmark = pytest.mark.gpu" in text
