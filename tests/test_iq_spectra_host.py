"""Host-side checks of the integer IQ forms of the spectra and demodulators (no GPU): the header declares them with the argument
order of tsdr_frames_iq_d, api.py exposes the helpers and the `iq_fmt` keywords, the Julia shim has the integer-element methods
and their ccalls name the new symbols.

The host-pointer forms are declared in include/tempest_hip.h itself; the device-pointer forms in include/tempest_hip_iq.h, which
tempest_hip.h includes, with their ctypes table (_lib._SIGS_IQ), their Python wrappers (iq.py, re-exported by api.py) and their
ccalls (julia/TempestHIP_iq.jl, included by the module).  The pins the main header has -- ctypes table == header == exported
symbols (test_abi.py), every ccall matches its prototype (test_julia_shim_static.py), every `_d` prototype is called from a GPU
test at offsets (test_dptr_host.py) -- are repeated here for that header."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import test_dptr_host as DH
import test_julia_shim_static as JS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPECTRA = {"tsdr_spectrum_iq": ["size_t N", "int lin", "float *y"],
           "tsdr_welch_iq": ["size_t len", "size_t sizeFFT", "int lin", "float *y"],
           "tsdr_waterfall_iq": ["size_t len", "size_t sizeFFT", "double *sMatrix"]}
DEMODS = ["tsdr_am_demod_iq_d", "tsdr_abs2_iq_d", "tsdr_invert_am_iq_d", "tsdr_fm_demod_iq_d"]
HEAD = ["tsdr_ctx *ctx", "const void *iq", "int iq_fmt", "float scale"]


HEADERS = [os.path.join(ROOT, "include", h) for h in ("tempest_hip.h", "tempest_hip_iq.h")]
SHIMS = [os.path.join(ROOT, "tempestsdr.jl_amd", "julia", f) for f in ("TempestHIP.jl", "TempestHIP_iq.jl")]
IQ_D = sorted([n + "_d" for n in SPECTRA] + DEMODS + ["tsdr_iq_expand_d"])


def _header_text():
    """tempest_hip.h as a C compiler reads it: with the one header it includes in place"""
    main, iq = (open(h).read() for h in HEADERS)
    assert main.count('#include "tempest_hip_iq.h"') == 1
    return main.replace('#include "tempest_hip_iq.h"', iq)


def _protos():
    src = _header_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(tsdr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        out[m.group(1)] = [" ".join(p.split()) for p in m.group(2).split(",")]
    return out


def test_header_declares_the_iq_forms():
    protos = _protos()
    assert protos["tsdr_frames_iq_d"][2:5] == HEAD[1:], "the order the new entry points copy"
    for name, rest in SPECTRA.items():
        for sym in (name, name + "_d"):
            assert protos[sym] == HEAD + rest, (sym, protos.get(sym))
    for sym in DEMODS:
        assert protos[sym] == HEAD + ["size_t n", "float *out"], (sym, protos.get(sym))
    assert protos["tsdr_iq_expand_d"] == HEAD + ["size_t n", "float *cf32_out"]
    for host_form in ("tsdr_am_demod_iq", "tsdr_abs2_iq", "tsdr_invert_am_iq", "tsdr_fm_demod_iq", "tsdr_iq_expand"):
        assert host_form not in protos, "the demodulators and the expansion have device-pointer forms only"


def test_header_states_the_contract():
    src = " ".join(_header_text().split())
    for phrase in ("BIT IDENTITY", "ROUTES", "ALIGNMENT", "EDGE CASES", "Bluestein", "GetSpectrum.jl:21-30", "GetSpectrum.jl:36-52",
                   "GetSpectrum.jl:54-66", "Demodulation.jl:26-28", "Demodulation.jl:31-35", "Demodulation.jl:17-23"):
        assert phrase in src, phrase


def test_ctypes_table_binds_them():
    from tempest_loader import load_package
    load_package()
    lib = importlib.import_module("tempestsdr_jl_amd._lib")
    import ctypes as C
    sigs = {**lib._SIGS, **lib._SIGS_IQ}
    for name in list(SPECTRA) + [n + "_d" for n in SPECTRA]:
        res, args = sigs[name]
        assert res is C.c_int and args[:4] == [C.c_void_p, C.c_void_p, C.c_int, C.c_float], name
        assert len(args) == 4 + len(SPECTRA[name[:-2] if name.endswith("_d") else name]), name
    for name in DEMODS + ["tsdr_iq_expand_d"]:
        assert sigs[name] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_void_p]), name


def test_api_exposes_helpers_and_keywords():
    from tempest_loader import load_package
    load_package()
    api = importlib.import_module("tempestsdr_jl_amd.api")
    for helper in ("spectrum_iq_d", "welch_iq_d", "waterfall_iq_d", "demod_iq_d", "expand_iq_d"):
        assert callable(getattr(api, helper)), helper
    assert list(inspect.signature(api.demod_iq_d).parameters)[0] == "kind"
    assert set(api.DEMOD_IQ) == {"am", "abs2", "invert_am", "fm"}
    for method in ("getSpectrum", "getWelch", "getWaterfall", "amDemod", "invert_amDemod", "fmDemod", "abs2"):
        p = inspect.signature(getattr(api.Context, method)).parameters
        assert p["iq_fmt"].kind is inspect.Parameter.KEYWORD_ONLY and p["iq_fmt"].default is None, method
        assert p["iq_scale"].kind is inspect.Parameter.KEYWORD_ONLY and p["iq_scale"].default == 1.0, method
    for helper in ("spectrum_iq_d", "welch_iq_d", "waterfall_iq_d", "demod_iq_d", "expand_iq_d"):
        assert helper in api.StagingRing.__doc__, "the ring's docstring names the consumers of raw slots"


def test_api_is_strict_about_the_component_dtype():
    """the checks that run before any library call: an integer format takes its own dtype, an even number of components"""
    from tempest_loader import load_package
    load_package()
    api = importlib.import_module("tempestsdr_jl_amd.api")
    a, code, n = api._int_iq(np.zeros(10, np.int8), "sc8", "getWelch")
    assert (code, n, a.dtype) == (2, 5, np.int8)
    assert api._int_iq(np.zeros(4, np.uint8), "uc8", "x")[1:] == (3, 2) and api._int_iq(np.zeros(4, np.int16), 1, "x")[1:] == (1, 2)
    for bad, fmt in ((np.zeros(10, np.uint8), "sc8"), (np.zeros(10, np.int16), "uc8"), (np.zeros(9, np.int8), "sc8"),
                     (np.zeros(10, np.complex64), "sc16"), ([0, 1], "sc8"), (np.zeros(4, np.float32), "cf32")):
        with pytest.raises(AssertionError):
            api._int_iq(bad, fmt, "getWelch")
    with pytest.raises(AssertionError):
        api.demod_iq_d("pm", None, 0, "sc8", 1.0, 0, 0)


def test_shim_has_integer_element_methods():
    main = open(SHIMS[0]).read()
    assert main.count('include("TempestHIP_iq.jl")') == 1 and main.index('include("TempestHIP_iq.jl")') > main.index("const IQ_FORMATS")
    src = main + open(SHIMS[1]).read()
    for T in ("Complex{Int16}", "Complex{Int8}", "Complex{UInt8}"):
        assert re.search(r"_iq_code\(::AbstractVector\{" + re.escape(T) + r"\}\)", src), T
    assert re.search(r"const IntIQ = Union\{Complex\{Int16\},\s*Complex\{Int8\},\s*Complex\{UInt8\}\}", src)
    for fn, sym in (("getSpectrum", "tsdr_spectrum_iq"), ("getWelch", "tsdr_welch_iq"), ("getWaterfall", "tsdr_waterfall_iq")):
        m = re.search(r"function " + fn + r"\(f[se], sig::AbstractVector\{<:IntIQ\};[^)]*scale::Float32[^)]*\)(.*?)\nend", src, flags=re.S)
        assert m, fn
        assert f"ccall((:{sym}, LIB)" in m.group(1), (fn, sym)
    for fn, sym in (("amDemod", "tsdr_am_demod_iq_d"), ("invert_amDemod", "tsdr_invert_am_iq_d")):
        m = re.search(r"function " + fn + r"\(sig::Vector\{<:Union\{Complex\{Int16\},Complex\{Int8\},Complex\{UInt8\}\}\}; scale::Float32[^)]*\)(.*?)\nend",
                      src, flags=re.S)
        assert m, fn
        assert f"ccall((:{sym}, LIB)" in m.group(1), (fn, sym)
    for sym in ("tsdr_welch_iq_d", "tsdr_waterfall_iq_d"):
        assert f"ccall((:{sym}, LIB)" in src, sym


# ---- the main header's pins, for include/tempest_hip_iq.h ---------------------------------------------------------------------
def _iq_header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADERS[1]).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdr_[a-z0-9_]+)\s*\(", src)))


def test_iq_header_table_and_library_agree():
    """as test_abi.py::test_library_exports_every_declared_symbol: header == ctypes table == exported symbols"""
    import ctypes as C
    from tempest_loader import load_package
    load_package()
    lib = importlib.import_module("tempestsdr_jl_amd._lib")
    assert _iq_header_symbols() == IQ_D == lib.exported_names_iq()
    assert not set(lib._SIGS) & set(lib._SIGS_IQ)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    for sym in IQ_D:
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_iq.h but not exported"
        assert getattr(bound, sym).argtypes == lib._SIGS_IQ[sym][1], sym


def test_every_iq_device_pointer_entry_point_is_called_at_offsets_by_a_gpu_test():
    """as test_dptr_host.py's two pins: every prototype of the header is CALLED (not just named) from the GPU suites of these
    entry points, which run them at sample offsets inside guarded arenas"""
    for path, want in (("test_iq_spectra_gpu.py", [n + "_d" for n in SPECTRA]), ("test_iq_demod_gpu.py", DEMODS + ["tsdr_iq_expand_d"])):
        text = open(os.path.join(ROOT, "tests", path)).read()
        called = DH.called_symbols(text)
        missing = [s for s in want if s not in called]
        assert not missing, (path, missing)
        assert "import dptr_util as D" in text and "D.Arenas(" in text, path


def test_every_ccall_of_the_iq_shim_matches_its_prototype():
    """as test_julia_shim_static.py, for julia/TempestHIP_iq.jl against the two headers"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADERS[1]).read(), flags=re.S)
    src = re.sub(r"^#.*$", "", src, flags=re.M)          # the include guard
    protos = JS.header_protos()
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(tsdr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        assert name not in protos, name
        protos[name] = ("ptr" if "*" in ret else JS.c_class(ret + " x"), [JS.c_class(p) for p in JS.split_args(args)])
    assert sorted(set(protos) - set(JS.header_protos())) == IQ_D and all(protos[k][0] == "i32" for k in IQ_D)
    jl = open(SHIMS[1]).read()
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
    assert {"tsdr_am_demod_iq_d", "tsdr_invert_am_iq_d", "tsdr_welch_iq_d", "tsdr_waterfall_iq_d"} <= seen
