"""Host-side checks of the 8-bit IQ input (no GPU): the conversion rule restated in numpy with known-answer pins, the three
generic entry points in the header / the ctypes table / the built library, and the Python layer's refusals, which come before
any library call."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import iq8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tempest_hip.h")
NEW = ("tsdr_frames_iq_d", "tsdr_frames_submit_iq_d", "tsdr_autocorr_search_iq_d")


def _f32(x):
    return np.float32(x)


@pytest.mark.parametrize("scale", [1.0, 1.0 / 127.0, 3.0e-5, 0.1, 1.7e-3])
def test_conversion_pins(scale):
    s = _f32(scale)
    uc = R.expand(np.array([0, 255, 127, 128], np.uint8), "uc8", s).view(np.float32)
    want = np.array([_f32(-127.5) * s, _f32(127.5) * s, _f32(-0.5) * s, _f32(0.5) * s], np.float32)
    assert np.array_equal(uc.view(np.uint32), want.view(np.uint32))
    sc = R.expand(np.array([-128, 127, 0, -1], np.int8), "sc8", s).view(np.float32)
    want = np.array([_f32(-128.0) * s, _f32(127.0) * s, _f32(0.0) * s, _f32(-1.0) * s], np.float32)
    assert np.array_equal(sc.view(np.uint32), want.view(np.uint32))
    s16 = R.expand(np.array([-32768, 32767], np.int16), "sc16", s).view(np.float32)
    assert np.array_equal(s16, np.array([_f32(-32768.0) * s, _f32(32767.0) * s], np.float32))


def test_uc8_subtraction_is_exact_for_all_codes():
    codes = np.arange(256, dtype=np.uint8)
    d32 = codes.astype(np.float32) - np.float32(127.5)
    d64 = codes.astype(np.float64) - 127.5
    assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), d64)
    assert d32[0] == -127.5 and d32[255] == 127.5 and np.all(np.abs(d32) <= 127.5) and np.all(d32 * 2 == np.round(d32 * 2))


def test_each_component_is_the_f32_product_of_the_exact_difference():
    """one rounding: the f32 product equals the correctly rounded f64 product of the same two f32 operands"""
    rng = np.random.default_rng(5)
    for fmt in ("sc8", "uc8"):
        q = rng.integers(0, 256, 4096).astype(np.uint8).view(R.DTYPES[fmt])
        for scale in (np.float32(1.0 / 127.0), np.float32(2.3456e-4)):
            got = R.expand(q, fmt, scale).view(np.float32)
            want = ((q.astype(np.float64) - R.OFFSETS[fmt]) * np.float64(scale)).astype(np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_package_expand_iq_is_the_same_rule(tsdr):
    api = importlib.import_module("tempestsdr_jl_amd.api")
    rng = np.random.default_rng(6)
    raw = rng.integers(0, 256, 2048).astype(np.uint8)
    for fmt in ("sc8", "uc8"):
        q = raw.view(R.DTYPES[fmt])
        a, b = api.expand_iq(q, fmt, 0.0123), R.expand(q, fmt, 0.0123)
        assert a.dtype == np.complex64 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    q16 = rng.integers(-2048, 2048, 512).astype(np.int16)
    assert np.array_equal(api.expand_iq(q16, "sc16", 0.5).view(np.uint32), R.expand(q16, "sc16", 0.5).view(np.uint32))
    with pytest.raises(AssertionError):
        api.expand_iq(raw, "sc8", 1.0)          # uint8 is not sc8
    assert {k: v[0] for k, v in api.IQ_FORMATS.items()} == R.CODES


def _header_proto(name):
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in tempest_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_formats_and_entry_points():
    text = open(HEADER).read()
    m = re.search(r"enum\s*\{\s*TSDR_IQ_CF32\s*=\s*0\s*,\s*TSDR_IQ_SC16\s*=\s*1\s*,\s*TSDR_IQ_SC8\s*=\s*2\s*,\s*TSDR_IQ_UC8\s*=\s*3\s*\}", text)
    assert m, "enum { TSDR_IQ_CF32 = 0, TSDR_IQ_SC16 = 1, TSDR_IQ_SC8 = 2, TSDR_IQ_UC8 = 3 }"
    assert "127.5" in text
    fr = _header_proto("tsdr_frames_iq_d")
    assert len(fr) == 16 and fr[2] == "const void *iq" and fr[3] == "int iq_fmt" and fr[4] == "float scale"
    assert _header_proto("tsdr_frames_submit_iq_d") == fr
    se = _header_proto("tsdr_autocorr_search_iq_d")
    assert len(se) == 15 and se[1] == "const void *iq" and se[2] == "int iq_fmt" and se[3] == "float scale"
    # the existing entry points keep their signatures
    assert len(_header_proto("tsdr_frames_sc16_d")) == 15 and len(_header_proto("tsdr_frames_d")) == 14
    assert len(_header_proto("tsdr_autocorr_search_d")) == 14
    # ring formats 3 .. 6 are documented where the ring is
    ring_doc = text[text.index("host -> device staging ring"):text.index("typedef struct tsdr_ring")]
    for word in ("fmt 3", "fmt 4", "fmt 5", "fmt 6"):
        assert word in ring_doc, word


def test_bound_in_lib_py_with_matching_argument_counts(tsdr):
    for name in NEW:
        assert name in tsdr._lib._SIGS, name
        restype, args = tsdr._lib._SIGS[name]
        assert restype is ctypes.c_int and len(args) == len(_header_proto(name)), name
    args = tsdr._lib._SIGS["tsdr_frames_iq_d"][1]
    assert args[3] is ctypes.c_int and args[4] is ctypes.c_float
    args = tsdr._lib._SIGS["tsdr_autocorr_search_iq_d"][1]
    assert args[2] is ctypes.c_int and args[3] is ctypes.c_float


def test_exported_by_the_built_library(tsdr):
    lib = tsdr._lib.load()      # (built by build(); cross-compiled where there is no GPU)
    for name in NEW:
        assert hasattr(lib, name), name


class _NoLib:
    """a context whose every library call is an error: the refusals below must come first"""
    h = None

    def call(self, *a, **k):
        raise RuntimeError("library call before the argument check")

    def __getattr__(self, name):
        raise RuntimeError(f"library access ({name}) before the argument check")


def test_staging_ring_refuses_unknown_formats_and_wrong_slots(tsdr):
    api = importlib.import_module("tempestsdr_jl_amd.api")
    with pytest.raises(AssertionError):
        api.StagingRing(_NoLib(), 64, 2, fmt="sc4")
    for fmt, dt, other in (("sc8", np.int8, np.uint8), ("sc8raw", np.int8, np.uint8), ("uc8", np.uint8, np.int8), ("uc8raw", np.uint8, np.int8)):
        r = api.StagingRing.__new__(api.StagingRing)
        r.ctx, r.nEch, r.depth, r.fmt, r.h, r.sample_bytes, r.scale = _NoLib(), 64, 2, fmt, None, 2, 1.0
        assert api.StagingRing.FORMATS[fmt] in (3, 4, 5, 6)
        with pytest.raises(AssertionError):
            r.put(np.zeros(2 * 64, np.int16))       # 4 bytes per sample: wrong slot size
        with pytest.raises(AssertionError):
            r.put(np.zeros(2 * 64 - 2, dt))         # one sample short
        with pytest.raises(AssertionError):
            r.put(np.zeros(2 * 64, other))          # right size, the other 8-bit format
        assert r.iq_fmt == ("cf32" if not fmt.endswith("raw") else fmt[:3])
    assert api.StagingRing.FORMATS == {"cf32": 0, "sc16": 1, "sc16raw": 2, "sc8": 3, "sc8raw": 4, "uc8": 5, "uc8raw": 6}


def test_autocorr_search_is_strict_about_integer_input(tsdr):
    api = importlib.import_module("tempestsdr_jl_amd.api")
    c = api.Context.__new__(api.Context)
    c.h, c.lib = None, _NoLib()
    for fmt, bad in (("sc8", np.zeros(64, np.uint8)), ("uc8", np.zeros(64, np.int8)), ("sc16", np.zeros(64, np.int8)),
                     ("sc8", np.zeros(63, np.int8)), ("sc8", np.zeros(32, np.complex64)), ("sc8", [0] * 64)):
        with pytest.raises(AssertionError):
            api.Context.autocorr_search(c, bad, 1000.0, 0, 0.01, iq_fmt=fmt, iq_scale=1.0)
    with pytest.raises(AssertionError):
        api.Context.autocorr_search(c, np.zeros(64, np.int8), 1000.0, 0, 0.01, iq_fmt="sc12")
    with pytest.raises(AssertionError):
        api.Context.autocorr_search(c, np.zeros(64, np.float32), 1000.0, 0, 0.01, iq_fmt="cf32")
    with pytest.raises(AssertionError):
        api.Context.autocorr_search(c, 0x1000, 1000.0, 0, 0.01, iq_fmt="sc8")      # a device address without n_samples
    with pytest.raises(AssertionError):
        api.frames_iq_d(_NoLib(), None, 0x1000, "sc4", 1.0, 10, 10, 2, 2, 0.1, True, 0x2000)
