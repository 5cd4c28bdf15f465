"""CPU side of the device-pointer tests: the arena guard (dptr_util.py) is shown to see a stray store -- in front of the
payload, behind it, into an input -- and to let an exact write pass; and every `_d` prototype of include/tempest_hip.h is
called by name from some tests/test_*_gpu.py, so a new device-pointer entry point cannot arrive untested."""
import ast
import glob
import os
import re

import numpy as np
import pytest

import dptr_util as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the guard, on a numpy stand-in for the device ---------------------------------------------------------------------
def _arena(phase, n, data=None):
    lead = D.MIN_GUARD + phase
    return lead, D.image(lead, 4 * n, data)


@pytest.mark.parametrize("phase", [0, 4, 8, 12])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_guard_lets_an_exact_write_pass(phase, n):
    lead, w = _arena(phase, n)
    assert w.size * 4 >= lead + 4 * n + D.MIN_GUARD and (w.size * 4) % 64 == 4
    w[lead // 4: lead // 4 + n] = np.arange(n, dtype=np.float32).view(np.uint32)   # the "kernel": exactly its n outputs
    D.verify(w, lead, 4 * n, "out")
    # an untouched output arena passes too (the guard does not demand that the payload was written: values are the test's job)
    D.verify(D.image(lead, 4 * n), lead, 4 * n, "out")


def test_sentinel_is_finite_far_from_data_and_never_repeats():
    w = D.sentinel_words(1 << 20)
    assert np.unique(w).size == w.size
    f = w.view(np.float32)
    assert np.all(np.isfinite(f)) and np.all(f < -5e5)
    d = w[: 1 << 10].view(np.float64)
    assert np.all(np.isfinite(d)) and np.all(d < -1e40)
    # a copy shifted by any number of words differs everywhere
    assert np.all(w[1:] != w[:-1]) and np.all(w[4:] != w[:-4])


@pytest.mark.parametrize("phase", [0, 4, 8, 12])
def test_guard_reports_a_word_in_front(phase):
    lead, w = _arena(phase, 100)
    w[lead // 4 - 1] = np.float32(1.0).view(np.uint32)
    with pytest.raises(AssertionError, match=r"1 word\(s\) written IN FRONT of the payload, 4 \.\. 4 bytes before its start"):
        D.verify(w, lead, 400, "out")
    lead, w = _arena(phase, 100)
    w[lead // 4 - 4: lead // 4] = 0     # one 16-byte vector that starts 16 bytes early
    with pytest.raises(AssertionError, match=r"4 word\(s\) written IN FRONT of the payload, 4 \.\. 16 bytes before"):
        D.verify(w, lead, 400, "out")
    lead, w = _arena(phase, 100)
    w[0] = 0                            # the far end of the lead is watched too
    with pytest.raises(AssertionError, match=rf"1 word\(s\) written IN FRONT of the payload, {lead} \.\. {lead} bytes before"):
        D.verify(w, lead, 400, "out")


@pytest.mark.parametrize("phase", [0, 4, 8, 12])
def test_guard_reports_a_word_behind(phase):
    lead, w = _arena(phase, 101)
    w[lead // 4 + 101] = np.float32(-2.5).view(np.uint32)
    with pytest.raises(AssertionError, match=r"1 word\(s\) written BEHIND the payload, 0 \.\. 0 bytes past its end"):
        D.verify(w, lead, 404, "out")
    lead, w = _arena(phase, 101)
    w[lead // 4 + 101 + 2] = 7          # e.g. the last lane of a float4 store that ran over a tail of 1
    with pytest.raises(AssertionError, match=r"1 word\(s\) written BEHIND the payload, 8 \.\. 8 bytes past its end"):
        D.verify(w, lead, 404, "out")
    lead, w = _arena(phase, 101)
    w[-1] = 7                           # the last word of the arena
    far = w.size * 4 - 4 - (lead + 404)
    with pytest.raises(AssertionError, match=rf"1 word\(s\) written BEHIND the payload, {far} \.\. {far} bytes past"):
        D.verify(w, lead, 404, "out")


def test_guard_reports_a_sentinel_copied_to_the_wrong_place():
    """a shifted copy of the guard region itself (what a memmove-like bug leaves) is not mistaken for the sentinel"""
    lead, w = _arena(8, 64)
    hi = lead // 4 + 64
    w[hi + 1] = w[hi]
    with pytest.raises(AssertionError, match=r"BEHIND the payload, 4 \.\. 4 bytes"):
        D.verify(w, lead, 256, "out")


def test_guard_reports_a_written_input():
    x = np.linspace(-1, 1, 333).astype(np.float32)
    lead, w = _arena(4, x.size, x)
    D.verify(w, lead, x.nbytes, "x", x)                      # as uploaded: fine
    w[lead // 4 + 17] = np.float32(0.25).view(np.uint32)     # an in-place "optimisation" of the kernel
    with pytest.raises(AssertionError, match=r"arena 'x' .*1 word\(s\) of the INPUT were overwritten, first at byte 68"):
        D.verify(w, lead, x.nbytes, "x", x)
    # complex and f64 inputs go in as they lie in memory
    z = (np.arange(10) + 1j * np.arange(10)).astype(np.complex128)
    lead = D.MIN_GUARD + 16
    w = D.image(lead, z.nbytes, z)
    assert np.array_equal(w[lead // 4: lead // 4 + 40].view(np.complex128), z)
    D.verify(w, lead, z.nbytes, "z", z)
    w[lead // 4 + 39] ^= 1
    with pytest.raises(AssertionError, match=r"INPUT were overwritten, first at byte 156"):
        D.verify(w, lead, z.nbytes, "z", z)


def test_guard_reports_both_sides_and_names_the_phase():
    lead, w = _arena(12, 10)
    w[lead // 4 - 2] = 1
    w[lead // 4 + 10] = 2
    with pytest.raises(AssertionError) as e:
        D.verify(w, lead, 40, "y")
    msg = str(e.value)
    assert "arena 'y'" in msg and "12 mod 16" in msg and "IN FRONT" in msg and "BEHIND" in msg


# ---- coverage pin: every `_d` prototype is called from the GPU suite -------------------------------------------------------
def _header_d_prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tempest_hip.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tsdr_\w+_d)\s*\(", src)))


def _symbols_in(tree, wrappers):
    out = set()
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        name = node.func.attr if isinstance(node.func, ast.Attribute) else node.func.id if isinstance(node.func, ast.Name) else ""
        if name.startswith("tsdr_") and isinstance(node.func, ast.Attribute):
            out.add(name)
        elif name == "call" and isinstance(node.func, ast.Attribute):
            for arg in node.args[:1]:
                for c in ast.walk(arg):
                    if isinstance(c, ast.Constant) and isinstance(c.value, str) and c.value.startswith("tsdr_"):
                        out.add(c.value)
        elif name in wrappers:
            out |= wrappers[name]
    return out


def api_wrappers():
    """functions and methods of tempestsdr.jl_amd/api.py that call a `_d` symbol themselves (frames_d, frames_iq_d, take_d,
    autocorr_search, ...) -> the `_d` symbols they call: a test that calls such a wrapper calls those entry points"""
    tree = ast.parse(open(os.path.join(ROOT, "tempestsdr.jl_amd", "api.py")).read())
    out = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef):
            syms = {s for s in _symbols_in(node, {}) if s.endswith("_d")}
            if syms:
                out.setdefault(node.name, set()).update(syms)
    return out


def called_symbols(py_source, wrappers=None):
    """tsdr_* names a test file CALLS: `x.call("tsdr_name", ...)` (string constants anywhere in the first argument, so
    `"a" if c else "b"` counts both), `x.lib.tsdr_name(...)`, and calls of the api.py wrappers given in `wrappers`.  Comments,
    docstrings and other strings do not count."""
    return _symbols_in(ast.parse(py_source), wrappers or {})


# name -> why no test calls it.  The only way out of the pin below; empty today.
NOT_CALLED_BY_NAME = {}


def _gpu_test_calls():
    calls, wrappers = {}, api_wrappers()
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*_gpu.py"))):
        for s in called_symbols(open(path).read(), wrappers):
            calls.setdefault(s, []).append(os.path.basename(path))
    return calls


def test_api_wrappers_are_the_expected_ones():
    w = api_wrappers()
    assert w["take_d"] == {"tsdr_ring_take_d"} and w["frames_d"] == {"tsdr_frames_d"}
    assert w["frames_iq_d"] == {"tsdr_frames_iq_d", "tsdr_frames_submit_iq_d"}
    assert w["frames_sc16_d"] == {"tsdr_frames_sc16_d", "tsdr_frames_submit_sc16_d"}
    assert w["autocorr_search"] == {"tsdr_autocorr_search_d", "tsdr_autocorr_search_iq_d"}
    assert set(w) == {"take_d", "frames_d", "frames_submit_d", "frames_iq_d", "frames_sc16_d", "autocorr_search"}, sorted(w)


def test_called_symbols_sees_calls_only():
    src = '''
def t(ctx):
    """tsdr_in_docstring_d"""
    # ctx.call("tsdr_in_comment_d")
    name = "tsdr_plain_string_d"
    ctx.call("tsdr_a_d", 1)
    ctx.call("tsdr_b_d" if x else "tsdr_c_d", 1)
    ctx.lib.tsdr_e_d(ctx.h)
    f = {"k": lambda c: c.call("tsdr_f_d")}
    api.wrapped(ctx)
    other(ctx)
'''
    assert called_symbols(src) == {"tsdr_a_d", "tsdr_b_d", "tsdr_c_d", "tsdr_e_d", "tsdr_f_d"}
    assert called_symbols(src, {"wrapped": {"tsdr_g_d"}, "unused": {"tsdr_h_d"}}) == {"tsdr_a_d", "tsdr_b_d", "tsdr_c_d", "tsdr_e_d", "tsdr_f_d",
                                                                                  "tsdr_g_d"}


def test_every_device_pointer_entry_point_is_called_by_a_gpu_test():
    protos = _header_d_prototypes()
    assert len(protos) >= 46 and "tsdr_welch_d" in protos and "tsdr_resampler_run_f64_d" in protos, protos
    calls = _gpu_test_calls()
    missing = [p for p in protos if p not in calls and p not in NOT_CALLED_BY_NAME]
    assert not missing, f"`_d` entry points no tests/test_*_gpu.py calls: {missing}"
    stale = [p for p in NOT_CALLED_BY_NAME if p not in protos or p in calls]
    assert not stale, f"allow-list entries that are no longer needed: {stale}"
    assert len(NOT_CALLED_BY_NAME) <= 2 and all(len(why) > 20 for why in NOT_CALLED_BY_NAME.values())


def test_the_offset_suite_itself_calls_the_per_function_forms():
    """the pin above is satisfied by ANY gpu test; the per-function `_d` forms (everything but the frame loop's pipeline, sc16 / iq
    variants, scan / combine and the ring, which have suites of their own) must be called from test_dptr_gpu.py, at offsets"""
    own = called_symbols(open(os.path.join(ROOT, "tests", "test_dptr_gpu.py")).read())
    elsewhere = {"tsdr_frames_submit_d", "tsdr_frames_sc16_d", "tsdr_frames_submit_sc16_d", "tsdr_frames_iq_d", "tsdr_frames_submit_iq_d",
                 "tsdr_frames_scan_d", "tsdr_frames_combine_d", "tsdr_autocorr_search_iq_d", "tsdr_ring_take_d"}
    missing = [p for p in _header_d_prototypes() if p not in own and p not in elsewhere]
    assert not missing, missing
