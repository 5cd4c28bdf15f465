"""Host-side checks of the tuner (no GPU): include/tempest_hip_tune.h, its ctypes table (_lib._SIGS_TUNE), its Python module (tune.py)
and its Julia shim (julia/TempestHIP_tune.jl) agree with each other and with the library; tune_plan over random cuts of a stream;
freq_fix and design_lowpass against what they are defined to be; the numpy reference (tests/tune_ref.py) cut into calls against itself;
and the capability the feature exists for, on the reference alone: a leak at +0.23 Fs beside a carrier 20 dB stronger, which the
envelope fold loses (0.015) and the tuned fold recovers (0.931)."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import test_hires_host as HH
import test_julia_shim_static as JS
import tune_ref as R

ROOT = HH.ROOT
TUNE_H = os.path.join(ROOT, "include", "tempest_hip_tune.h")
SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP_tune.jl")
KERNEL = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "raster_tune.hip")

SYMS = ["tsdr_tune_iq", "tsdr_tune_iq_d", "tsdr_tune_tile"]
TUNE = ["tsdr_ctx *ctx", "const void *iq", "int iq_fmt", "float scale", "size_t n", "uint64_t m0", "uint64_t nu_fix", "uint64_t phi_fix",
        "const float *taps", "int n_taps", "int decim", "uint64_t j0", "float *hist", "int n_hist", "float *out", "size_t out_cap",
        "size_t *n_out"]


def _cls(p):
    """test_julia_shim_static.c_class, which does not know uint64_t"""
    c = JS.c_class(p)
    return "i64" if c == "uint64_t" else c


# ---------------------------------------------------------------- header, table, library, shims
def test_header_declares_the_entry_points():
    p = HH._protos(TUNE_H)
    assert sorted(p) == SYMS
    assert p["tsdr_tune_iq"] == p["tsdr_tune_iq_d"] == TUNE
    assert p["tsdr_tune_tile"] == ["int n_taps", "int decim"]
    main = open(HH.MAIN_H).read()
    assert main.count('#include "tempest_hip_tune.h"') == 1
    assert main.index('#include "tempest_hip_tune.h"') > main.index('#include "tempest_hip_gram.h"')
    assert not re.search(r"tsdr_tune|TSDR_TUNE", HH._strip(HH.MAIN_H))
    text = open(TUNE_H).read()
    assert "#ifndef TEMPEST_HIP_TUNE_H" in text and "#ifndef TEMPEST_HIP_GRAM_H\n#error" in text
    lib = HH._pkg("_lib")
    assert int(re.search(r"#define TSDR_TUNE_TAPS_MAX (\d+)\b", text).group(1)) == lib.TUNE_TAPS_MAX == 1024
    assert int(re.search(r"#define TSDR_TUNE_DECIM_MAX (\d+)\b", text).group(1)) == lib.TUNE_DECIM_MAX == 64


def test_header_states_the_contract():
    src = " ".join(open(TUNE_H).read().split())
    for phrase in ("STREAM, OSCILLATOR", "MIXED SAMPLE", "OUTPUT", "A CALL", "CHAINING", "FORMATS", "REPEATS", "ERROR BOUND", "REFUSALS", "COST",
                   "p[m] = (phi_fix + nu_fix * m) mod 2^64", "the integer arithmetic wraps", "Phase 0 gives w = (1, 0) exactly",
                   "re = fsub(fmul(xr, c), fmul(xi, s)), im = fadd(fmul(xr, s), fmul(xi, c))",
                   "a function of x[m]'s bits and of p[m] alone", "only complete windows, no padding",
                   "acc = fmaf(h[i], u[j*D + i], acc) for i = 0, 1, ..., L-1", "The order is a function of L only",
                   "j1 = floor((m0 + n - L) / D)", "the last min(L-1, n_hist + n) mixed samples, right-aligned",
                   "computed before anything is enqueued", "hist == NULL is allowed exactly when n_hist == 0",
                   "Nothing is written outside out[0 .. n_out) and hist", "at ANY boundaries", "chunks of one sample",
                   "(f32(q) - offset) * f32(scale)", "No float atomics", "|y[j] - y_ref[j]| <= (L + 8) * u * A * H1",
                   "at most 4 for w", "THE OSCILLATOR'S TERM", "j0 * D < m0 - n_hist", "out_cap < n_out", "n >= 2^31",
                   "not aligned to one sample", "not float-aligned", '"tune"', '"tune_hist"', "profiles/tune.json", '"wait_ms"',
                   "NOT BUILT: complex taps; rational resampling; a fused tune + detector; a tuner inside the frame loop; L > 1024"):
        assert phrase in src, phrase


def test_header_table_and_library_agree():
    lib = HH._pkg("_lib")
    assert sorted(HH._protos(TUNE_H)) == SYMS == lib.exported_names_tune()
    for other in (lib._SIGS, lib._SIGS_IQ, lib._SIGS_CPLX, lib._SIGS_HIRES, lib._SIGS_REGISTER, lib._SIGS_DISPLAY, lib._SIGS_FOLD,
                  lib._SIGS_CFOLD, lib._SIGS_CSTACK, lib._SIGS_CTRACK, lib._SIGS_GRAM):
        assert not set(other) & set(lib._SIGS_TUNE)
    bound = lib.load()
    raw = C.CDLL(lib.LIB_PATH)
    ct = {"i32": C.c_int, "i64": C.c_size_t, "f32": C.c_float, "f64": C.c_double}
    assert C.c_uint64 is C.c_size_t or C.sizeof(C.c_uint64) == C.sizeof(C.c_size_t) == 8
    for sym, params in HH._protos(TUNE_H).items():
        assert hasattr(raw, sym), f"{sym} declared in include/tempest_hip_tune.h but not exported"
        res, args = lib._SIGS_TUNE[sym]
        assert getattr(bound, sym).restype is C.c_int and getattr(bound, sym).argtypes == args, sym
        assert res is C.c_int and len(args) == len(params), sym
        for k, (a, p) in enumerate(zip(args, params)):
            cls = _cls(p)
            if cls == "ptr":
                assert a is C.c_void_p, (sym, k, p, a)
            elif "uint64_t" in p:
                assert a is C.c_uint64, (sym, k, p, a)
            else:
                assert a is ct[cls], (sym, k, p, a)


def test_every_ccall_of_the_shim_matches_its_prototype():
    protos = {name: ("i32", [_cls(p) for p in params]) for name, params in HH._protos(TUNE_H).items()}
    jl = open(SHIM).read()
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
        seen.append(m.group(1))
        cret, cparams = protos[m.group(1)]
        assert (ret, types, len(parts) - 3) == (cret, cparams, len(cparams)), (m.group(1), ret, types, cret, cparams)
    assert sorted(seen) == SYMS, "one ccall per symbol"
    main = open(HH.SHIM).read()
    assert main.count('include("TempestHIP_tune.jl")') == 1
    assert main.index('include("TempestHIP_tune.jl")') > main.index('include("TempestHIP_gram.jl")')
    for name in ("hip_tune!", "hip_tune_d!", "freq_fix", "design_lowpass", "tune_plan"):
        assert re.search(r"\nfunction " + re.escape(name) + r"\(", jl), name
    tests = open(os.path.join(os.path.dirname(SHIM), "runtests.jl")).read()
    assert "TempestHIP.hip_tune!(" in tests and "TempestHIP.tune_plan(" in tests


def test_python_interface_and_delegation():
    api, mod = HH._pkg("api"), HH._pkg("tune")
    want = {"tune_d": ["iq", "fmt", "scale", "n", "m0", "nu_fix", "phi_fix", "taps", "n_taps", "decim", "j0", "hist", "n_hist", "out", "out_cap"],
            "tune": ["iq", "nu_fix", "taps", "decim", "m0", "phi_fix", "j0", "hist", "n_hist", "fmt", "scale"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(api.Context, name)).parameters) == ["self"] + params, name
        assert list(inspect.signature(getattr(mod, name)).parameters) == ["ctx"] + params, name
    assert list(inspect.signature(api.Context.tuner).parameters) == ["self", "nu_fix", "taps", "decim", "phi_fix", "m0"]
    assert list(inspect.signature(mod.Tuner.push_d).parameters) == ["self", "iq", "fmt", "scale", "n", "out", "out_cap"]
    assert list(inspect.signature(mod.tune_plan).parameters) == ["m0", "n", "L", "D", "j0", "n_hist", "Fs"]
    p = inspect.signature(mod.design_lowpass).parameters
    assert list(p) == ["L", "D", "width", "window"] and p["width"].default == 0.9 and p["window"].default == "blackman"
    pkg = importlib.import_module("tempestsdr_jl_amd")
    for name in ("Tuner", "design_lowpass", "freq_fix", "tune", "tune_d", "tune_plan"):
        assert getattr(pkg, name) is getattr(mod, name), name
    # every call of the symbols is in tune.py
    d = os.path.dirname(mod.__file__)
    for f in os.listdir(d):
        if f.endswith(".py") and f not in ("tune.py", "_lib.py"):
            assert "tsdr_tune" not in open(os.path.join(d, f)).read(), f
    assert os.path.exists(KERNEL), "picked up by build.py's directory scan"
    assert '"tempest_hip_tune.h"' in open(os.path.join(ROOT, "tempestsdr.jl_amd", "build.py")).read()


def test_refusals_need_no_device():
    """a NULL context is refused before anything else; tsdr_tune_tile needs none"""
    lib = HH._pkg("_lib").load()
    n_out = C.c_size_t(77)
    buf = np.zeros(16, np.float32)
    for sym in ("tsdr_tune_iq", "tsdr_tune_iq_d"):
        rc = getattr(lib, sym)(None, buf.ctypes.data, 0, C.c_float(1.0), 4, 0, 0, 0, buf.ctypes.data, 1, 1, 0, None, 0, buf.ctypes.data, 8,
                               C.byref(n_out))
        assert rc == -1 and n_out.value == 77
    assert lib.tsdr_tune_tile(63, 4) == 1024 and lib.tsdr_tune_tile(1024, 64) == 80
    for L, D in ((0, 1), (1025, 1), (1, 0), (1, 65)):
        assert lib.tsdr_tune_tile(L, D) == -1
    for L in (1, 2, 63, 64, 65, 255, 1024):
        for D in (1, 2, 3, 4, 7, 16, 64):
            t = lib.tsdr_tune_tile(L, D)
            S = 4 * D
            ns = (t - 1) * D + L
            assert t % 4 == 0 and 80 <= t <= 1024 and (ns + ns // S + 1) * 8 <= 48 * 1024, (L, D, t)


# ---------------------------------------------------------------- tune_plan, freq_fix, design_lowpass
@pytest.mark.parametrize("L,D", [(1, 1), (1, 3), (3, 7), (63, 4), (65, 4), (64, 1), (1024, 64)])
def test_plan_over_random_cuts_covers_every_output_once(L, D):
    """a stream cut at random boundaries -- single samples, chunks below L - 1, chunks that are no multiple of D: the calls' outputs
    are j = first .. last of the whole stream, each exactly once, in order, and no call asks for a window before its history"""
    mod = HH._pkg("tune")
    rng = np.random.default_rng(L * 131 + D)
    for trial in range(20):
        m_start = int(rng.integers(0, 3)) * int(rng.integers(0, 1 << 40))
        total = int(rng.integers(1, 6 * L + 40 * D))
        whole_n, _ = mod.tune_plan(m_start, total, L, D, -(-m_start // D), 0)
        m0, j0, nh, left, got = m_start, -(-m_start // D), 0, total, []
        while left:
            n = int(min(left, rng.choice([1, 1, max(L - 2, 1), int(rng.integers(1, 3 * L + 5 * D))])))
            assert j0 * D >= m0 - nh
            k, nxt = mod.tune_plan(m0, n, L, D, j0, nh)
            got += list(range(j0, j0 + k))
            assert nxt["m0"] == m0 + n and nxt["j0"] == j0 + k and nxt["n_hist"] == min(L - 1, nh + n)
            assert nxt["decim"] == D and nxt["delay"] == (L - 1) / 2.0
            m0, j0, nh, left = nxt["m0"], nxt["j0"], nxt["n_hist"], left - n
        first = -(-m_start // D)
        assert got == list(range(first, first + whole_n)), (trial, m_start, total)
        if whole_n:
            assert got[-1] * D + L <= m_start + total < (got[-1] + 1) * D + L
    assert mod.tune_plan(0, 100, L, D, 0, 0, Fs=50e6)[1]["Fs_out"] == 50e6 / D
    with pytest.raises(AssertionError):
        mod.tune_plan(10 * D + 1, 5, L, D, 9, 0)          # 9 D < m0 with no history
    with pytest.raises(AssertionError):
        mod.tune_plan(0, 5, L, D, 0, L)                    # n_hist > L - 1


def test_freq_fix_wraps_and_negates():
    mod = HH._pkg("tune")
    M = 1 << 64
    assert mod.freq_fix(0.0, 1.0) == 0
    assert mod.freq_fix(0.25, 1.0) == M // 4 and mod.freq_fix(-0.25, 1.0) == 3 * M // 4
    assert mod.freq_fix(12.5e6, 50e6) == M // 4
    assert mod.freq_fix(1.25, 1.0) == M // 4 and mod.freq_fix(-1.0, 1.0) == 0 and mod.freq_fix(0.5, 1.0) == mod.freq_fix(-0.5, 1.0) == M // 2
    for f, Fs in ((0.23, 1.0), (1234567.0, 50e6), (3.3e6, 2e8), (1e-9, 1.0)):
        a, b = mod.freq_fix(f, Fs), mod.freq_fix(-f, Fs)
        assert (a + b) % M == 0 and 0 <= a < M
        assert abs(a / M - (f / Fs) % 1.0) < 1e-15
    assert mod.phase_fix(0.5) == M // 2 and mod.phase_fix(-0.25) == 3 * M // 4
    with pytest.raises(AssertionError):
        mod.freq_fix(1.0, 0.0)


@pytest.mark.parametrize("L,D", [(1, 1), (2, 1), (63, 4), (64, 4), (127, 2), (255, 16), (1024, 64)])
def test_design_lowpass_has_unit_gain_and_symmetry(L, D):
    mod = HH._pkg("tune")
    h = mod.design_lowpass(L, D)
    assert h.dtype == np.float32 and h.shape == (L,)
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= L * 2.0 ** -25
    assert np.array_equal(h, h[::-1])
    if L >= 63:
        f = np.fft.rfft(h.astype(np.float64), 16384)
        k = np.arange(f.size) / 16384.0
        edge = 0.45 / D + 6.0 / L          # the cut-off plus the Blackman window's main lobe
        assert edge < 0.5 and np.abs(f[k >= edge]).max() < 2e-3, "the stop band"
        assert abs(abs(f[0]) - 1.0) < 1e-6
    if (L, D) == (63, 4):
        assert np.array_equal(h, R.cap_taps())
    assert mod.tuned_t0(4 * 9150.37, 63, 4) == 9150.37 - 31 / 4


# ---------------------------------------------------------------- the reference
def test_the_reference_knows_its_phases():
    """uint64 wrap against Python integers at an index far out; the oscillator at the quarter turns"""
    nu, phi, m0 = (0xD1B54A32D192ED03 | 1), 0x0123456789ABCDEF, (1 << 40) + 12345
    p = R.phases(m0, 1000, nu, phi)
    for k in (0, 1, 999):
        assert int(p[k]) == R.phase_exact(m0 + k, nu, phi)
    w = R.oscillator(np.array([0, 1 << 62, 1 << 63, 3 << 62], np.uint64))
    assert np.allclose(w, [1, 1j, -1, -1j], atol=1e-15) and w[0] == 1.0
    # a tone shifted to DC and low-passed by unit-gain taps is the constant it started from
    m = np.arange(4000)
    x = (0.5 * np.exp(2j * np.pi * 0.125 * m)).astype(np.complex64)
    y = R.whole(x, 0, (7 << 61), 0, HH._pkg("tune").design_lowpass(31, 4), 4)
    assert y.size == (4000 - 31) // 4 + 1 and np.abs(y - 0.5).max() < 1e-6


@pytest.mark.parametrize("cut", ["ones", "short", "random"])
def test_the_reference_is_chaining_invariant(cut):
    L, D, n, m_start = 65, 4, 5000, 1237
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    h = HH._pkg("tune").design_lowpass(L, D)
    nu, phi = 0x3AE147AE147AE147, 12345
    first = -(-m_start // D)
    want = R.whole(x, m_start, nu, phi, h, D)
    chunks = {"ones": [1] * (L + 3), "short": [L - 2] * (n // (L - 2)), "random": [int(c) | 1 for c in rng.integers(1, 300, 60)]}[cut]
    hist, nh, m0, j0, pos, got = np.zeros(L - 1, np.complex128), 0, m_start, first, 0, []
    for c in chunks + [n]:
        c = min(c, n - pos)
        if c == 0:
            break
        y, hist, nh = R.call(x[pos:pos + c], m0, nu, phi, h, D, j0, hist, nh)
        got.append(y)
        m0, j0, pos = m0 + c, j0 + y.size, pos + c
    got = np.concatenate(got)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12
    assert np.abs(hist - R.mixed(x, m_start, nu, phi)[-(L - 1):]).max() == 0.0


def test_capability_on_the_reference():
    """the figures of the feature: the jammed capture folds to 0.015 raw and to 0.931 tuned; without the interferer 0.905"""
    synth = HH._pkg("synth")
    clean, jammed = R.cap_captures(synth)
    card = R.cap_card(synth)
    y = R.whole(jammed, 0, R.cap_nu(), 0, R.cap_taps(), R.CAP["D"])
    tuned, raw, base = R.corr(R.cap_fold_tuned(y), card), R.corr(R.cap_fold_raw(jammed), card), R.corr(R.cap_fold_raw(clean), card)
    print(f"capability (reference): tuned {tuned:.4f}, raw {raw:.4f}, without the interferer {base:.4f}")
    assert tuned >= 0.85 and raw <= 0.2
    assert abs(tuned - 0.931) < 2e-3 and abs(raw - 0.015) < 2e-3 and abs(base - 0.905) < 2e-3
