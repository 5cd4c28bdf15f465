"""Float64 getWelch / getWaterfall / init_resampler, CPU side: the header and the ctypes table carry the seven `_f64`
symbols, the Julia shim has Float64 / ComplexF64 methods that call them with the right pointer types, and the numpy
restatement (f64_spec_ref.py) is pinned by known answers."""
import os
import re

import numpy as np
import pytest

import f64_spec_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP.jl")
rng = np.random.default_rng(4064)

SYMBOLS = ["tsdr_welch_f64", "tsdr_welch_f64_d", "tsdr_waterfall_f64", "tsdr_waterfall_f64_d", "tsdr_resampler_init_f64",
           "tsdr_resampler_run_f64", "tsdr_resampler_run_f64_d"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tempest_hip.h")).read(), flags=re.S)


def test_header_declares_the_spectra_f64_symbols():
    src = _header()
    missing = [s for s in SYMBOLS if not re.search(r"\b" + s + r"\s*\(", src)]
    assert not missing, missing


def test_ctypes_table_binds_the_spectra_f64_symbols():
    src = open(os.path.join(ROOT, "tempestsdr.jl_amd", "_lib.py")).read()
    missing = [s for s in SYMBOLS if f'"{s}":' not in src]
    assert not missing, missing


def test_header_no_longer_keeps_welch_waterfall_resampler_float32():
    raw = open(os.path.join(ROOT, "include", "tempest_hip.h")).read()
    assert "getWelch / getWaterfall and init_resampler stay Float32" not in raw


def _functions(src, name):
    out = []
    for m in re.finditer(r"^function " + re.escape(name) + r"\((.*?)\)(?: where [^\n]*)?(?:\s+#[^\n]*)?$", src, flags=re.M):
        out.append((m.group(1), src[m.end(): src.find("\nend", m.end())]))
    return out


@pytest.mark.parametrize("name,sym", [("getWelch", "tsdr_welch_f64"), ("getWaterfall", "tsdr_waterfall_f64")])
def test_shim_spectra_have_float64_methods(name, sym):
    src = open(SHIM).read()
    hits = [(sig, body) for sig, body in _functions(src, name) if "Union{Float64,ComplexF64}" in sig]
    assert len(hits) == 1, f"{name}: expected one Float64 / ComplexF64 method"
    sig, body = hits[0]
    assert f"(:{sym}," in body and "Ptr{Float64}" in body
    assert ("Vector{Float64}" in body) if name == "getWelch" else ("Matrix{Float64}" in body)
    # the Float32 methods keep their element types (other types stay a MethodError)
    assert "_raw32(sig::AbstractVector{<:Union{Float32,ComplexF32}})" in src


def test_shim_init_resampler_float64():
    src = open(SHIM).read()
    (sig, body), = _functions(src, "init_resampler")
    assert "T == Float32 || T == Float64 || throw(AssertionError(" in body
    assert "T == Float64 && return _init_resampler64(bufferSize, upCoeff)" in body
    (_, b64), = _functions(src, "_init_resampler64")
    assert "(:tsdr_resampler_init_f64," in b64
    run = re.search(r"ccall\(\(:tsdr_resampler_run_f64, LIB\), Cint, \(([^)]*)\)", b64)
    assert run and run.group(1) == "Ptr{Cvoid}, Ptr{Float64}, Csize_t, Ptr{Float64}", run and run.group(1)
    assert '@assert T == T2 "Type of input ($T2) should match type used during init ($T)"' in b64
    assert "@assert length(in) == bufferSize" in b64


# ---- the restatement, pinned ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k,nb", [(1024, 3, 5), (1000, 17, 3), (6, 1, 4), (17, 5, 2), (2, 1, 7)])
def test_ref_welch_tone(N, k, nb):
    n = np.arange(nb * N + N // 2)   # a ragged tail that must be dropped
    x = np.exp(2j * np.pi * k * n / N)
    y = S.welch(x, N, lin=True)
    j = (k + N // 2) % N   # fftshift: input k lands at (k - ceil(N/2)) mod N
    assert abs(y[j] - nb * N * N) < 1e-9 * nb * N * N
    y[j] = 0
    assert np.max(np.abs(y)) < 1e-9 * nb * N * N
    assert S.welch(x, N)[j] == pytest.approx(10 * np.log10(nb * N * N), abs=1e-9)


def test_ref_welch_no_segment_is_minus_inf():
    assert np.array_equal(S.welch(np.ones(5), 8, lin=True), np.zeros(8))
    assert np.all(np.isneginf(S.welch(np.ones(5), 8)))
    assert S.waterfall(np.ones(5, np.complex128), 8).shape == (8, 0)


@pytest.mark.parametrize("N", [8, 1000, 17])
def test_ref_waterfall_impulses_give_flat_columns(N):
    nb = 6
    amp = rng.standard_normal(nb) + 1j * rng.standard_normal(nb)
    x = np.zeros(nb * N + 3, np.complex128)
    x[np.arange(nb) * N] = amp
    m = S.waterfall(x, N)
    assert m.shape == (N, nb) and m.dtype == np.float64 and m.flags.f_contiguous
    assert np.allclose(m, np.abs(amp)[None, :] ** 2, rtol=1e-14, atol=0)


@pytest.mark.parametrize("bufferSize,up", [(1024, 4), (7, 3), (10, 1)])
def test_ref_resampler_all_pass(bufferSize, up):
    x = rng.standard_normal(bufferSize)
    N = bufferSize * up
    out = S.resampler(x, up, np.ones(N, np.complex128))
    c = np.zeros(N)
    c[::up] = x
    assert np.max(np.abs(out - 2 * up * np.fft.ifft(np.fft.fft(c)).real)) == 0
    assert np.max(np.abs(out - 2 * up * c)) < 1e-13 * np.max(np.abs(x)) * 2 * up
