"""Float64 / ComplexF64 per-function API, CPU side: the numpy restatement (f64_ref.py) pinned against analytic answers and
against the f32 oracle on f32-representable input, and static checks that the header and the Julia shim carry the `_f64`
surface (the prototype-matching test of test_julia_shim_static.py then covers the new ccalls)."""
import math
import os
import re

import numpy as np
import pytest

import f64_ref as R
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rng = np.random.default_rng(64)

F64_SYMBOLS = [
    "tsdr_am_demod_f64", "tsdr_am_demod_f64_d", "tsdr_invert_am_f64", "tsdr_invert_am_f64_d", "tsdr_fm_demod_f64",
    "tsdr_fm_demod_f64_d", "tsdr_abs2_f64", "tsdr_abs2_f64_d", "tsdr_resize1d_f64", "tsdr_resize1d_f64_d",
    "tsdr_sig_to_image_f64", "tsdr_sig_to_image_f64_d", "tsdr_resize2d_f64", "tsdr_resize2d_f64_d", "tsdr_downgrade_f64",
    "tsdr_downgrade_f64_d", "tsdr_naive_resample_f64", "tsdr_naive_resample_f64_d", "tsdr_sync_create_f64", "tsdr_vsync_f64",
    "tsdr_vsync_f64_d", "tsdr_sync_beta_f64", "tsdr_fill_beta_f64", "tsdr_autocorr_f64", "tsdr_autocorr_f64_d",
    "tsdr_spectrum_f64", "tsdr_spectrum_f64_d",
]

# shim function -> the _f64 symbol its Float64 / ComplexF64 method calls, and the element pointer type it passes
SHIM_F64 = {
    "amDemod": ("tsdr_am_demod_f64", "Ptr{ComplexF64}"),
    "invert_amDemod": ("tsdr_invert_am_f64", "Ptr{ComplexF64}"),
    "fmDemod": ("tsdr_fm_demod_f64", "Ptr{ComplexF64}"),
    "hip_abs2": ("tsdr_abs2_f64", "Ptr{ComplexF64}"),
    "sig_to_image": ("tsdr_sig_to_image_f64", "Ptr{Float64}"),
    "downgradeImage": ("tsdr_downgrade_f64", "Ptr{Float64}"),
    "naiveResampler": ("tsdr_naive_resample_f64", "Ptr{Float64}"),
    "hip_imresize": ("tsdr_resize1d_f64", "Ptr{Float64}"),
    "calculate_autocorrelation": ("tsdr_autocorr_f64", "Ptr{Float64}"),
    "getSpectrum": ("tsdr_spectrum_f64", "Ptr{Float64}"),
    "SyncXY": ("tsdr_sync_create_f64", "Ptr{Ptr{Cvoid}}"),
    "vsync": ("tsdr_vsync_f64", "Ptr{Float64}"),
    "hip_sync_beta": ("tsdr_sync_beta_f64", "Ptr{Float64}"),
    "hip_fill_beta": ("tsdr_fill_beta_f64", "Ptr{Float64}"),
}


# ---- static checks ---------------------------------------------------------------------------------------------------
def test_header_declares_every_f64_symbol():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tempest_hip.h")).read(), flags=re.S)
    missing = [s for s in F64_SYMBOLS if not re.search(r"\b" + s + r"\s*\(", src)]
    assert not missing, missing


def _shim_methods(src, name):
    """bodies of every `function name(...)` definition of the shim (inner constructors included)"""
    out = []
    for m in re.finditer(r"^\s*function " + re.escape(name) + r"\((.*?)\)(?: where [^\n]*)?(?:\s+#[^\n]*)?$", src, flags=re.M):
        end = src.find("\nend", m.end())
        inner = src.find("\n    end\n", m.end())
        stop = end if inner < 0 or src[m.start()] != " " else inner
        out.append((m.group(1), src[m.end(): stop]))
    return out


@pytest.mark.parametrize("name", sorted(SHIM_F64))
def test_shim_has_a_float64_method(name):
    src = open(os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP.jl")).read()
    sym, ptr = SHIM_F64[name]
    methods = _shim_methods(src, name)
    assert methods, f"no method {name} in the shim"
    hits = [body for sig, body in methods if re.search(r"\b(Float64|ComplexF64|T)\b", sig) and f":{sym}," in body]
    assert hits, f"{name}: no Float64 / ComplexF64 method calls {sym}"
    assert any(ptr in body for body in hits), f"{name}: the ccall of {sym} does not pass {ptr}"


def test_shim_keeps_other_element_types_a_method_error():
    src = open(os.path.join(ROOT, "tempestsdr.jl_amd", "julia", "TempestHIP.jl")).read()
    assert "T == Float32 || T == Float64 || throw(MethodError(SyncXY" in src
    for name in ("amDemod", "fmDemod", "invert_amDemod"):
        sigs = [s for s, _ in _shim_methods(src, name)]
        assert sorted(sigs) == ["sig::Array{ComplexF32}", "sig::Array{ComplexF64}"], sigs


def test_f64_prototypes_in_ctypes_table(tsdr):
    from tempestsdr_jl_amd import _lib
    names = set(_lib.exported_names())
    assert set(F64_SYMBOLS) <= names


def test_api_dtype_keyword_rejects_other_types(tsdr):
    api = tsdr.api
    assert api._is64(None) is False and api._is64(np.float64) is True
    with pytest.raises(AssertionError):
        api._is64(np.int16)
    with pytest.raises(AssertionError):
        api._c128(np.zeros(4, np.complex64), "amDemod")
    with pytest.raises(AssertionError):
        api._f64(np.zeros(4, np.float32), "imresize")


# ---- restatement pins: analytic ------------------------------------------------------------------------------------
def test_taps_are_the_normalised_gaussian():
    h = R.taps()
    assert h[0] == h[4] and h[1] == h[3]
    assert abs(sum(h) - 1.0) < 4e-16
    assert h[1] / h[2] == pytest.approx(math.exp(-2 / 25), rel=1e-15) and h[0] / h[2] == pytest.approx(math.exp(-8 / 25), rel=1e-15)


def test_fma_is_single_rounding():
    a = 1.0 + 2.0 ** -30
    # a*a = 1 + 2^-29 + 2^-60: the product alone rounds the 2^-60 away, the fused form keeps it
    assert R.fma(a, a, -1.0) == 2.0 ** -29 + 2.0 ** -60
    assert a * a - 1.0 == 2.0 ** -29


def test_fir_impulse_and_step_responses():
    h = R.taps()
    assert list(R.fir(h, [1.0, 0, 0, 0, 0, 0])) == h + [0.0]
    step = R.fir(h, np.ones(8))
    assert step[4] == pytest.approx(1.0, abs=3e-16) and all(step[i] <= step[i + 1] for i in range(4))


def test_sums_on_exact_integer_data():
    img = np.asfortranarray(rng.integers(0, 1000, (150, 70)).astype(np.float64))
    assert np.array_equal(R.col_sums(img), img.sum(axis=0))
    assert np.array_equal(R.row_sums(img), img.sum(axis=1))
    v = rng.integers(0, 1000, 333).astype(np.float64)
    assert R.sum64(v) == v.sum()


def test_argmax_first_maximum_nan_maximal():
    b = np.asfortranarray(np.array([[1.0, 5.0, 5.0], [2.0, 3.0, 5.0]]))
    assert R.argmax_col(b) == 2
    b[1, 2] = np.nan
    b[0, 0] = np.nan
    assert R.argmax_col(b) == 1


def test_resize_identities():
    x = rng.random(57)
    assert np.array_equal(R.resize1d(x, 57), x)
    assert np.array_equal(R.naive_resample([1.5, -2.0], 3), [1.5, 1.5, 1.5, -2.0, -2.0, -2.0])
    # a ramp sampled on the integers: every output lies on the line (the blend of two exact neighbours)
    ramp = np.arange(1, 101, dtype=np.float64)
    up = R.resize1d(ramp, 250)
    sf = 100 / 250
    want = np.clip(sf * np.arange(1, 251) + (0.5 - sf * 0.5), 1, 100)
    assert np.max(np.abs(up - want)) < 1e-13
    img = np.asfortranarray(rng.random((20, 30)))
    assert np.array_equal(R.resize2d(img, 20, 30), img)


def test_sync_stale_sy_and_reset():
    y_t, x_t = 77, 131
    img = np.asfortranarray(rng.random((y_t, x_t)))
    img[:, 40:50] = 0.0
    img[20:26, :] = 0.0
    s = R.SyncXY64(y_t, x_t)
    sy, sx = s.vsync(img)
    assert sy == 1 and sx == R.argmax_col(s.beta_x)     # a fresh state's beta_y is all zeros: findmax -> column 1
    pending = R.argmax_col(s.beta_y)
    assert s.vsync(img)[0] == pending and pending != 1   # the second call returns the first call's beta_y argmax
    s.reset()
    assert s.vsync(img)[0] == 1


# ---- restatement vs the f32 oracle on f32-representable input ------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(333, 41), (125, 500), (1000, 1000), (2, 7), (4097, 1024)])
def test_resize1d_rounds_to_the_oracle(n_in, n_out):
    x = rng.random(n_in, dtype=np.float32)
    got = R.resize1d(x.astype(np.float64), n_out).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), O.imresize1d(x, n_out).view(np.uint32))


@pytest.mark.parametrize("S,y_t,x_t", [(1200, 30, 40), (137, 30, 40), (3333, 70, 130), (26001, 125, 161)])
def test_sig_to_image_rounds_to_the_oracle(S, y_t, x_t):
    x = rng.random(S, dtype=np.float32)
    got = R.sig_to_image(x.astype(np.float64), y_t, x_t).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), O.sig_to_image(x, y_t, x_t).view(np.uint32))


@pytest.mark.parametrize("h,w,ho,wo", [(45, 64, 20, 30), (45, 64, 600, 800), (700, 900, 600, 800), (20, 30, 20, 30)])
def test_resize2d_rounds_to_the_oracle(h, w, ho, wo):
    img = np.asfortranarray(rng.random((h, w), dtype=np.float32))
    got = R.resize2d(img.astype(np.float64), ho, wo).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), O.imresize2d(img, (ho, wo)).view(np.uint32))


def test_sync_indices_agree_with_the_oracle_on_a_clear_band():
    y_t, x_t = 77, 131
    img = np.asfortranarray(rng.random((y_t, x_t), dtype=np.float32) * 0.1 + 1.0)
    img[:, 90:99] = 0.05
    img[60:64, :] = 0.05
    r, o = R.SyncXY64(y_t, x_t), O.SyncXY(y_t, x_t)
    for _ in range(3):
        assert r.vsync(img.astype(np.float64)) == o.vsync(img)
    b32 = o.beta("x").astype(np.float64)
    assert np.max(np.abs(r.beta_x - b32)) <= 1e-5 * np.max(np.abs(b32))
