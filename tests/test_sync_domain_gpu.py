"""SyncXY on the MI355X over the whole domain tsdr_sync_create accepts (sync_cases.py): every size-dependent branch of
k_proj / k_beta<4> / k_beta<8>, the per-lane IEEE re-run, NaN / Inf / subnormal / overflowing / negative / tied beta, the
stale-s_y hand-over across all of them, and the Float64 twin; plus fill_beta and circshift_neg at their edges.

There is no tolerance in this file: (s_y, s_x) equal the reference's and beta_x / beta_y are bit-identical to it (NaN == NaN).
The reference is the oracle (Float32) and f64_ref.SyncXY64 (Float64); test_sync_domain_host.py holds both to the
conditions that make each image exercise its edge.
"""
import functools

import numpy as np
import pytest

import f64_ref as R
import oracle_lib as O
import sync_cases as K
from test_f64_gpu import _same, _ulps
from test_frame_path_gpu import assert_bitexact

pytestmark = pytest.mark.gpu

F64 = np.float64


def assert_same64(got, want, what):
    """Float64, bit for bit.  Where the bits differ the only licence is a NaN's payload (numpy and the GPU produce different
    ones): _ulps asserts that the NaN patterns agree and must find distance 0, and the signs of zeros must agree too.
    (In chunks: the largest fill_beta result is 515 MB.)"""
    assert got.shape == want.shape and got.dtype == want.dtype == F64, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    assert got.flags.f_contiguous and want.flags.f_contiguous, what
    if _same(got, want):
        return
    a, b = got.ravel(order="K"), want.ravel(order="K")
    step = 1 << 22
    for i in range(0, a.size, step):
        ca, cb = a[i:i + step], b[i:i + step]
        d = _ulps(ca, cb)
        assert d == 0, f"{what}: differs by {d} ulp in elements [{i}, {i + ca.size})"
        assert np.array_equal(np.signbit(ca) | np.isnan(ca), np.signbit(cb) | np.isnan(cb)), f"{what}: sign of a zero"


def _sequence(y_t, x_t):
    """the vsync calls of one state: every family in its fixed order, `noise` once more (it returns the s_y the last family
    left pending), a reset, and one more call"""
    fams = K.families(y_t, x_t)
    return [(f, False) for f in fams] + [("noise", False), ("zero-band", True)]


@functools.lru_cache(maxsize=1)   # shared by the two beta_waves values of a size (the largest beta_x is 29 MB per call)
def _oracle_run(y_t, x_t):
    o = O.SyncXY(y_t, x_t)
    out = []
    for fam, reset in _sequence(y_t, x_t):
        if reset:
            o.reset()
        img = K.image(fam, y_t, x_t)
        idx = o.vsync(img)
        out.append((fam, reset, img, idx, o.beta("x"), o.beta("y")))
    for a in out:
        for v in a[2:]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return (o.wmin_y, o.wmax_y, o.wmin_x, o.wmax_x), out


@pytest.mark.parametrize("y_t,x_t,beta_waves", [(y, x, bw) for (y, x) in K.SIZES for bw in (4, 8)])
def test_vsync_domain(ctx, tsdr, y_t, x_t, beta_waves):
    bnd, want = _oracle_run(y_t, x_t)
    ctx.set_option("beta_waves", beta_waves)
    g = None
    try:
        g = tsdr.SyncXY(ctx, y_t, x_t)
        assert (g.wmin_y, g.wmax_y, g.wmin_x, g.wmax_x) == bnd
        compared = 0
        for k, (fam, reset, img, idx, bx, by) in enumerate(want):
            if reset:
                g.reset()
            got = g.vsync(img)
            what = f"{y_t}x{x_t} beta_waves={beta_waves} call {k} ({fam})"
            assert got == idx, f"{what}: (s_y, s_x) {got} vs oracle {idx}"
            if k == 0 or reset:
                assert got[0] == 1, what   # beta_y is still all zero (FrameSynchronisation.jl:66)
            assert_bitexact(g.beta("x"), bx, f"{what}: beta_x")
            assert_bitexact(g.beta("y"), by, f"{what}: beta_y")
            compared += bx.size + by.size
        print(f"vsync domain {y_t}x{x_t} beta_waves={beta_waves}: {len(want)} calls, {compared} beta values compared")
    finally:
        ctx.set_option("beta_waves", 4)
        if g is not None:
            g.close()


@pytest.mark.parametrize("y_t,x_t", K.SIZES_F64)
def test_vsync_domain_f64(ctx, tsdr, y_t, x_t):
    g, r = tsdr.SyncXY(ctx, y_t, x_t, dtype=F64), R.SyncXY64(y_t, x_t)
    compared = 0
    try:
        with np.errstate(all="ignore"):
            for k, (fam, reset) in enumerate(_sequence(y_t, x_t)):
                if reset:
                    g.reset(); r.reset()
                img = K.image(fam, y_t, x_t, F64)
                got, want = g.vsync(img), r.vsync(img)
                what = f"f64 {y_t}x{x_t} call {k} ({fam})"
                assert got == want, f"{what}: (s_y, s_x) {got} vs restatement {want}"
                if k == 0 or reset:
                    assert got[0] == 1, what
                for name, a, b in (("beta_x", g.beta("x"), r.beta_x), ("beta_y", g.beta("y"), r.beta_y)):
                    assert_same64(a, b, f"{what}: {name}")
                    compared += a.size
        print(f"vsync domain f64 {y_t}x{x_t}: {k + 1} calls, {compared} beta values compared")
    finally:
        g.close()


# ---- fill_beta --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,w_min,w_max", K.FILL_BETA_CASES)
def test_fill_beta_domain(ctx, n, w_min, w_max):
    for kind in K.FILL_BETA_INPUTS:
        cv = K.fill_beta_input(kind, n, w_min)
        assert_bitexact(ctx.fill_beta(cv, n, w_min, w_max), O.fill_beta(cv, n, w_min, w_max), f"fill_beta {kind} n={n}")


@pytest.mark.parametrize("n,w_min,w_max", K.FILL_BETA_CASES)
def test_fill_beta_domain_f64(ctx, n, w_min, w_max):
    for kind in K.FILL_BETA_INPUTS:
        cv = K.fill_beta_input(kind, n, w_min, F64)
        with np.errstate(all="ignore"):
            want = R.fill_beta(cv, n, w_min, w_max)
        got = ctx.fill_beta(cv, n, w_min, w_max, dtype=F64)
        assert_same64(got, want, f"fill_beta f64 {kind} n={n}")


def test_fill_beta_refuses_a_vector_longer_than_lds_on_the_host(ctx):
    """n * 4 bytes of c_v live in LDS: n = 16384 is the largest the Float32 kernel can be launched with.  A longer vector is
    refused by the entry point, with the limit in the message, before anything is launched (the refused call issues no launch);
    the Float64 form reads c_v from memory and has no such limit."""
    n = K.FILL_BETA_MAX_N + 1
    cv = K.fill_beta_input("noise", n, 1)
    with pytest.raises(AssertionError) as e:   # TSDR_EINVAL (a refused launch would be TSDR_EHIP: TempestHIPError)
        ctx.fill_beta(cv, n, 1, 1)
    msg = str(e.value)
    assert str(K.FILL_BETA_MAX_N) in msg and "fill_beta" in msg, msg
    assert_same64(ctx.fill_beta(cv.astype(F64), n, 1, 2, dtype=F64), R.fill_beta(cv.astype(F64), n, 1, 2), "fill_beta f64 n=16385")
    small = K.fill_beta_input("noise", 64, 2)   # the context is as usable as before
    assert_bitexact(ctx.fill_beta(small, 64, 2, 16), O.fill_beta(small, 64, 2, 16), "fill_beta after the refusal")


# ---- circshift_neg ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", K.CIRCSHIFT_SIZES)
def test_circshift_domain(ctx, h, w):
    img = np.asfortranarray(np.random.default_rng([h, w]).random((h, w), dtype=np.float32))
    img[h // 2, w // 2] = np.nan
    img[0, 0], img[h - 1, w - 1] = -0.0, np.inf
    for s_y, s_x in K.circshift_shifts(h, w):
        got = ctx.circshift_neg(img, s_y, s_x)
        assert_bitexact(got, np.roll(img, (-s_y, -s_x), axis=(0, 1)), f"circshift {h}x{w} by ({s_y}, {s_x}) vs np.roll")
        assert_bitexact(got, O.circshift_neg(img, s_y, s_x), f"circshift {h}x{w} by ({s_y}, {s_x}) vs oracle")
