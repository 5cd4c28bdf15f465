"""GPU tests of the display export (include/tempest_hip_display.h): bytes and ranges against tests/display_ref.py BIT FOR BIT (`==`
on the floats, so the two zeros are equal), over the ROIs, alignments and path switches of the kernels (16-byte / dword loads,
dword / byte stores, heads and tails), every mode and flag, special pictures, every refusal, the host form, and one end-to-end
case behind the full-size frame loop.  Every device pointer sits inside a guarded arena (tests/dptr_util.py); `out` sits at a BYTE
offset inside a larger payload whose remaining bytes must keep their sentinel.

Pictures are made once per shape (functools caches); nothing modifies them."""
import ctypes as C
import functools

import numpy as np
import pytest

import display_ref as R
import dptr_util as D

pytestmark = pytest.mark.gpu

EINVAL = -1
F = np.float32
MODES = (R.FIXED, R.MINMAX, R.PERCENTILE)
FLAGS = (0, R.INVERT, R.SHARED, R.INVERT | R.SHARED)
P_DEFAULT = (0.02, 0.98)
FIXED_RANGE = (-1.5, 6.0)


@functools.lru_cache(maxsize=None)
def _pics(h, w, n, seed=0):
    """n pictures (row f: picture f, column-major): positive amplitudes of mixed magnitude, each picture on a level of its own (so
    that a shared range differs from the pictures' own)"""
    rng = np.random.default_rng(1000 * h + w + seed)
    a = (np.abs(rng.normal(2.0, 1.0, (n, h * w))) * np.exp(rng.uniform(-1, 1, (n, h * w))) + np.arange(n)[:, None]).astype(F)
    a.setflags(write=False)
    return a


def _mats(flat, h, w):
    return [flat[f].reshape((h, w), order="F") for f in range(len(flat))]


def _sentinel_bytes(a):
    return D.sentinel_words(a.size // 4)[a.lead // 4: (a.lead + a.payload) // 4].view(np.uint8)


class Call:
    """one tsdr_display_u8_d call inside an Arenas block: out at byte offset `off` of a larger payload, ranges in an arena of
    their own; verify() compares with the reference after A.check()"""

    def __init__(self, ctx, A, img, flat, h, w, roi, mode, flags=0, p=P_DEFAULT, lohi=FIXED_RANGE, off=0, want_out=True, want_rng=True,
                 n=None):
        self.flat, self.h, self.w, self.roi, self.mode, self.flags, self.p, self.lohi, self.off = flat, h, w, roi, mode, flags, p, lohi, off
        self.n = len(flat) if n is None else n
        i0, j0, rh, rw = roi
        self.nbytes = self.n * rh * rw
        self.out = A.output("out", (off + self.nbytes + 8 + 3) // 4 * 4, 0) if want_out else None
        self.rng = A.output("ranges", max(self.n, 1) * 8, 4) if want_rng else None
        ctx.call("tsdr_display_u8_d", img.ptr, self.n, h, w, i0, j0, rh, rw, mode, C.c_float(lohi[0]), C.c_float(lohi[1]), C.c_double(p[0]),
                 C.c_double(p[1]), flags, C.c_void_p(self.out.addr + off) if want_out else None, self.rng.ptr if want_rng else None)

    def got(self):
        i0, j0, rh, rw = self.roi
        out = rng = None
        if self.out is not None:
            raw, sent = self.out.get(np.uint8), _sentinel_bytes(self.out)
            lo, hi = self.off, self.off + self.nbytes
            assert np.array_equal(raw[:lo], sent[:lo]), f"bytes in front of out (offset {self.off}) were written"
            assert np.array_equal(raw[hi:], sent[hi:]), f"bytes behind out (offset {self.off}) were written"
            out = np.stack([raw[lo:hi].reshape(self.n, rh * rw)[f].reshape((rh, rw), order="F") for f in range(self.n)])
        if self.rng is not None:
            rng = self.rng.get(F).reshape(-1, 2)[:self.n]
        return out, rng

    def verify(self):
        what = (self.h, self.w, self.roi, self.mode, self.flags, self.p, self.off)
        want_out, want_rng = R.display(_mats(self.flat[:self.n], self.h, self.w), self.roi, self.mode, self.lohi[0], self.lohi[1], self.p,
                                       bool(self.flags & R.INVERT), bool(self.flags & R.SHARED))
        out, rng = self.got()
        if rng is not None:
            assert np.all(rng == want_rng), (what, rng.tolist(), want_rng.tolist())
        if out is not None:
            bad = np.argwhere(out != want_out)
            assert bad.size == 0, (what, len(bad), bad[:4].tolist(), out[tuple(bad[0])], want_out[tuple(bad[0])])
        return out, rng


def _run(ctx, flat, h, w, specs, phase=0):
    """specs: dicts of Call's keyword arguments, all run on one upload of `flat` at pointer phase `phase`, then checked"""
    with D.Arenas(ctx) as A:
        img = A.input("images", flat, phase)
        calls = [Call(ctx, A, img, flat, h, w, **s) for s in specs]
        A.check()
        return [c.verify() for c in calls]


# ---------------------------------------------------------------- ROIs, modes, flags
@pytest.mark.parametrize("roi", [(0, 0, 77, 131), (1, 2, 70, 100), (76, 130, 1, 1), (0, 5, 77, 1), (3, 0, 1, 131)])
def test_rois_every_mode_and_flag(ctx, roi):
    flat = _pics(77, 131, 3)
    specs = [dict(roi=roi, mode=m, flags=fl, off=(m + fl) % 4) for m in MODES for fl in FLAGS]
    res = _run(ctx, flat, 77, 131, specs, phase=4 * (roi[0] % 2))
    # SHARED: every picture reports one range; INVERT of the same call is 255 - q where the range is not degenerate
    by = {(s["mode"], s["flags"]): r for s, r in zip(specs, res)}
    for m in MODES:
        assert np.all(by[(m, R.SHARED)][1] == by[(m, R.SHARED)][1][0])
        if roi[2] * roi[3] > 1:
            assert np.array_equal(by[(m, R.INVERT)][0], 255 - by[(m, 0)][0])
    assert np.all(by[(R.FIXED, 0)][1] == np.array(FIXED_RANGE, F)), "FIXED echoes its arguments"


@pytest.mark.parametrize("phase", [0, 4])
@pytest.mark.parametrize("i0", [0, 3, 4])
def test_row_paths_heads_and_tails(ctx, i0, phase):
    """80x64 at pointer phase 0: columns start on 16-byte boundaries (16-byte loads; i0 = 3 shifts the quads by one row, i0 = 4 by a
    whole quad); phase 4 (images at base + 4): dword loads.  rh in {80, 77, 76, 5}: whole quads, tails of 1 and 0 rows, one
    partial quad; out at byte offsets 0 .. 3, so a column's first byte falls on every dword phase."""
    flat = _pics(80, 64, 2)
    specs = [dict(roi=(i0, 1, rh, 61), mode=m, off=off, flags=fl)
             for k, rh in enumerate(r for r in (80, 77, 76, 5) if i0 + r <= 80)
             for m, off, fl in ((R.MINMAX, k % 4, 0), (R.PERCENTILE, (k + 1) % 4, R.SHARED), (R.FIXED, (k + 2) % 4, R.INVERT),
                                (R.PERCENTILE, (k + 3) % 4, 0))]
    _run(ctx, flat, 80, 64, specs, phase=phase)


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_out_at_every_byte_offset(ctx, off):
    flat = _pics(77, 131, 3)
    specs = [dict(roi=roi, mode=R.PERCENTILE, off=off) for roi in ((1, 2, 70, 100), (0, 0, 77, 131), (2, 3, 72, 9))]
    _run(ctx, flat, 77, 131, specs, phase=4)


@pytest.mark.parametrize("roi", [(0, 0, 600, 800), (60, 80, 480, 640), (61, 83, 479, 333)])
def test_several_workgroups_per_picture(ctx, roi):
    """600x800, n = 2: 30 workgroups of the statistics pass, 15 of the histogram pass, 235 of the mapping pass per picture"""
    flat = _pics(600, 800, 2)
    _run(ctx, flat, 600, 800, [dict(roi=roi, mode=R.PERCENTILE, off=1), dict(roi=roi, mode=R.MINMAX, flags=R.SHARED),
                               dict(roi=roi, mode=R.FIXED, flags=R.INVERT, off=2)])


# ---------------------------------------------------------------- special pictures
@functools.lru_cache(maxsize=None)
def _special(kind):
    h, w = 64, 80
    rng = np.random.default_rng(5)
    if kind == "nan_inf":
        a = rng.normal(0.0, 3.0, (3, h * w)).astype(F)
        a[:, ::7] = np.nan
        a[0, 3::11] = np.inf
        a[1, 5::13] = -np.inf
        a[2, 1::3] = np.inf
    elif kind == "no_finite":                 # picture 1 holds no finite pixel at all; 0 and 2 are ordinary
        a = rng.normal(1.0, 3.0, (3, h * w)).astype(F)
        a[1] = np.nan
        a[1, ::2] = np.inf
        a[1, 1::4] = -np.inf
    elif kind == "constant":                  # picture 0 constant, picture 1 constant with NaN holes, picture 2 all zeros of both signs
        a = np.full((3, h * w), 2.5, F)
        a[1, ::5] = np.nan
        a[2] = 0.0
        a[2, ::2] = -0.0
    elif kind == "two_valued":                # everything in bins 0 and 4095
        a = np.where(rng.random((3, h * w)) < 0.3, F(-7.25), F(100.5)).astype(F)
        a[1] = np.where(rng.random(h * w) < 0.995, F(1.0), F(2.0))
        a[2, :] = F(3.0)
        a[2, 17] = F(1000.0)                  # constant plus one outlier
    elif kind == "ramp":                      # integers 0 .. 4095 repeated: values on bin edges (d = 4095), and 0 .. 4096 (d = 4096, wd = 1)
        a = np.empty((3, h * w), F)
        a[0] = np.tile(np.arange(4096), 2)[: h * w][rng.permutation(h * w)]
        a[1] = rng.integers(0, 4097, h * w)
        a[1, :2] = (0, 4096)
        a[2] = np.arange(h * w) % 4096
    elif kind == "tiny":                      # subnormal amplitudes: IEEE f32 means they are not flushed (0 .. 1.1e-38, normals start at 1.18e-38)
        a = (rng.random((3, h * w)) * 1.1e-38).astype(F)
        a[1] *= F(0.01)
        a[2, ::3] = 0.0
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("agg", [0, 1])
@pytest.mark.parametrize("kind", ["nan_inf", "no_finite", "constant", "two_valued", "ramp", "tiny"])
def test_special_pictures(ctx, kind, agg):
    """agg: the histogram pass's two forms (option "display_hist_agg": one LDS add per lane, or one per wave whose lanes agree)"""
    ctx.set_option("display_hist_agg", agg)
    try:
        _special_pictures(ctx, kind)
    finally:
        ctx.set_option("display_hist_agg", 0)


def _special_pictures(ctx, kind):
    flat = _special(kind)
    specs = [dict(roi=(0, 0, 64, 80), mode=R.PERCENTILE, p=p, flags=fl) for p in (P_DEFAULT, (0.0, 1.0), (0.5, 0.5)) for fl in (0, R.SHARED)]
    specs += [dict(roi=(0, 0, 64, 80), mode=R.MINMAX, flags=fl) for fl in FLAGS]
    specs += [dict(roi=(3, 1, 57, 70), mode=R.PERCENTILE, flags=R.INVERT, off=3), dict(roi=(0, 0, 64, 80), mode=R.FIXED, lohi=(0.0, 4095.0))]
    if kind == "tiny":                        # s = 255 / 1e-36 is finite: a subnormal pixel v gives q = v * 2.55e38 = 0 .. 2.8
        specs.append(dict(roi=(0, 0, 64, 80), mode=R.FIXED, lohi=(0.0, 1e-36)))
    res = _run(ctx, flat, 64, 80, specs)
    if kind == "tiny":
        assert sorted(set(res[-1][0][0].ravel().tolist())) == [0, 1, 2, 3], "subnormal inputs are kept, not flushed to zero"
        assert not res[6][0].any() and np.all(res[6][1][:, 1] > 0), "mx - mn is subnormal: 255 / dd overflows, every byte 0"
    if kind == "no_finite":
        out, rng = res[6]                     # MINMAX, no flags
        assert np.all(rng[1] == 0) and not out[1].any() and out[0].any()
    if kind == "constant":
        assert not res[0][0].any() and not res[6][0].any() and res[6][1].tolist() == [[2.5, 2.5], [2.5, 2.5], [0.0, 0.0]]
    if kind == "ramp":
        assert res[2][1][1].tolist() == [0.0, 4096.0], "p = (0, 1) gives exactly (mn, mx)"


def test_more_pictures_than_a_workgroup_has_lanes(ctx):
    """300 pictures of 3x5: one workgroup per picture in every pass, 300 groups -- or, SHARED, one group whose range
    k_display_pick's 256 lanes write for all 300 pictures"""
    flat = _pics(3, 5, 300)
    _run(ctx, flat, 3, 5, [dict(roi=roi, mode=m, flags=fl, off=fl + 1) for roi in ((0, 0, 3, 5), (1, 1, 2, 3)) for m in MODES for fl in (0, R.SHARED)],
         phase=4)


def test_degenerate_fixed_ranges_give_zeros(ctx):
    flat = _pics(77, 131, 3)
    specs = [dict(roi=(0, 0, 77, 131), mode=R.FIXED, lohi=lohi, flags=fl)
             for lohi in ((1.0, 1.0), (2.0, 1.0), (-np.inf, 1.0), (0.0, np.inf), (0.0, 1e-42)) for fl in (0, R.INVERT)]
    for out, rng in _run(ctx, flat, 77, 131, specs):
        assert not out.any()


def test_ranges_only_and_bytes_only(ctx):
    flat = _pics(77, 131, 3)
    roi = (1, 2, 70, 100)
    specs = [dict(roi=roi, mode=m, flags=fl, want_out=False) for m in MODES for fl in (0, R.SHARED)]
    specs += [dict(roi=roi, mode=m, want_rng=False, off=1) for m in MODES]
    _run(ctx, flat, 77, 131, specs)


def test_back_to_back_calls_do_not_see_each_others_scratch(ctx):
    """two PERCENTILE calls with different inputs (then a MINMAX one on fewer pictures) back to back on one stream, no
    synchronisation in between: a histogram or a minimum that survived the first call shows in the second"""
    a, b = _pics(77, 131, 3), _pics(77, 131, 3, seed=9) * F(0.25) - F(3.0)
    roi = (1, 2, 70, 100)
    with D.Arenas(ctx) as A:
        ia, ib = A.input("a", a, 0), A.input("b", b, 0)
        calls = [Call(ctx, A, ia, a, 77, 131, roi, R.PERCENTILE), Call(ctx, A, ib, b, 77, 131, roi, R.PERCENTILE),
                 Call(ctx, A, ia, a, 77, 131, roi, R.PERCENTILE, flags=R.SHARED), Call(ctx, A, ib, b, 77, 131, roi, R.MINMAX, n=2),
                 Call(ctx, A, ia, a, 77, 131, roi, R.PERCENTILE)]
        A.check()
        res = [c.verify() for c in calls]
    assert np.array_equal(res[0][0], res[4][0]) and np.all(res[0][1] == res[4][1]), "the same input gives the same bytes"
    assert not np.array_equal(res[0][0], res[1][0])


def test_zero_pictures_touch_nothing(ctx):
    flat = _pics(77, 131, 3)
    with D.Arenas(ctx) as A:
        img = A.input("images", flat, 0)
        c = Call(ctx, A, img, flat, 77, 131, (0, 0, 77, 131), R.PERCENTILE, n=0)
        assert ctx.lib.tsdr_display_u8_d(ctx.h, None, 0, 0, 0, -1, -1, 0, 0, 9, 0.0, 0.0, 2.0, -1.0, 64, None, None) == 0
        A.check()
        assert np.array_equal(c.out.get(np.uint8), _sentinel_bytes(c.out)) and np.array_equal(c.rng.get(np.uint8), _sentinel_bytes(c.rng))


# ---------------------------------------------------------------- refusals
def test_every_refusal_leaves_the_outputs_alone(ctx):
    h, w, n = 77, 131, 3
    flat = _pics(h, w, n)
    nan = float("nan")
    base = dict(images=None, n=n, h=h, w=w, i0=1, j0=2, rh=70, rw=100, mode=R.PERCENTILE, lo=0.0, hi=1.0, p_lo=0.02, p_hi=0.98, flags=0, out=None,
                rng=None)
    order = ["images", "n", "h", "w", "i0", "j0", "rh", "rw", "mode", "lo", "hi", "p_lo", "p_hi", "flags", "out", "rng"]
    with D.Arenas(ctx) as A:
        img = A.input("images", flat, 0)
        out, rng = A.output("out", n * 70 * 100, 0), A.output("ranges", n * 8, 4)
        base.update(images=img.addr, out=out.addr, rng=rng.addr)
        changes = [dict(images=None), dict(out=None, rng=None), dict(h=0), dict(w=-1), dict(rh=0), dict(rw=-3), dict(i0=-1), dict(j0=-1),
                   dict(i0=8), dict(j0=32), dict(rh=78, i0=0), dict(rw=132, j0=0), dict(h=46341, w=46341), dict(n=-1), dict(mode=3), dict(mode=-1),
                   dict(flags=4), dict(flags=-1), dict(p_lo=nan), dict(p_hi=nan), dict(p_lo=-0.01), dict(p_hi=1.01), dict(p_lo=0.6, p_hi=0.4),
                   dict(mode=R.FIXED, lo=nan), dict(mode=R.FIXED, hi=nan), dict(images=img.addr + 2), dict(rng=rng.addr + 2),
                   dict(rng=rng.addr + 1)]
        for form in ("tsdr_display_u8_d", "tsdr_display_u8"):
            for change in changes:
                a = [dict(base, **change)[k] for k in order]
                rc = getattr(ctx.lib, form)(ctx.h, *a)
                assert rc == EINVAL, (form, change, rc)
                assert b"display_u8" in ctx.lib.tsdr_last_error(ctx.h), change
        assert ctx.lib.tsdr_display_u8_d(None, *[base[k] for k in order]) == EINVAL
        A.check()                             # every payload and every guard word as uploaded
        assert np.array_equal(out.get(np.uint8), _sentinel_bytes(out)) and np.array_equal(rng.get(np.uint8), _sentinel_bytes(rng))
    with pytest.raises(ValueError):
        ctx.display_u8(_mats(flat, h, w), mode="gamma")
    # ... and the context still works; an unaligned out alone is no refusal
    _run(ctx, flat, h, w, [dict(roi=(1, 2, 70, 100), mode=R.PERCENTILE, off=3)])


# ---------------------------------------------------------------- the host form, the Python layer
def test_host_form_equals_device_form(ctx, tsdr):
    h, w = 77, 131
    flat = _pics(h, w, 3)
    mats = _mats(flat, h, w)
    for roi in (None, (1, 2, 70, 100)):
        for mode, name in ((R.FIXED, "fixed"), (R.MINMAX, "minmax"), (R.PERCENTILE, "percentile")):
            for fl in FLAGS:
                out, rng = ctx.display_u8(mats, roi, name, FIXED_RANGE[0], FIXED_RANGE[1], P_DEFAULT, bool(fl & R.INVERT), bool(fl & R.SHARED))
                want_out, want_rng = R.display(mats, roi, mode, FIXED_RANGE[0], FIXED_RANGE[1], P_DEFAULT, bool(fl & R.INVERT), bool(fl & R.SHARED))
                assert out.dtype == np.uint8 and np.array_equal(out, want_out) and np.all(rng == want_rng), (roi, name, fl)
    dev = _run(ctx, flat, h, w, [dict(roi=(1, 2, 70, 100), mode=R.PERCENTILE, flags=R.SHARED)])[0]
    host = tsdr.display_u8(ctx, mats, (1, 2, 70, 100), "percentile", p=P_DEFAULT, shared=True)
    assert np.array_equal(dev[0], host[0]) and np.all(dev[1] == host[1])
    # the raw host entry point with out == NULL and with ranges_out == NULL
    r = np.full((3, 2), 7, F)
    assert ctx.lib.tsdr_display_u8(ctx.h, flat.ctypes.data, 3, h, w, 0, 0, h, w, R.MINMAX, 0.0, 0.0, 0.0, 1.0, 0, None, r.ctypes.data) == 0
    assert np.all(r == R.display(mats, None, R.MINMAX)[1])
    o = np.zeros(3 * h * w, np.uint8)
    assert ctx.lib.tsdr_display_u8(ctx.h, flat.ctypes.data, 3, h, w, 0, 0, h, w, R.MINMAX, 0.0, 0.0, 0.0, 1.0, 0, o.ctypes.data, None) == 0
    assert np.array_equal(o.reshape(3, -1), np.stack([m.reshape(-1, order="F") for m in R.display(mats, None, R.MINMAX)[0]]))


# ---------------------------------------------------------------- behind the full-size frame loop
def test_display_of_the_full_size_state(ctx, tsdr):
    """Context.frames_hires_d on the 125x160 geometry of tests/test_hires_gpu.py, then display_u8_d on hires_state as the loop
    left it on the device: an active-area ROI, percentiles (0.01, 0.99); compared with the reference applied to the downloaded
    state.  The statistics are the ROI's: the range lies inside the ROI's own extremes."""
    import test_hires_gpu as HG
    g = HG.GEOMS["125x160"]
    iq, _, _, S = HG._capture("125x160")
    y_t, x_t = g["y_t"], g["x_t"]
    roi = (10, 16, 100, 128)
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, 0)
        d_st = HG._inout(A, "imageOut", np.zeros(600 * 800, F), 0)
        d_hs = HG._inout(A, "hires_state", np.zeros(y_t * x_t, F), 12)
        out, rng = A.output("out", roi[2] * roi[3] + 4, 0), A.output("ranges", 8, 4)
        n = ctx.frames_hires_d(tsdr.SyncXY(ctx, 600, 800), d_iq.addr, "cf32", 1.0, iq.size, S, y_t, x_t, HG.ALPHA, True, d_st.addr, HG.ALPHA_H,
                               d_hs.addr, None, None)
        ctx.display_u8_d(d_hs.addr, 1, y_t, x_t, out.addr + 1, roi, "percentile", p=(0.01, 0.99), ranges_out=rng.addr)
        A.check()
        state = d_hs.get(F, (y_t, x_t), "F")
        got = out.get(np.uint8)[1:1 + roi[2] * roi[3]].reshape((roi[2], roi[3]), order="F")
        got_rng = rng.get(F)
    assert n == g["nfr"] and state.max() > 0
    want, want_rng = R.display([state], roi, R.PERCENTILE, p=(0.01, 0.99))
    assert np.array_equal(got, want[0]) and np.all(got_rng == want_rng[0])
    c = R.crop(state, roi)
    assert c.min() <= got_rng[0] < got_rng[1] <= c.max() and got.min() == 0 and got.max() == 255
