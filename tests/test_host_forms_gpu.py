"""GPU tests: a host-pointer entry point is its device-pointer form plus staging (csrc/host_stage.h), so on the same input the two
give the same bits -- with every optional array present and absent, because what can go wrong in the staging is a byte count, a
slot, the order of the copies or a NULL case, not the arithmetic.  Shapes are the smallest the device forms' own tests use.

Where a state is documented as NOT READ (alpha == 0: fold, cfold, cstack) the host form must not upload it either: the staging slot
is first left holding another call's values, the host state is all NaN, the device form's state is zeros -- equal results show
that the state was neither uploaded nor read."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sync_cases as SC
from test_dptr_gpu import FRAME_CASE
from test_fold_gpu import CASES as FOLD_CASES

pytestmark = pytest.mark.gpu

NPX = 600 * 800
FOLD = FOLD_CASES["X"]                      # 8 x 16, three frames: the smallest geometry of tests/test_fold_gpu.py
Y, X, NR = 37, 53, 3                        # the rasters of raster_accumulate / raster_register
f32, f64, cf = C.c_float, C.c_double, np.complex64


@pytest.fixture(scope="module")
def hctx(tsdr):
    c = tsdr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def P(tsdr):
    from tempestsdr_jl_amd import api
    return api._ptr


class Dev:
    """device twins of host arrays, freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, a):
        """a device copy of `a`; None stays None"""
        if a is None:
            return None
        self.ptrs.append(self.ctx.upload(a))
        return self.ptrs[-1]

    def down(self, p, like):
        return None if p is None else self.ctx.download(p, like.shape, like.dtype)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.synchronize()
        for p in self.ptrs:
            self.ctx.dev_free(p)


def same(host, dev, what):
    assert (host is None) == (dev is None), what
    if host is not None:
        assert host.tobytes() == dev.tobytes(), f"{what}: host form and device form differ in {np.count_nonzero(host.view(np.uint8) != dev.view(np.uint8))} bytes"


def rng(*key):
    return np.random.default_rng([20260, *key])


# ---- frames -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_iq(synth):
    c = FRAME_CASE
    S = synth.samples_per_frame(c["Fs"], c["fv"])
    iq = synth.synth_leak(c["Fs"], c["x_t"], c["y_t"], c["fv"], S * c["nfr"])
    return S, iq


@pytest.mark.parametrize("do_align", [0, 1])
@pytest.mark.parametrize("want", list(itertools.product([0, 1], repeat=3)), ids=lambda w: "frames%d-raster%d-idx%d" % w)
def test_frames_equals_frames_d(tsdr, hctx, P, frame_iq, want, do_align):
    S, iq = frame_iq
    c, nb = FRAME_CASE, FRAME_CASE["nfr"]
    assert S == 33333 and iq.size == nb * S
    state0 = rng(1).random(NPX, dtype=np.float32)

    def outputs():
        return [state0.copy(), np.full(nb * NPX, -1, np.float32) if want[0] else None,
                np.full(nb * c["y_t"] * c["x_t"], -1, np.float32) if want[1] else None, np.full(2 * nb, -7, np.int32) if want[2] else None]

    hctx.set_precision("exact")
    sync_h, sync_d = tsdr.SyncXY(hctx, 600, 800), tsdr.SyncXY(hctx, 600, 800)
    try:
        host, n_h, n_d = outputs(), C.c_int(-1), C.c_int(-1)
        args = (iq.size, S, c["y_t"], c["x_t"], f32(0.1), do_align)
        hctx.call("tsdr_frames", C.c_void_p(sync_h.h), P(iq), *args, *[P(a) for a in host], C.byref(n_h))
        with Dev(hctx) as d:
            like = outputs()
            ptrs = [d.up(a) for a in like]
            hctx.call("tsdr_frames_d", C.c_void_p(sync_d.h), P(d.up(iq)), *args, *[P(p) for p in ptrs], C.byref(n_d))
            dev = [d.down(p, a) for p, a in zip(ptrs, like)]
        assert n_h.value == n_d.value == nb
        for h, v, what in zip(host, dev, ("state", "frames_out", "raster_out", "sync_idx")):
            same(h, v, what)
        assert not np.array_equal(host[0], state0)
        if want[2]:   # indices exist only with do_align: without, the caller's array is left alone by both forms
            assert (host[3] == -7).all() == (do_align == 0)
    finally:
        sync_h.close()
        sync_d.close()
        hctx.set_precision("fast")


# ---- rasters ----------------------------------------------------------------------------------------------------------------
def _rasters():
    r = rng(2)
    return r.random(NR * Y * X, dtype=np.float32), r.random(Y * X, dtype=np.float32), r.integers(-5, 6, 2 * NR).astype(np.int32)


@pytest.mark.parametrize("with_shifts", [False, True])
def test_raster_accumulate_equals_its_device_form(hctx, P, with_shifts):
    from tempestsdr_jl_amd import hires
    rasters, state0, shifts = _rasters()
    sh = shifts if with_shifts else None
    tail = (hires.UNITS["raster"], 600, 800, f32(0.3))
    host = state0.copy()
    hctx.call("tsdr_raster_accum", P(rasters), NR, Y, X, P(sh), *tail, P(host))
    with Dev(hctx) as d:
        p = d.up(state0)
        hctx.call("tsdr_raster_accum_d", P(d.up(rasters)), NR, Y, X, P(d.up(sh)), *tail, P(p))
        same(host, d.down(p, state0), "state")
    assert not np.array_equal(host, state0)


@pytest.mark.parametrize("have", list(itertools.product([0, 1], repeat=3)), ids=lambda w: "ref%d-shifts%d-scores%d" % w)
def test_raster_register_equals_its_device_form(hctx, P, have):
    from tempestsdr_jl_amd import hires, register
    rasters, ref, shifts = _rasters()
    ref, sh = ref if have[0] else None, shifts if have[1] else None
    d_y = d_x = 2
    tail = (hires.UNITS["raster"], 600, 800, d_y, d_x)

    def outputs():
        return np.full(2 * NR, -99, np.int32), np.full(NR * register.n_scores(d_y, d_x), -1.0) if have[2] else None

    host = outputs()
    hctx.call("tsdr_raster_register", P(rasters), NR, Y, X, P(ref), P(sh), *tail, P(host[0]), P(host[1]))
    with Dev(hctx) as d:
        like = outputs()
        ptrs = [d.up(a) for a in like]
        hctx.call("tsdr_raster_register_d", P(d.up(rasters)), NR, Y, X, P(d.up(ref)), P(d.up(sh)), *tail, P(ptrs[0]), P(ptrs[1]))
        dev = [d.down(p, a) for p, a in zip(ptrs, like)]
    same(host[0], dev[0], "shifts_out")
    same(host[1], dev[1], "scores")
    assert (host[0] != -99).all()


@pytest.mark.parametrize("have", [(1, 0), (0, 1), (1, 1)], ids=lambda w: "out%d-ranges%d" % w)
def test_display_u8_equals_its_device_form(hctx, P, have):
    from tempestsdr_jl_amd import display
    n, h, w, roi = 2, 24, 40, (3, 5, 10, 17)
    images = rng(3).random(n * h * w, dtype=np.float32)
    tail = (display.MODES["minmax"], f32(0.0), f32(1.0), f64(0.01), f64(0.99), 0)

    def outputs():
        return np.full(n * roi[2] * roi[3], 7, np.uint8) if have[0] else None, np.full(2 * n, -1, np.float32) if have[1] else None

    host = outputs()
    hctx.call("tsdr_display_u8", P(images), n, h, w, *roi, *tail, P(host[0]), P(host[1]))
    with Dev(hctx) as d:
        like = outputs()
        ptrs = [d.up(a) for a in like]
        hctx.call("tsdr_display_u8_d", P(d.up(images)), n, h, w, *roi, *tail, P(ptrs[0]), P(ptrs[1]))
        dev = [d.down(p, a) for p, a in zip(ptrs, like)]
    same(host[0], dev[0], "out")
    same(host[1], dev[1], "ranges_out")
    assert have[1] == 0 or (host[1] != -1).all()


# ---- fold, cfold, cstack --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fold_iq():
    from test_fold_gpu import _capture
    return _capture("X")[0]


def _fold_args(kind):
    """(host entry point, arguments between n and alpha) of fold / cfold / cstack at the X geometry"""
    c = FOLD
    geom = (c["F"], c["y"], c["x"])
    if kind == "fold":
        return "tsdr_fold_iq", (f64(c["t0"]), f64(c["T"])) + geom
    if kind == "cfold":
        return "tsdr_cfold_iq", (f64(c["t0"]), f64(c["T"]), f64(0.0625)) + geom
    return "tsdr_cstack_iq", (f64(c["t0"]), f64(c["T"]), f64(0.0625), f64(0.2)) + geom


@pytest.mark.parametrize("alpha", [0.0, 0.25])
@pytest.mark.parametrize("kind", ["fold", "cfold"])
def test_fold_and_cfold_equal_their_device_forms(hctx, P, fold_iq, kind, alpha):
    name, mid = _fold_args(kind)
    npx = FOLD["y"] * FOLD["x"]
    state0 = rng(4).random(npx, dtype=np.float32)
    head = (0, f32(1.0), fold_iq.size)
    if alpha == 0.0:   # the staging slot holds another call's picture; the state handed in is NaN, and must not matter
        warm = state0[::-1].copy()
        hctx.call(name, P(fold_iq), *head, *mid, f32(0.25), P(warm))
        host, dev0 = np.full(npx, np.nan, np.float32), np.zeros(npx, np.float32)
    else:
        host, dev0 = state0.copy(), state0
    hctx.call(name, P(fold_iq), *head, *mid, f32(alpha), P(host))
    with Dev(hctx) as d:
        p = d.up(dev0)
        hctx.call(name + "_d", P(d.up(fold_iq)), *head, *mid, f32(alpha), P(p))
        same(host, d.down(p, dev0), "state")
    assert np.isfinite(host).all() and host.any()


@pytest.mark.parametrize("kind", ["fold", "cfold"])
def test_fold_scans_equal_their_device_forms(hctx, P, fold_iq, kind):
    c, nt = FOLD, 9
    head, geom = (0, f32(1.0), fold_iq.size), (nt, c["F"], c["y"], c["x"])
    if kind == "fold":
        name, mid = "tsdr_fold_scan_iq", (f64(c["t0"]), f64(c["T"] - 1.0), f64(0.25)) + geom
    else:
        name, mid = "tsdr_cfold_scan_iq", (f64(c["t0"]), f64(c["T"]), f64(0.0), f64(0.03125)) + geom
    host, best = np.full(nt, -1.0), C.c_int(-2)
    hctx.call(name, P(fold_iq), *head, *mid, P(host), C.byref(best))
    with Dev(hctx) as d:
        p = d.up(np.full(nt, -1.0))
        hctx.call(name + "_d", P(d.up(fold_iq)), *head, *mid, P(p))
        dev = d.down(p, host)
    same(host, dev, "scores")
    assert best.value == int(np.argmax(dev)) and (host != -1.0).all()   # the first maximum, found on the host after the wait


@pytest.mark.parametrize("alpha", [0.0, 0.25])
@pytest.mark.parametrize("have", list(itertools.product([0, 1], repeat=2)), ids=lambda w: "mag%d-info%d" % w)
def test_cstack_equals_its_device_form(hctx, P, fold_iq, have, alpha):
    from tempestsdr_jl_amd import api
    cstack = api._cstack                     # (the module: the package exports a function of that name)
    name, mid = _fold_args("cstack")
    npx = FOLD["y"] * FOLD["x"]
    r = rng(5)
    z0 = (r.standard_normal(npx) + 1j * r.standard_normal(npx)).astype(cf) * cf(1e-3)
    head, mode = (0, f32(1.0), fold_iq.size), cstack.MODES["lock"]

    def outputs():
        return np.full(npx, -1, np.float32) if have[0] else None, np.full(cstack.CSTACK_INFO, -1.0) if have[1] else None

    if alpha == 0.0:
        warm = z0[::-1].copy()
        hctx.call(name, P(fold_iq), *head, *mid, f32(0.25), mode, P(warm), None, None)
        host_z, dev_z0 = np.full(npx, np.nan + 1j * np.nan, cf), np.zeros(npx, cf)
    else:
        host_z, dev_z0 = z0.copy(), z0
    host = outputs()
    hctx.call(name, P(fold_iq), *head, *mid, f32(alpha), mode, P(host_z), P(host[0]), P(host[1]))
    with Dev(hctx) as d:
        like = outputs()
        ptrs = [d.up(a) for a in like]
        pz = d.up(dev_z0)
        hctx.call(name + "_d", P(d.up(fold_iq)), *head, *mid, f32(alpha), mode, P(pz), P(ptrs[0]), P(ptrs[1]))
        same(host_z, d.down(pz, dev_z0), "zstate")
        for h, p, a, what in zip(host, ptrs, like, ("mag", "info")):
            same(h, d.down(p, a) if p is not None else None, what)
    assert np.isfinite(host_z.view(np.float32)).all() and host_z.any()


# ---- vsync -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("y_t, x_t", [(8, 20), (24, 6000), (6000, 24)])   # (sync_cases.SIZES has 6000 lines of 24: both ways round)
def test_vsync_equals_vsync_d_three_calls_in_a_row(tsdr, hctx, P, y_t, x_t, dtype):
    assert (y_t, x_t) in SC.SIZES or (x_t, y_t) in SC.SIZES
    host_sync, dev_sync = tsdr.SyncXY(hctx, y_t, x_t, dtype=dtype), tsdr.SyncXY(hctx, y_t, x_t, dtype=dtype)
    fn_d = "tsdr_vsync_f64_d" if dtype == np.float64 else "tsdr_vsync_d"
    try:
        got, want = [], []
        for family in ("noise", "negative", "zero-band"):   # (the pinned block of small results is reused call after call)
            img = SC.image(family, y_t, x_t, dtype)
            got.append(host_sync.vsync(img))
            with Dev(hctx) as d:
                p = d.up(np.full(2, -1, np.int32))
                rc = getattr(hctx.lib, fn_d)(dev_sync.h, P(d.up(img.ravel(order="F"))), P(p))   # (column-major, as the host form reads it)
                assert rc == 0, hctx.lib.tsdr_last_error(hctx.h)
                want.append(tuple(int(v) for v in hctx.download(p, (2,), np.int32)))
        assert got == want, (got, want)
    finally:
        host_sync.close()
        dev_sync.close()
