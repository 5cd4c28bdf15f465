"""GPU tests of the full-resolution frame average (include/tempest_hip_hires.h): k_raster_accum against the numpy reference
tests/hires_ref.py, bit for bit, at odd word offsets inside guarded arenas (tests/dptr_util.py); every refusal of the contract;
and the whole loop tsdr_frames_hires_iq_d against one tsdr_frames_iq_d call (600x800 outputs) and against the reference
recurrence over the CPU oracle's rasters and sync indices (the full-size state).

References are computed once per geometry and shared (_capture / _oracle); nothing below modifies them."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import dptr_util as D
import hires_ref as R
import oracle_lib as O
from test_hires_host import frames_in_flight

pytestmark = pytest.mark.gpu

U = frames_in_flight()                               # the kernel's frames in flight per lane
NS = [0, 1] + list(range(U - 1, 2 * U + 2))          # n: nothing, one, and every count from U-1 to 2U+1
NMAX = NS[-1]
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 5), (64, 5), (65, 5), (77, 131), (255, 3), (257, 5), (1125, 37)]
ALPHAS = [0.0, 1.0, 0.1, 0.95]
GRID = (600, 800)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
KINDS = [("null", "raster")] + [(k, u) for u in ("raster", "image") for k in ("zero", "last", "neg", "big", "rand", "extreme")]
RTOL = 6e-7                                          # the project's FAST raster bar (tests/test_fast_mode_gpu.py)


def bits(a):
    return np.asfortranarray(a, dtype=np.float32).reshape(-1, order="F").view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def _data(y_t, x_t):
    """NMAX rasters (row f: frame f, column-major) and a start state: sign-changing values of mixed magnitude"""
    rng = np.random.default_rng(1000 * y_t + x_t)
    P = y_t * x_t
    rasters = (rng.standard_normal((NMAX, P)) * np.exp(rng.uniform(-6, 6, (NMAX, P)))).astype(np.float32)
    state = rng.standard_normal(P).astype(np.float32)
    rasters.setflags(write=False)
    state.setflags(write=False)
    return rasters, state


def _mats(flat, n, y_t, x_t):
    return [flat[f].reshape((y_t, x_t), order="F") for f in range(n)]


def _shifts(kind, units, y_t, x_t):
    """NMAX pairs (s_y, s_x), int32, or None"""
    sy, sx = (y_t, x_t) if units == "raster" else GRID
    f = np.arange(NMAX, dtype=np.int64)
    if kind == "null":
        return None
    if kind == "zero":
        s = np.zeros((NMAX, 2), np.int64)
    elif kind == "last":
        s = np.tile([sy - 1, sx - 1], (NMAX, 1))
    elif kind == "neg":
        s = np.stack([-1 - f, -2 - 3 * f], axis=1)
    elif kind == "big":                                   # at and beyond the size
        s = np.stack([sy + f, 2 * sx + 1 - f], axis=1)
    elif kind == "rand":
        rng = np.random.default_rng(7 * y_t + x_t)
        s = np.stack([rng.integers(-3 * sy, 3 * sy + 1, NMAX), rng.integers(-3 * sx, 3 * sx + 1, NMAX)], axis=1)
    else:                                                 # "extreme": the ends of int
        s = np.stack([np.where(f % 2, INT_MIN, INT_MAX), np.where(f % 2, INT_MAX, INT_MIN)], axis=1)
    return np.ascontiguousarray(s, dtype=np.int32)


def _inout(A, name, data, phase):
    """an arena whose payload the call may rewrite: the guards around it are still checked"""
    a = A.input(name, data, phase)
    a.data = None
    return a


def _accum_d(ctx, r, n, y_t, x_t, s, units, alpha, st, grid=GRID):
    ctx.call("tsdr_raster_accum_d", r.ptr if r is not None else None, n, y_t, x_t, s.ptr if s is not None else None,
             R.UNITS[units], grid[0], grid[1], C.c_float(alpha), st.ptr)


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("kind,units", KINDS)
@pytest.mark.parametrize("y_t,x_t", SHAPES)
def test_kernel_equals_reference(ctx, y_t, x_t, kind, units):
    """every n of NS at one shape and one kind of shift, alpha walking through ALPHAS; rasters, shifts and state sit at odd
    word offsets (12, 4, 4 bytes past a 256-byte boundary) inside guarded arenas"""
    flat, state0 = _data(y_t, x_t)
    sh = _shifts(kind, units, y_t, x_t)
    salt = SHAPES.index((y_t, x_t)) + KINDS.index((kind, units))
    with D.Arenas(ctx) as A:
        r = A.input("rasters", flat, 12)
        s = A.input("shifts", sh, 4) if sh is not None else None
        runs = []
        for k, n in enumerate(NS):
            alpha = ALPHAS[(k + salt) % len(ALPHAS)]
            st = _inout(A, f"state n={n}", state0, 4)
            _accum_d(ctx, r, n, y_t, x_t, s, units, alpha, st)
            runs.append((n, alpha, st))
        A.check()     # rasters and shifts unchanged, every guard word intact
        for n, alpha, st in runs:
            want = R.accumulate(_mats(flat, n, y_t, x_t), state0.reshape((y_t, x_t), order="F"), alpha, sh, units, GRID)
            got = st.get(np.float32)
            assert np.array_equal(got.view(np.uint32), bits(want)), (n, alpha)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_kernel_every_alpha_with_every_shift_kind(ctx, alpha):
    y_t, x_t, n = 77, 131, U + 1
    flat, state0 = _data(y_t, x_t)
    with D.Arenas(ctx) as A:
        r = A.input("rasters", flat, 4)
        runs = []
        for kind, units in KINDS:
            sh = _shifts(kind, units, y_t, x_t)
            s = A.input("shifts", sh, 12) if sh is not None else None
            st = _inout(A, f"state {kind} {units}", state0, 12)
            _accum_d(ctx, r, n, y_t, x_t, s, units, alpha, st)
            runs.append((kind, units, sh, st))
        A.check()
        for kind, units, sh, st in runs:
            want = R.accumulate(_mats(flat, n, y_t, x_t), state0.reshape((y_t, x_t), order="F"), alpha, sh, units, GRID)
            assert np.array_equal(st.get(np.float32).view(np.uint32), bits(want)), (kind, units)


def test_shift_moves_the_picture_as_circshift_does(ctx):
    """alpha = 0, one frame: the state IS the shifted raster -- against np.roll directly, in both units"""
    y_t, x_t = 77, 131
    flat, state0 = _data(y_t, x_t)
    m = flat[0].reshape((y_t, x_t), order="F")
    with D.Arenas(ctx) as A:
        r = A.input("rasters", flat[:1], 4)
        for units, (a, b), (ry, rx) in (("raster", (5, -3), (5, x_t - 3)), ("image", (300, 200), ((2 * 300 * y_t + 600) // 1200, (2 * 200 * x_t + 800) // 1600))):
            s = A.input("shifts", np.array([a, b], np.int32), 4)
            st = _inout(A, "state", state0, 4)
            _accum_d(ctx, r, 1, y_t, x_t, s, units, 0.0, st)
            A.check()
            # (alpha = 0: 0 * state + 1 * v; the zero product keeps v's bits unless the state is non-finite)
            assert same_bits(st.get(np.float32, (y_t, x_t), "F"), np.float32(0.0) * state0.reshape((y_t, x_t), order="F") + np.roll(m, (-ry, -rx), axis=(0, 1)))


def test_nan_and_inf_propagate(ctx):
    y_t, x_t, n = 65, 5, U + 2
    flat, state0 = (a.copy() for a in _data(y_t, x_t))
    flat[0, 3] = np.nan
    flat[n - 1, 100] = np.inf
    flat[2, 200] = -np.inf
    flat[3, 200] = np.inf           # Inf - Inf further down the chain
    state0[7] = np.nan
    state0[8] = np.inf
    sh = _shifts("rand", "raster", y_t, x_t)
    for alpha in (0.1, 0.0, 1.0):
        with D.Arenas(ctx) as A:
            r, s = A.input("rasters", flat, 4), A.input("shifts", sh, 4)
            st = _inout(A, "state", state0, 12)
            _accum_d(ctx, r, n, y_t, x_t, s, "raster", alpha, st)
            A.check()
            got = st.get(np.float32)
        want = R.accumulate(_mats(flat, n, y_t, x_t), state0.reshape((y_t, x_t), order="F"), alpha, sh, "raster").reshape(-1, order="F")
        nan = np.isnan(want)
        assert nan.any() and np.array_equal(np.isnan(got), nan), alpha          # NaN positions only (payload bits are not promised)
        assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), alpha   # everything else exact, Inf included
        assert np.isinf(want).any()


@pytest.mark.parametrize("y_t,x_t", [(1, 1), (65, 5), (77, 131), (1125, 37)])
def test_host_form_equals_device_form(ctx, y_t, x_t):
    flat, state0 = _data(y_t, x_t)
    s0 = state0.reshape((y_t, x_t), order="F")
    for n, alpha, (kind, units) in ((0, 0.1, ("rand", "raster")), (1, 0.95, ("null", "raster")), (U + 3, 0.1, ("rand", "image")),
                                    (NMAX, 0.95, ("neg", "raster"))):
        sh = _shifts(kind, units, y_t, x_t)
        mats = _mats(flat, n, y_t, x_t)
        host = np.asfortranarray(s0.copy())
        back = ctx.raster_accumulate(mats, host, alpha, None if sh is None else sh[:n], units, GRID)
        assert back is host
        with D.Arenas(ctx) as A:
            r = A.input("rasters", flat, 4)
            s = A.input("shifts", sh, 4) if sh is not None else None
            st = _inout(A, "state", state0, 4)
            ctx.raster_accumulate_d(r.addr, n, y_t, x_t, alpha, st.addr, None if s is None else s.addr, units, GRID)
            A.check()
            dev = st.get(np.float32, (y_t, x_t), "F")
        assert same_bits(host, dev) and same_bits(host, R.accumulate(mats, s0, alpha, None if sh is None else sh[:n], units, GRID)), (n, kind)


def test_every_refusal_writes_nothing(ctx):
    y_t, x_t, n = 65, 5, 3
    flat, state0 = _data(y_t, x_t)
    sh = _shifts("rand", "raster", y_t, x_t)
    call = ctx.lib.tsdr_raster_accum_d
    EINVAL = -1
    with D.Arenas(ctx) as A:
        r, s = A.input("rasters", flat, 4), A.input("shifts", sh, 4)
        st = A.input("state", state0, 4)       # an INPUT arena: the payload must come back untouched as well
        ok = dict(rasters=r.addr, n=n, y_t=y_t, x_t=x_t, shifts=s.addr, units=0, img_h=600, img_w=800, state=st.addr)
        bad = [dict(y_t=0), dict(y_t=-5), dict(x_t=0), dict(x_t=-1), dict(n=-1), dict(y_t=1 << 16, x_t=1 << 15), dict(y_t=46341, x_t=46341),
               dict(state=None), dict(rasters=None), dict(units=2), dict(units=-1), dict(units=1, img_h=0), dict(units=1, img_w=0),
               dict(units=1, img_h=-600), dict(state=st.addr + 2), dict(state=st.addr + 1), dict(rasters=r.addr + 2), dict(shifts=s.addr + 2)]
        for change in bad:
            a = dict(ok, **change)
            rc = call(ctx.h, a["rasters"], a["n"], a["y_t"], a["x_t"], a["shifts"], a["units"], a["img_h"], a["img_w"], C.c_float(0.5), a["state"])
            assert rc == EINVAL, (change, rc)
            assert ctx.lib.tsdr_last_error(ctx.h), change
        # the host form refuses the same before it stages anything
        host = np.asfortranarray(state0.reshape((y_t, x_t), order="F").copy())
        keep = host.copy()
        for units, grid in ((2, GRID), (1, (0, 800)), (1, (600, -1))):
            with pytest.raises(AssertionError):
                ctx.raster_accumulate(_mats(flat, n, y_t, x_t), host, 0.5, sh[:n], units, grid)
        rc = ctx.lib.tsdr_raster_accum(ctx.h, flat.ctypes.data, n, y_t, x_t, None, 0, 600, 800, C.c_float(0.5), None)
        assert rc == EINVAL and np.array_equal(host, keep)
        # NULL rasters are fine when there is nothing to read; img_h / img_w are ignored in raster units
        assert call(ctx.h, None, 0, y_t, x_t, None, 0, 0, 0, C.c_float(0.5), st.addr) == 0
        A.check()                             # state, rasters, shifts and all guard words as uploaded
        # ... and the context still works
        st2 = _inout(A, "state after", state0, 4)
        _accum_d(ctx, r, n, y_t, x_t, s, "raster", 0.5, st2)
        A.check()
        want = R.accumulate(_mats(flat, n, y_t, x_t), state0.reshape((y_t, x_t), order="F"), 0.5, sh, "raster")
        assert np.array_equal(st2.get(np.float32).view(np.uint32), bits(want))


# ---------------------------------------------------------------- the whole loop
GEOMS = {"125x160": dict(Fs=1.0e6, x_t=160, y_t=125, fv=50.0, nfr=5, extra=778),     # S = 20000: the raster is smaller than the sync grid
         "628x1056": dict(Fs=2.0e6, x_t=1056, y_t=628, fv=60.0, nfr=3, extra=777)}   # S = 33333: larger than the grid
ALPHA, ALPHA_H = np.float32(0.1), np.float32(0.1)


def _api():
    from tempest_loader import load_package
    load_package()
    return importlib.import_module("tempestsdr_jl_amd.api")


def _quantise(iq, fmt):
    """the capture as an SDR would have stored it -> (integer components, scale)"""
    v = np.ascontiguousarray(iq).view(np.float32)
    m = float(np.abs(v).max())
    if fmt == "sc16":
        return np.round(v / (m / 30000)).astype(np.int16), m / 30000
    return np.clip(np.round(v / (m / 120) + 127.5), 0, 255).astype(np.uint8), m / 120


@functools.lru_cache(maxsize=None)
def _capture(name, fmt="cf32"):
    """-> (what goes to the device, scale, the ComplexF32 samples it stands for, S)"""
    _api()
    synth = importlib.import_module("tempestsdr_jl_amd.synth")
    g = GEOMS[name]
    S = synth.samples_per_frame(g["Fs"], g["fv"])
    iq = synth.synth_leak(g["Fs"], g["x_t"], g["y_t"], g["fv"], S * g["nfr"] + g["extra"])   # (the ragged tail is dropped, GUI.jl:137)
    if fmt == "cf32":
        return iq, 1.0, iq, S
    q, scale = _quantise(iq, fmt)
    return q, scale, _api().expand_iq(q, fmt, scale), S


def _first_col(beta, dark):
    """findmax(beta)[2][2] (findmin under "vsync_blank_dark"): 1-based column of the first extremum in column-major order"""
    b = np.asarray(beta).ravel(order="F")
    return int(np.argmin(b) if dark else np.argmax(b)) // np.shape(beta)[0] + 1


@functools.lru_cache(maxsize=None)
def _oracle(name, fmt="cf32"):
    """The CPU oracle's view of a capture (orc_frames): its rasters, its aligned run (600x800 frames, state, sync indices), and
    the sync indices of the two vsync options, which the oracle's loop does not have: picked from the oracle's OWN beta matrices
    of its unaligned 600x800 images (first extremum, s_y lagging one frame unless "vsync_current_sy")."""
    g = GEOMS[name]
    _, _, z, S = _capture(name, fmt)
    st = np.zeros(GRID, np.float32, order="F")
    o = O.frames(O.SyncXY(*GRID), z, S, g["y_t"], g["x_t"], ALPHA, st, want_raster=True)
    raw = O.frames(None, z, S, g["y_t"], g["x_t"], np.float32(0.0), np.zeros(GRID, np.float32, order="F"), do_align=False)
    assert o["n_frames"] == g["nfr"]
    assert all(float(r.min()) > 0.0 for r in o["raster"]), "the FAST tolerance is relative: the rasters must be strictly positive"
    idx = {}
    for dark in (0, 1):
        sync, picks = O.SyncXY(*GRID), []
        for im in raw["frames"]:
            sync.vsync(np.asfortranarray(im))
            picks.append((_first_col(sync.beta("y"), dark), _first_col(sync.beta("x"), dark)))
        for cur in (0, 1):
            prev, rows = 1, []
            for cy, cx in picks:
                rows.append((cy if cur else prev, cx))
                prev = cy
            idx[(dark, cur)] = np.array(rows, np.int32)
    assert np.array_equal(idx[(0, 0)], o["sync_idx"]), "the picks reproduce the oracle's own loop in the default mode"
    return dict(raster=o["raster"], frames=o["frames"], state=st, sync_idx=o["sync_idx"], idx=idx)


def _run(ctx, tsdr, name, fmt="cf32", *, hires, do_align=True, chunk=None, split=None, state=None, hires_state=None, sync=None):
    """one pass over the capture on device buffers -> dict(n, state, frames, idx[, hires]).  hires=False: ONE tsdr_frames_iq_d call.
    split: frames in the first of two consecutive calls (both states and the SyncXY carry over)."""
    api = _api()
    g = GEOMS[name]
    dev, scale, _, S = _capture(name, fmt)
    y_t, x_t, nfr = g["y_t"], g["x_t"], g["nfr"]
    per = 1 if fmt == "cf32" else 2                       # array elements per sample
    bounds = [(0, nfr)] if split is None else [(0, split), (split, nfr)]
    sync = tsdr.SyncXY(ctx, *GRID) if (sync is None and do_align) else sync
    if chunk is not None:
        ctx.set_option("hires_chunk_frames", chunk)
    try:
        with D.Arenas(ctx) as A:
            d_iq = A.input("iq", dev, 0)
            st = _inout(A, "imageOut", np.zeros(GRID[0] * GRID[1], np.float32) if state is None else state, 0)
            hs = _inout(A, "hires_state", np.zeros(y_t * x_t, np.float32) if hires_state is None else hires_state, 4)
            fr = A.output("frames_out", nfr * GRID[0] * GRID[1] * 4, 0)
            ix = A.output("sync_idx", nfr * 8, 4)
            total = 0
            for f0, f1 in bounds:
                nE = (f1 - f0) * S + (g["extra"] if f1 == nfr else 0)
                a_iq = d_iq.addr + f0 * S * per * dev.itemsize
                a_fr, a_ix = fr.addr + f0 * GRID[0] * GRID[1] * 4, ix.addr + f0 * 8
                if hires:
                    n = C.c_int(0)
                    ctx.call("tsdr_frames_hires_iq_d", C.c_void_p(sync.h if sync is not None else 0), C.c_void_p(a_iq), api.iq_fmt_code(fmt),
                             C.c_float(scale), nE, S, y_t, x_t, C.c_float(ALPHA), int(do_align), st.ptr, C.c_void_p(a_fr), C.c_float(ALPHA_H),
                             hs.ptr, C.c_void_p(a_ix), C.byref(n))
                    total += n.value
                else:
                    total += api.frames_iq_d(ctx, sync, a_iq, fmt, scale, nE, S, y_t, x_t, ALPHA, do_align, st.addr, a_fr, None, a_ix)
            A.check()
            out = dict(n=total, state=st.get(np.float32), frames=fr.get(np.float32), idx=ix.get(np.int32).reshape(nfr, 2), sync=sync)
            if hires:
                out["hires"] = hs.get(np.float32, (y_t, x_t), "F")
            return out
    finally:
        if chunk is not None:
            ctx.set_option("hires_chunk_frames", 0)


class _exact:
    def __init__(self, ctx, **options):
        self.ctx, self.options = ctx, options

    def __enter__(self):
        self.ctx.set_precision("exact")
        for k, v in self.options.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.options:
            self.ctx.set_option(k, 0)
        self.ctx.set_precision("fast")


def _check_exact(name, got, one, want_hires, do_align=True):
    g = GEOMS[name]
    assert got["n"] == one["n"] == g["nfr"]
    assert np.array_equal(got["state"].view(np.uint32), one["state"].view(np.uint32)), "imageOut"
    assert np.array_equal(got["frames"].view(np.uint32), one["frames"].view(np.uint32)), "frames_out"
    if do_align:
        assert np.array_equal(got["idx"], one["idx"]), (got["idx"].tolist(), one["idx"].tolist())
    else:
        assert np.array_equal(got["idx"].view(np.uint32), one["idx"].view(np.uint32)), "sync_idx is not written without do_align"
    assert same_bits(got["hires"], want_hires), "hires_state"


def _want_hires(name, fmt="cf32", idx=None, do_align=True, state=None):
    o = _oracle(name, fmt)
    g = GEOMS[name]
    s0 = np.zeros((g["y_t"], g["x_t"]), np.float32, order="F") if state is None else state
    return R.accumulate(o["raster"], s0, ALPHA_H, (o["sync_idx"] if idx is None else idx) if do_align else None, "image", GRID)


@pytest.mark.parametrize("chunk", [0, 1, 2])
@pytest.mark.parametrize("name", list(GEOMS))
def test_loop_exact_in_chunks(ctx, tsdr, name, chunk):
    """chunks of all, 1 and 2 frames (2 divides neither 5 nor 3): the 600x800 outputs are those of one tsdr_frames_iq_d call and
    of the oracle; the full-size state is the reference recurrence over the oracle's rasters and indices"""
    o = _oracle(name)
    with _exact(ctx):
        one = _run(ctx, tsdr, name, hires=False)
        got = _run(ctx, tsdr, name, hires=True, chunk=chunk)
    _check_exact(name, got, one, _want_hires(name))
    assert np.array_equal(got["idx"], o["sync_idx"]) and np.array_equal(got["state"].view(np.uint32), bits(o["state"]))
    # the registration is doing something on this input: the unaligned average differs
    assert not same_bits(got["hires"], _want_hires(name, do_align=False))


@pytest.mark.parametrize("name", list(GEOMS))
def test_loop_exact_without_alignment(ctx, tsdr, name):
    with _exact(ctx):
        one = _run(ctx, tsdr, name, hires=False, do_align=False)
        got = _run(ctx, tsdr, name, hires=True, do_align=False, chunk=2)
    _check_exact(name, got, one, _want_hires(name, do_align=False), do_align=False)


@pytest.mark.parametrize("option,key", [("vsync_blank_dark", (1, 0)), ("vsync_current_sy", (0, 1))])
@pytest.mark.parametrize("name", list(GEOMS))
def test_loop_exact_under_the_vsync_options(ctx, tsdr, name, option, key):
    """the full-size picture follows the loop's own sync_idx, whatever polarity and s_y ordering produced it"""
    idx = _oracle(name)["idx"][key]
    assert not np.array_equal(idx, _oracle(name)["sync_idx"]), "the option changes the indices on this input"
    with _exact(ctx, **{option: 1}):
        one = _run(ctx, tsdr, name, hires=False)
        got = _run(ctx, tsdr, name, hires=True, chunk=2)
    _check_exact(name, got, one, _want_hires(name, idx=idx))
    assert np.array_equal(got["idx"], idx)


@pytest.mark.parametrize("fmt", ["sc16", "uc8"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_loop_exact_on_integer_iq(ctx, tsdr, name, fmt):
    """the raw integer buffer gives what its expanded samples give: against one tsdr_frames_iq_d call on the raw buffer, the
    hires loop on the EXPANDED ComplexF32 samples, and the oracle on the expanded samples"""
    _, _, z, S = _capture(name, fmt)
    g = GEOMS[name]
    with _exact(ctx):
        one = _run(ctx, tsdr, name, fmt, hires=False)
        got = _run(ctx, tsdr, name, fmt, hires=True, chunk=2)
        hs = np.zeros((g["y_t"], g["x_t"]), np.float32, order="F")
        st = np.zeros(GRID, np.float32, order="F")
        exp = ctx.frames_hires(tsdr.SyncXY(ctx, *GRID), z, S, g["y_t"], g["x_t"], ALPHA, st, ALPHA_H, hs)
    _check_exact(name, got, one, _want_hires(name, fmt))
    assert exp["n_frames"] == g["nfr"] and np.array_equal(exp["sync_idx"], got["idx"])
    assert same_bits(hs, got["hires"]) and np.array_equal(bits(st), got["state"].view(np.uint32))
    assert all(np.array_equal(bits(exp["frames"][f]), got["frames"].reshape(g["nfr"], -1)[f].view(np.uint32)) for f in range(g["nfr"]))


@pytest.mark.parametrize("name", list(GEOMS))
def test_loop_exact_over_two_buffers(ctx, tsdr, name):
    """two consecutive calls on one SyncXY carry imageOut, the pending s_y and the full-size state: the same as one call over
    all frames, from non-trivial start states"""
    g = GEOMS[name]
    rng = np.random.default_rng(11)
    st0 = rng.random(GRID[0] * GRID[1], dtype=np.float32)
    hs0 = rng.random(g["y_t"] * g["x_t"], dtype=np.float32)
    with _exact(ctx):
        one = _run(ctx, tsdr, name, hires=False, state=st0)
        got = _run(ctx, tsdr, name, hires=True, split=g["nfr"] // 2 + 1, state=st0, hires_state=hs0)
    _check_exact(name, got, one, _want_hires(name, state=hs0.reshape((g["y_t"], g["x_t"]), order="F")))


def test_host_array_form_and_null_sync_idx(ctx, tsdr):
    """Context.frames_hires (host arrays) and a NULL sync_idx (indices go to workspace) give the same full-size state"""
    name = "125x160"
    g = GEOMS[name]
    iq, _, _, S = _capture(name)
    with _exact(ctx):
        hs = np.zeros((g["y_t"], g["x_t"]), np.float32, order="F")
        st = np.zeros(GRID, np.float32, order="F")
        r = ctx.frames_hires(tsdr.SyncXY(ctx, *GRID), iq, S, g["y_t"], g["x_t"], ALPHA, st, ALPHA_H, hs)
        with D.Arenas(ctx) as A:
            d_iq = A.input("iq", iq, 0)
            d_st = _inout(A, "imageOut", np.zeros(GRID[0] * GRID[1], np.float32), 0)
            d_hs = _inout(A, "hires_state", np.zeros(g["y_t"] * g["x_t"], np.float32), 12)
            n = ctx.frames_hires_d(tsdr.SyncXY(ctx, *GRID), d_iq.addr, "cf32", 1.0, iq.size, S, g["y_t"], g["x_t"], ALPHA, True, d_st.addr,
                                   ALPHA_H, d_hs.addr, None, None)
            A.check()
            dev = d_hs.get(np.float32, (g["y_t"], g["x_t"]), "F")
    assert n == r["n_frames"] == g["nfr"] and np.array_equal(r["sync_idx"], _oracle(name)["sync_idx"])
    assert same_bits(hs, _want_hires(name)) and same_bits(dev, hs) and same_bits(st, _oracle(name)["state"])
    # fewer samples than one frame: nothing happens
    out = ctx.frames_hires(tsdr.SyncXY(ctx, *GRID), iq[:100], S, g["y_t"], g["x_t"], ALPHA, st, ALPHA_H, hs)
    assert out["n_frames"] == 0 and same_bits(hs, _want_hires(name))
    # what the second stage refuses is refused before anything runs
    with pytest.raises(AssertionError):
        ctx.frames_hires_d(None, 256, "cf32", 1.0, 10, 5, 125, 160, ALPHA, False, 256, ALPHA_H, None)


@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("name", list(GEOMS))
def test_loop_fast(ctx, tsdr, name, chunk):
    """TSDR_FAST, alpha = 0.1: indices identical to the oracle's; every pixel of the full-size state within
    RTOL + 4 * 2^-24 / (1 - alpha) relative of the reference.  RTOL is the FAST raster bar; a combination with non-negative
    weights of non-negative pixels, each within RTOL, stays within RTOL; the second term bounds the two chains' own roundings.
    No pixel is excluded: the oracle's rasters are strictly positive on these inputs (asserted in _oracle)."""
    assert ctx.precision == "fast"
    o = _oracle(name)
    got = _run(ctx, tsdr, name, hires=True, chunk=chunk)
    assert got["n"] == GEOMS[name]["nfr"] and np.array_equal(got["idx"], o["sync_idx"])
    want = np.asarray(_want_hires(name), np.float64)
    assert want.min() > 0.0
    rel = float(np.max(np.abs(np.asarray(got["hires"], np.float64) - want) / want))
    bound = RTOL + 4 * 2.0 ** -24 / (1.0 - float(ALPHA_H))
    print(f"{name} chunk {chunk}: max relative error {rel:.3e} (bound {bound:.3e})")
    assert bound < 9e-7 and rel <= bound
