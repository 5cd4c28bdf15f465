"""GPU tests of the registration to the raster pixel (include/tempest_hip_register.h): the profiles against numpy (bit for bit on
integers, within the derived bound of any f64 summation order on random data), the registration against tests/register_ref.py
(shifts and scores bit for bit on integer pictures), every refusal, and the frame loop under "hires_refine" against the reference
evaluated chunk by chunk on the CPU oracle's rasters.  Every device pointer sits at an offset inside a guarded arena
(tests/dptr_util.py).

References are computed once per case and shared (functools caches here and in test_register_host.py); nothing modifies them."""
import ctypes as C
import functools

import numpy as np
import pytest

import dptr_util as D
import hires_ref as H
import register_ref as R
import test_register_host as RH
from test_hires_gpu import RTOL, _exact, _inout, same_bits

pytestmark = pytest.mark.gpu

# the shapes of tests/test_hires_gpu.py, and one whose 16-byte path has two row blocks and two column strips
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 5), (64, 5), (65, 5), (77, 131), (255, 3), (257, 5), (1125, 37), (1028, 70)]
NS = [0, 1, 2, 5]
NMAX = max(NS)
GRID = RH.GRID
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
EINVAL = -1


@functools.lru_cache(maxsize=None)
def _ints(y_t, x_t):
    """NMAX + 1 integer-valued pictures in 0 .. 255 (row f: frame f, column-major; the last one serves as ref)"""
    rng = np.random.default_rng(31 * y_t + x_t)
    a = rng.integers(0, 256, (NMAX + 1, y_t * x_t)).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _floats(y_t, x_t):
    rng = np.random.default_rng(77 * y_t + x_t)
    P = y_t * x_t
    a = (rng.standard_normal((NMAX, P)) * np.exp(rng.uniform(-6, 6, (NMAX, P)))).astype(np.float32)
    a.setflags(write=False)
    return a


def _mats(flat, n, y_t, x_t):
    return [flat[f].reshape((y_t, x_t), order="F") for f in range(n)]


def _profiles_d(ctx, r, n, y_t, x_t, col, row):
    ctx.call("tsdr_raster_profiles_d", r.ptr if r is not None else None, n, y_t, x_t, col.ptr if col is not None else None,
             row.ptr if row is not None else None)


# ---------------------------------------------------------------- profiles
@pytest.mark.parametrize("phase", [0, 4])
@pytest.mark.parametrize("y_t,x_t", SHAPES)
def test_profiles_of_integers_are_exact(ctx, y_t, x_t, phase):
    """phase 0: every column starts on a 16-byte boundary when y_t is a multiple of 4 (the 16-byte loads); phase 4: it never does
    (dword loads).  Sums of integers up to 1125 * 255 are exact in f64 in any order: bit-identical to numpy."""
    flat = _ints(y_t, x_t)
    with D.Arenas(ctx) as A:
        r = A.input("rasters", flat[:NMAX], phase)
        runs = []
        for n in NS:
            col, row = A.output(f"col n={n}", max(n, 1) * x_t * 8, 8), A.output(f"row n={n}", max(n, 1) * y_t * 8, 24)
            again = A.output(f"col again n={n}", max(n, 1) * x_t * 8, 0), A.output(f"row again n={n}", max(n, 1) * y_t * 8, 16)
            _profiles_d(ctx, r, n, y_t, x_t, col, row)
            _profiles_d(ctx, r, n, y_t, x_t, *again)
            runs.append((n, col, row, again))
        A.check()
        for n, col, row, again in runs:
            if n == 0:      # touches nothing: the payloads still hold their sentinels
                for a in (col, row):
                    assert np.array_equal(a.get(np.uint32), D.sentinel_words(a.size // 4)[a.lead // 4: (a.lead + a.payload) // 4])
                continue
            m = np.stack(_mats(flat, n, y_t, x_t)).astype(np.float64)
            want_col, want_row = m.sum(axis=1), m.sum(axis=2)
            assert np.array_equal(col.get(np.float64).view(np.uint64), want_col.reshape(-1).view(np.uint64)), n
            assert np.array_equal(row.get(np.float64).view(np.uint64), want_row.reshape(-1).view(np.uint64)), n
            assert np.array_equal(again[0].get(np.uint64), col.get(np.uint64)) and np.array_equal(again[1].get(np.uint64), row.get(np.uint64))


@pytest.mark.parametrize("y_t,x_t", SHAPES)
def test_profiles_of_floats_within_the_bound_of_any_order(ctx, y_t, x_t):
    """|got - fsum| <= n_terms * 2^-53 * sum|x| per element: the worst case of ANY f64 summation order of exactly converted f32
    values (each of the n_terms - 1 additions rounds by at most 2^-53 of a partial sum that never exceeds sum|x|), not a measured
    tolerance.  A second call returns the same bits; a NULL col or row leaves the other correct."""
    flat = _floats(y_t, x_t)
    n = NMAX
    phase = 0 if (y_t + x_t) % 2 else 12
    with D.Arenas(ctx) as A:
        r = A.input("rasters", flat, phase)
        outs = [(A.output("col", n * x_t * 8, 8), A.output("row", n * y_t * 8, 8)), (A.output("col 2", n * x_t * 8, 16), A.output("row 2", n * y_t * 8, 0)),
                (A.output("col only", n * x_t * 8, 24), None), (None, A.output("row only", n * y_t * 8, 8))]
        for col, row in outs:
            _profiles_d(ctx, r, n, y_t, x_t, col, row)
        A.check()
        col, row = outs[0][0].get(np.float64).reshape(n, x_t), outs[0][1].get(np.float64).reshape(n, y_t)
        for f, m in enumerate(_mats(flat, n, y_t, x_t)):
            wc, wr, ac, ar = R.profiles_fsum(m)
            assert np.all(np.abs(col[f] - wc) <= y_t * 2.0 ** -53 * ac), (f, float(np.max(np.abs(col[f] - wc) / np.maximum(ac, 1e-300))))
            assert np.all(np.abs(row[f] - wr) <= x_t * 2.0 ** -53 * ar), (f, float(np.max(np.abs(row[f] - wr) / np.maximum(ar, 1e-300))))
        for c2, r2 in outs[1:]:
            assert c2 is None or np.array_equal(c2.get(np.uint64), outs[0][0].get(np.uint64))
            assert r2 is None or np.array_equal(r2.get(np.uint64), outs[0][1].get(np.uint64))


# ---------------------------------------------------------------- register
def _shifts(kind, units, y_t, x_t, n):
    sy, sx = (y_t, x_t) if units == "raster" else GRID
    f = np.arange(n, dtype=np.int64)
    if kind == "null":
        return None
    if kind == "neg":
        s = np.stack([-1 - f, -2 - 3 * f], axis=1)
    elif kind == "big":
        s = np.stack([sy + f, 2 * sx + 1 - f], axis=1)
    elif kind == "rand":
        rng = np.random.default_rng(7 * y_t + x_t)
        s = np.stack([rng.integers(-3 * sy, 3 * sy + 1, n), rng.integers(-3 * sx, 3 * sx + 1, n)], axis=1)
    else:                                                 # "extreme": the ends of int
        s = np.stack([np.where(f % 2, INT_MIN, INT_MAX), np.where(f % 2, INT_MAX, INT_MIN)], axis=1)
    return np.ascontiguousarray(s, dtype=np.int32)


def _pairs(sh):
    return None if sh is None else [tuple(int(v) for v in row) for row in sh]


def _register_d(ctx, r, n, y_t, x_t, ref, s, units, d_y, d_x, out, sc, grid=GRID):
    ctx.call("tsdr_raster_register_d", r.ptr if r is not None else None, n, y_t, x_t, ref.ptr if ref is not None else None,
             s.ptr if s is not None else None, H.UNITS[units], grid[0], grid[1], d_y, d_x, out.ptr if out is not None else None,
             sc.ptr if sc is not None else None)


def _check_register(got_shifts, got_scores, want, what):
    assert np.array_equal(got_shifts, want[0]), (what, got_shifts.tolist(), want[0].tolist())
    assert np.array_equal(got_scores.view(np.uint64), want[1].view(np.uint64)), what


@pytest.mark.parametrize("y_t,x_t", SHAPES)
def test_register_equals_reference(ctx, y_t, x_t):
    """integer rasters and ref: every product and sum stays far below 2^53, so shifts and scores are bit-identical to the
    reference in any order.  One shape per case; inside, every kind of coarse shift in both units at D = 1, and D in {0, 1,
    (size - 1) / 2} with a picture, no picture and a flat picture as ref."""
    n = 3
    flat = _ints(y_t, x_t)
    mats, refm = _mats(flat, n, y_t, x_t), flat[NMAX].reshape((y_t, x_t), order="F")
    flatref = np.full(y_t * x_t, 7.0, np.float32)
    Dm = ((y_t - 1) // 2, (x_t - 1) // 2)
    D1 = (min(1, Dm[0]), min(1, Dm[1]))
    combos = [(kind, units, D1, "pic") for units in ("raster", "image") for kind in ("neg", "big", "rand", "extreme")]
    combos += [("null", "raster", D1, "pic"), ("rand", "image", (0, 0), "pic"), ("rand", "raster", Dm, "pic"), ("rand", "image", D1, "none"),
               ("null", "raster", Dm, "none"), ("rand", "raster", D1, "flat"), ("rand", "image", Dm, "flat")]
    phase = 0 if x_t % 2 else 4
    with D.Arenas(ctx) as A:
        r = A.input("rasters", flat[:n], phase)
        refs = {"pic": (A.input("ref", refm.reshape(-1, order="F"), phase), refm), "none": (None, None),
                "flat": (A.input("flat ref", flatref, phase), flatref.reshape((y_t, x_t), order="F"))}
        runs = []
        for kind, units, (d_y, d_x), which in combos:
            sh = _shifts(kind, units, y_t, x_t, n)
            s = A.input("shifts", sh, 4) if sh is not None else None
            out = A.output("shifts_out", n * 8, 4)
            sc = A.output("scores", n * (2 * d_y + 1 + 2 * d_x + 1) * 8, 8)
            _register_d(ctx, r, n, y_t, x_t, refs[which][0], s, units, d_y, d_x, out, sc)
            runs.append((kind, units, d_y, d_x, which, sh, out, sc))
        A.check()
        for kind, units, d_y, d_x, which, sh, out, sc in runs:
            want = R.register(mats, refs[which][1], d_y, d_x, _pairs(sh), units, GRID)
            _check_register(out.get(np.int32).reshape(n, 2), sc.get(np.float64).reshape(n, -1), want, (kind, units, d_y, d_x, which))


def test_register_without_scores_and_with_many_frames(ctx):
    """scores == NULL; and more frames than one workgroup's worth of anything (n = 70 of a small shape)"""
    y_t, x_t, n = 12, 20, 70
    rng = np.random.default_rng(9)
    flat = rng.integers(0, 41, (n, y_t * x_t)).astype(np.float32)
    ref = rng.integers(0, 41, y_t * x_t).astype(np.float32)
    sh = np.stack([rng.integers(-50, 50, n), rng.integers(-50, 50, n)], axis=1).astype(np.int32)
    with D.Arenas(ctx) as A:
        r, rf, s = A.input("rasters", flat, 0), A.input("ref", ref, 0), A.input("shifts", sh, 12)
        out = A.output("shifts_out", n * 8, 12)
        _register_d(ctx, r, n, y_t, x_t, rf, s, "raster", 2, 4, out, None)
        A.check()
        want = R.register(_mats(flat, n, y_t, x_t), ref.reshape((y_t, x_t), order="F"), 2, 4, _pairs(sh))
        assert np.array_equal(out.get(np.int32).reshape(n, 2), want[0])


def test_nan_frame_gets_d_zero_and_the_others_are_untouched(ctx):
    y_t, x_t, n = 65, 5, 3
    flat = _ints(y_t, x_t)[:n].copy()
    refm = _ints(y_t, x_t)[NMAX].reshape((y_t, x_t), order="F")
    sh = _shifts("rand", "raster", y_t, x_t, n)
    clean = R.register(_mats(flat, n, y_t, x_t), refm, 3, 2, _pairs(sh))
    flat[1, 100] = np.nan
    with D.Arenas(ctx) as A:
        r, rf, s = A.input("rasters", flat, 4), A.input("ref", refm.reshape(-1, order="F"), 4), A.input("shifts", sh, 4)
        out, sc = A.output("shifts_out", n * 8, 4), A.output("scores", n * 12 * 8, 8)
        _register_d(ctx, r, n, y_t, x_t, rf, s, "raster", 3, 2, out, sc)
        A.check()
        got, scores = out.get(np.int32).reshape(n, 2), sc.get(np.float64).reshape(n, -1)
    assert np.array_equal(got[1], [sh[1][0] % y_t, sh[1][1] % x_t]) and np.all(np.isnan(scores[1])), "d = 0 on both axes"
    for f in (0, 2):
        assert np.array_equal(got[f], clean[0][f]) and np.array_equal(scores[f].view(np.uint64), clean[1][f].view(np.uint64)), f


def test_constructed_tie_gives_minus_one(ctx):
    rasters, ref = RH.tie_case()
    y_t, x_t = ref.shape
    with D.Arenas(ctx) as A:
        r, rf = A.input("rasters", rasters[0].reshape(-1, order="F"), 0), A.input("ref", ref.reshape(-1, order="F"), 0)
        out, sc = A.output("shifts_out", 8, 4), A.output("scores", 6 * 8, 8)
        _register_d(ctx, r, 1, y_t, x_t, rf, None, "raster", 1, 1, out, sc)
        A.check()
        got, scores = out.get(np.int32), sc.get(np.float64)
    assert scores[3] == scores[5] > scores[4] and got[1] == x_t - 1, (got.tolist(), scores.tolist())
    _check_register(got.reshape(1, 2), scores.reshape(1, -1), R.register(rasters, ref, 1, 1), "tie")


@pytest.mark.parametrize("sigma", RH.DISP["sigmas"])
def test_known_displacement_gives_t(ctx, sigma):
    rasters, ref, idx, ts, (d_y, d_x) = RH.displacement_case(sigma)
    y_t, x_t, grid, n = RH.DISP["y_t"], RH.DISP["x_t"], RH.DISP["grid"], len(rasters)
    flat = np.stack([m.reshape(-1, order="F") for m in rasters])
    with D.Arenas(ctx) as A:
        r, rf, s = A.input("rasters", flat, 0), A.input("ref", ref.reshape(-1, order="F"), 0), A.input("shifts", idx, 4)
        out, sc = A.output("shifts_out", n * 8, 4), A.output("scores", n * (2 * d_y + 1 + 2 * d_x + 1) * 8, 8)
        _register_d(ctx, r, n, y_t, x_t, rf, s, "image", d_y, d_x, out, sc, grid)
        A.check()
        got, scores = out.get(np.int32).reshape(n, 2), sc.get(np.float64).reshape(n, -1)
    assert np.array_equal(got, ts % [y_t, x_t]), (got.tolist(), ts.tolist())
    _check_register(got, scores, R.register(rasters, ref, d_y, d_x, _pairs(idx), "image", grid), sigma)


@pytest.mark.parametrize("y_t,x_t", [(1, 1), (65, 5), (77, 131), (1028, 70)])
def test_host_form_equals_device_form(ctx, y_t, x_t):
    flat = _ints(y_t, x_t)
    refm = flat[NMAX].reshape((y_t, x_t), order="F")
    Dm = ((y_t - 1) // 2, (x_t - 1) // 2)
    for n, (d_y, d_x), (kind, units), use_ref in ((0, (0, 0), ("rand", "raster"), True), (1, Dm, ("null", "raster"), True),
                                                  (NMAX, (min(2, Dm[0]), min(3, Dm[1])), ("rand", "image"), True),
                                                  (2, (min(1, Dm[0]), min(1, Dm[1])), ("neg", "raster"), False)):
        sh = _shifts(kind, units, y_t, x_t, n)
        mats = _mats(flat, n, y_t, x_t)
        host, hsc = ctx.raster_register(mats, d_y, d_x, refm if use_ref else None, sh, units, GRID, want_scores=True)
        assert np.array_equal(ctx.raster_register(mats, d_y, d_x, refm if use_ref else None, sh, units, GRID), host)
        with D.Arenas(ctx) as A:
            r = A.input("rasters", flat[:max(n, 1)], 4)
            rf = A.input("ref", refm.reshape(-1, order="F"), 4) if use_ref else None
            s = A.input("shifts", sh, 4) if sh is not None and n else None
            out = A.output("shifts_out", max(n, 1) * 8, 4)
            sc = A.output("scores", max(n, 1) * (2 * d_y + 1 + 2 * d_x + 1) * 8, 8)
            ctx.raster_register_d(r.addr, n, y_t, x_t, d_y, d_x, out.addr, None if rf is None else rf.addr, None if s is None else s.addr,
                                  units, GRID, sc.addr)
            A.check()
            dev, dsc = out.get(np.int32).reshape(-1, 2)[:n], sc.get(np.float64).reshape(max(n, 1), -1)[:n]
        want = R.register(mats, refm if use_ref else None, d_y, d_x, _pairs(sh), units, GRID)
        _check_register(host, hsc, want, (n, kind, "host"))
        _check_register(dev, dsc, want, (n, kind, "device"))
    col, row = ctx.raster_profiles(_mats(flat, 2, y_t, x_t))
    m = np.stack(_mats(flat, 2, y_t, x_t)).astype(np.float64)
    assert np.array_equal(col, m.sum(axis=1)) and np.array_equal(row, m.sum(axis=2))


def test_every_refusal_writes_nothing(ctx):
    y_t, x_t, n = 65, 5, 3
    flat = _ints(y_t, x_t)
    sh = _shifts("rand", "raster", y_t, x_t, n)
    reg, prof = ctx.lib.tsdr_raster_register_d, ctx.lib.tsdr_raster_profiles_d
    with D.Arenas(ctx) as A:
        r, rf, s = A.input("rasters", flat[:n], 4), A.input("ref", flat[NMAX], 4), A.input("shifts", sh, 4)
        # INPUT arenas for the outputs too: their payloads must come back untouched
        out = A.input("shifts_out", np.full(2 * n, 12345, np.int32), 4)
        sc = A.input("scores", np.full(n * 6, 1.5, np.float64), 8)
        col, row = A.input("col", np.full(n * x_t, 2.5, np.float64), 8), A.input("row", np.full(n * y_t, 3.5, np.float64), 8)
        ok = dict(rasters=r.addr, n=n, y_t=y_t, x_t=x_t, ref=rf.addr, shifts=s.addr, units=0, img_h=600, img_w=800, d_y=1, d_x=1,
                  out=out.addr, scores=sc.addr)
        bad = [dict(y_t=0), dict(y_t=-5), dict(x_t=0), dict(x_t=-1), dict(n=-1), dict(y_t=1 << 16, x_t=1 << 15), dict(y_t=46341, x_t=46341),
               dict(rasters=None), dict(units=2), dict(units=-1), dict(units=1, img_h=0), dict(units=1, img_w=0), dict(units=1, img_h=-600),
               dict(rasters=r.addr + 2), dict(shifts=s.addr + 2),                           # ... what tsdr_raster_accum_d refuses
               dict(d_y=-1), dict(d_x=-1), dict(d_y=33), dict(d_x=3), dict(d_y=INT_MAX), dict(d_x=INT_MAX), dict(out=None),
               dict(ref=rf.addr + 2), dict(out=out.addr + 2), dict(out=out.addr + 1), dict(scores=sc.addr + 4), dict(scores=sc.addr + 2)]
        for change in bad:
            a = dict(ok, **change)
            rc = reg(ctx.h, a["rasters"], a["n"], a["y_t"], a["x_t"], a["ref"], a["shifts"], a["units"], a["img_h"], a["img_w"], a["d_y"],
                     a["d_x"], a["out"], a["scores"])
            assert rc == EINVAL, (change, rc)
            assert b"raster_register" in ctx.lib.tsdr_last_error(ctx.h), change
        for change in (dict(y_t=0), dict(x_t=-1), dict(n=-1), dict(y_t=46341, x_t=46341), dict(rasters=None), dict(rasters=r.addr + 2),
                       dict(col=col.addr + 4), dict(row=row.addr + 4), dict(row=row.addr + 2)):
            a = dict(dict(rasters=r.addr, n=n, y_t=y_t, x_t=x_t, col=col.addr, row=row.addr), **change)
            rc = prof(ctx.h, a["rasters"], a["n"], a["y_t"], a["x_t"], a["col"], a["row"])
            assert rc == EINVAL, (change, rc)
            assert b"raster_profiles" in ctx.lib.tsdr_last_error(ctx.h), change
        # the host form refuses the same before it stages anything
        hout = np.full((n, 2), 777, np.int32)
        for change in (dict(d_y=33), dict(d_x=-1), dict(units=2), dict(y_t=0)):
            a = dict(ok, **change)
            rc = ctx.lib.tsdr_raster_register(ctx.h, flat.ctypes.data, n, a["y_t"], a["x_t"], None, None, a["units"], 600, 800, a["d_y"], a["d_x"],
                                              hout.ctypes.data, None)
            assert rc == EINVAL and np.all(hout == 777), change
        assert ctx.lib.tsdr_raster_register(ctx.h, flat.ctypes.data, n, y_t, x_t, None, None, 0, 600, 800, 1, 1, None, None) == EINVAL
        with pytest.raises(AssertionError):
            ctx.raster_register(_mats(flat, n, y_t, x_t), 1, 1, units="pixels")
        # n_frames == 0 is fine with NULL everywhere and touches nothing; (2*d + 1 == size is still distinct)
        assert reg(ctx.h, None, 0, y_t, x_t, None, None, 0, 0, 0, 32, 2, None, None) == 0
        assert prof(ctx.h, None, 0, y_t, x_t, col.addr, row.addr) == 0
        n0, q = C.c_int(-1), np.full(4, 9, np.int32)
        assert ctx.lib.tsdr_frames_hires_shifts(ctx.h, -1, q.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n0)) == EINVAL
        assert ctx.lib.tsdr_frames_hires_shifts(ctx.h, 2, None, C.byref(n0)) == EINVAL and n0.value == -1 and np.all(q == 9)
        with pytest.raises(Exception):
            ctx.set_option("hires_refine", 9)
        with pytest.raises(Exception):
            ctx.set_option("hires_refine", -1)
        A.check()                             # every payload and every guard word as uploaded
        # ... and the context still works
        out2, sc2 = A.output("shifts_out after", n * 8, 4), A.output("scores after", n * 6 * 8, 8)
        _register_d(ctx, r, n, y_t, x_t, rf, s, "raster", 1, 1, out2, sc2)
        A.check()
        want = R.register(_mats(flat, n, y_t, x_t), flat[NMAX].reshape((y_t, x_t), order="F"), 1, 1, _pairs(sh))
        _check_register(out2.get(np.int32).reshape(n, 2), sc2.get(np.float64).reshape(n, -1), want, "after the refusals")


# ---------------------------------------------------------------- the whole loop
GEOMS = RH.GEOMS
ALPHA, ALPHA_H = RH.ALPHA, RH.ALPHA_H
NPX = GRID[0] * GRID[1]


def _run(ctx, tsdr, name, *, refine, chunk=0, do_align=True, split=None):
    """one pass over the capture through tsdr_frames_hires_iq_d on device buffers, in one call or (split: frames in the first) two
    -> dict(n, state, frames, idx, hires, shifts: what tsdr_frames_hires_shifts returned after each call)"""
    g = GEOMS[name]
    iq, S = RH.capture(name)
    y_t, x_t, nfr = g["y_t"], g["x_t"], g["nfr"]
    bounds = [(0, nfr)] if split is None else [(0, split), (split, nfr)]
    sync = tsdr.SyncXY(ctx, *GRID) if do_align else None
    ctx.set_option("hires_chunk_frames", chunk)
    ctx.set_option("hires_refine", refine)
    try:
        with D.Arenas(ctx) as A:
            d_iq = A.input("iq", iq, 0)
            st = _inout(A, "imageOut", np.zeros(NPX, np.float32), 0)
            hs = _inout(A, "hires_state", np.zeros(y_t * x_t, np.float32), 4)
            fr = A.output("frames_out", nfr * NPX * 4, 0)
            ix = A.output("sync_idx", nfr * 8, 4)
            total, shifts = 0, []
            for f0, f1 in bounds:
                nE = (f1 - f0) * S + (g["extra"] if f1 == nfr else 0)
                n = C.c_int(0)
                ctx.call("tsdr_frames_hires_iq_d", C.c_void_p(sync.h if sync is not None else 0), C.c_void_p(d_iq.addr + f0 * S * 8), 0,
                         C.c_float(1.0), nE, S, y_t, x_t, C.c_float(ALPHA), int(do_align), st.ptr, C.c_void_p(fr.addr + f0 * NPX * 4),
                         C.c_float(ALPHA_H), hs.ptr, C.c_void_p(ix.addr + f0 * 8), C.byref(n))
                total += n.value
                shifts.append(ctx.hires_shifts())
            A.check()
            return dict(n=total, state=st.get(np.float32), frames=fr.get(np.float32), idx=ix.get(np.int32).reshape(nfr, 2),
                        hires=hs.get(np.float32, (y_t, x_t), "F"), shifts=shifts)
    finally:
        ctx.set_option("hires_chunk_frames", 0)
        ctx.set_option("hires_refine", 0)


@functools.lru_cache(maxsize=None)
def _want(name, refine, chunk, split=None):
    """the reference loop on the oracle's rasters and indices, call by call and chunk by chunk with the state evolving
    -> (final state, [applied shifts of each call])"""
    g, o = GEOMS[name], RH.oracle(name)
    st = np.zeros((g["y_t"], g["x_t"]), np.float32, order="F")
    bounds = [(0, g["nfr"])] if split is None else [(0, split), (split, g["nfr"])]
    shifts = []
    for f0, f1 in bounds:
        st, sh, _, _ = R.refined_loop(o["raster"][f0:f1], o["sync_idx"][f0:f1], st, ALPHA_H, 1, chunk=chunk, refine=bool(refine))
        shifts.append(sh)
    return st, shifts


def _same_600x800(a, b):
    assert a["n"] == b["n"]
    assert np.array_equal(a["state"].view(np.uint32), b["state"].view(np.uint32)), "imageOut"
    assert np.array_equal(a["frames"].view(np.uint32), b["frames"].view(np.uint32)), "frames_out"
    assert np.array_equal(a["idx"], b["idx"]), "sync_idx"


@pytest.mark.parametrize("chunk", [0, 1, 2])
@pytest.mark.parametrize("name", list(GEOMS))
def test_loop_exact(ctx, tsdr, name, chunk):
    """TSDR_EXACT: with the option at 1 the 600x800 outputs are bit-identical to the run with the option at 0; the applied shifts are
    the reference's; hires_state is hires_ref.accumulate with those shifts, bit for bit.  With the option at 0,
    tsdr_frames_hires_shifts returns the resolved coarse shifts."""
    g, o = GEOMS[name], RH.oracle(name)
    with _exact(ctx):
        off = _run(ctx, tsdr, name, refine=0, chunk=chunk)
        on = _run(ctx, tsdr, name, refine=1, chunk=chunk)
    _same_600x800(on, off)
    assert on["n"] == g["nfr"] and np.array_equal(on["idx"], o["sync_idx"])
    for got, refine in ((off, 0), (on, 1)):
        st, shifts = _want(name, refine, chunk)
        assert np.array_equal(got["shifts"][0], shifts[0]), (refine, got["shifts"][0].tolist(), shifts[0].tolist())
        assert same_bits(got["hires"], st), ("hires_state", refine)
    assert not np.array_equal(on["shifts"][0], off["shifts"][0]), "the refinement moves at least one frame on this input"


@pytest.mark.parametrize("name", list(GEOMS))
def test_loop_exact_over_two_buffers(ctx, tsdr, name):
    """the second buffer registers to the state the first left"""
    g = GEOMS[name]
    split = g["nfr"] // 2 + 1
    with _exact(ctx):
        off = _run(ctx, tsdr, name, refine=0, split=split)
        on = _run(ctx, tsdr, name, refine=1, split=split)
    _same_600x800(on, off)
    st, shifts = _want(name, 1, 0, split)
    assert [s.shape[0] for s in on["shifts"]] == [split, g["nfr"] - split]
    assert all(np.array_equal(a, b) for a, b in zip(on["shifts"], shifts)), ([s.tolist() for s in on["shifts"]], [s.tolist() for s in shifts])
    assert same_bits(on["hires"], st)
    # registered to the FIRST buffer's state, not to its own first frame: the second call's shifts differ from a cold start's
    cold = R.refined_loop(RH.oracle(name)["raster"][split:], RH.oracle(name)["sync_idx"][split:],
                          np.zeros((g["y_t"], g["x_t"]), np.float32, order="F"), ALPHA_H, 1)[1]
    print(f"{name}: second buffer {shifts[1].tolist()}, from a cold start {cold.tolist()}")


@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("name", list(GEOMS))
def test_loop_fast(ctx, tsdr, name, chunk):
    """TSDR_FAST: the shifts are the reference's (every top-2 score margin exceeds 1e-9, asserted on the host), hires_state within
    the bound of tests/test_hires_gpu.py::test_loop_fast: RTOL + 4 * 2^-24 / (1 - alpha) relative."""
    assert ctx.precision == "fast"
    got = _run(ctx, tsdr, name, refine=1, chunk=chunk)
    st, shifts = _want(name, 1, chunk)
    assert got["n"] == GEOMS[name]["nfr"] and np.array_equal(got["idx"], RH.oracle(name)["sync_idx"])
    assert np.array_equal(got["shifts"][0], shifts[0]), (got["shifts"][0].tolist(), shifts[0].tolist())
    want = np.asarray(st, np.float64)
    assert want.min() > 0.0
    rel = float(np.max(np.abs(np.asarray(got["hires"], np.float64) - want) / want))
    bound = RTOL + 4 * 2.0 ** -24 / (1.0 - float(ALPHA_H))
    print(f"{name} chunk {chunk}: max relative error {rel:.3e} (bound {bound:.3e})")
    assert bound < 9e-7 and rel <= bound


@pytest.mark.parametrize("name", list(GEOMS))
def test_option_has_no_effect_without_alignment(ctx, tsdr, name):
    with _exact(ctx):
        off = _run(ctx, tsdr, name, refine=0, do_align=False, chunk=2)
        on = _run(ctx, tsdr, name, refine=1, do_align=False, chunk=2)
    assert on["n"] == off["n"] == GEOMS[name]["nfr"]
    assert np.array_equal(on["state"].view(np.uint32), off["state"].view(np.uint32)) and np.array_equal(on["frames"].view(np.uint32), off["frames"].view(np.uint32))
    assert same_bits(on["hires"], off["hires"])
    assert same_bits(on["hires"], H.accumulate(RH.oracle(name)["raster"], np.zeros_like(on["hires"]), ALPHA_H))
    assert on["shifts"][0].shape == (0, 2) and off["shifts"][0].shape == (0, 2), "n = 0 without do_align"


def test_residual_ratio_on_the_gpu_states(ctx, tsdr):
    """the sharpening measure of test_register_host.py on the states the GPU loop produced (TSDR_EXACT, so they are the
    reference's bit for bit: the strict inequality carries over)"""
    name = "150x2400"
    o = RH.oracle(name)
    with _exact(ctx):
        off, on = _run(ctx, tsdr, name, refine=0), _run(ctx, tsdr, name, refine=1)
    res_c, res_r = RH.residual(o["raster"], off["shifts"][0], off["hires"]), RH.residual(o["raster"], on["shifts"][0], on["hires"])
    print(f"{name}: residual coarse {res_c:.6e}, refined {res_r:.6e}, ratio {res_r / res_c:.4f}")
    assert res_r < res_c
