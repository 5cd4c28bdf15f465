"""numpy reference of the registration rule of include/tempest_hip_register.h: profiles in float64 (math.fsum for the bound tests,
plain float64 sums otherwise), the coarse shift by tests/hires_ref.py, scores as product-then-sum in float64, the ordered choice.
`register` is the vectorised form the GPU tests compare against; `brute` is the definition element by element in Python ints and
floats.  Shared by tests/test_register_host.py and tests/test_register_gpu.py."""
import math

import numpy as np

import hires_ref as H


def profiles(raster):
    """-> (col (x_t,), row (y_t,)) float64: sums over rows and over columns, every value converted to f64 first"""
    r = np.asarray(raster, np.float32).astype(np.float64)
    return r.sum(axis=0), r.sum(axis=1)


def profiles_fsum(raster):
    """the same, correctly rounded (math.fsum), with sum|x| per element for the error bound"""
    r = np.asarray(raster, np.float32).astype(np.float64)
    col = np.array([math.fsum(r[:, j]) for j in range(r.shape[1])])
    row = np.array([math.fsum(r[i, :]) for i in range(r.shape[0])])
    return col, row, np.abs(r).sum(axis=0), np.abs(r).sum(axis=1)


def is_flat(p):
    """every element compares IEEE-equal to element 0 (a NaN anywhere: not flat)"""
    return bool(np.all(p == p[0]))


def coarse(shifts, f, y_t, x_t, units, grid):
    if shifts is None:
        return 0, 0
    return H.resolve(shifts[f][0], y_t, units, grid[0]), H.resolve(shifts[f][1], x_t, units, grid[1])


def pick(scores, D):
    """the ordered choice over scores[d + D]: 0, -1, +1, -2, +2, ...; replaced on a strict > only"""
    best, bd = scores[D], 0
    for m in range(1, D + 1):
        for d in (-m, m):
            if scores[D + d] > best:
                best, bd = scores[D + d], d
    return bd


def axis_scores(refp, prof, r0, D):
    """s(d) = sum_j refp[j] * prof[(j + r0 + d) mod size], d = -D .. D"""
    with np.errstate(all="ignore"):
        return np.array([np.sum(refp * np.roll(prof, -(r0 + d))) for d in range(-D, D + 1)], np.float64)


def register(rasters, ref, d_y, d_x, shifts=None, units="raster", grid=(600, 800)):
    """-> (shifts_out (n, 2) int32 in raster units, scores (n, 2*d_y+1 + 2*d_x+1) float64, d (n, 2) the chosen refinements)"""
    n = len(rasters)
    out, sc, ds = np.zeros((n, 2), np.int32), np.zeros((n, 2 * d_y + 1 + 2 * d_x + 1), np.float64), np.zeros((n, 2), np.int64)
    if n == 0:
        return out, sc, ds
    y_t, x_t = np.shape(rasters[0])
    prof = [profiles(r) for r in rasters]               # (col, row) per frame
    r00 = coarse(shifts, 0, y_t, x_t, units, grid)
    refs = []
    for axis in (0, 1):                                 # 0: y (row profile), 1: x (column profile)
        p = None if ref is None else profiles(ref)[1 - axis]
        if p is None or is_flat(p):
            p = np.roll(prof[0][1 - axis], -r00[axis])  # frame 0's profile rotated by its coarse shift
        refs.append(p)
    for f in range(n):
        r0 = coarse(shifts, f, y_t, x_t, units, grid)
        sy = axis_scores(refs[0], prof[f][1], r0[0], d_y)
        sx = axis_scores(refs[1], prof[f][0], r0[1], d_x)
        dy, dx = pick(sy, d_y), pick(sx, d_x)
        sc[f] = np.concatenate([sy, sx])
        ds[f] = dy, dx
        out[f] = (r0[0] + dy) % y_t, (r0[1] + dx) % x_t
    return out, sc, ds


def brute(rasters, ref, d_y, d_x, shifts=None, units="raster", grid=(600, 800)):
    """the definition, element by element: Python ints for the shift rule, Python floats (f64), product then sum in index order"""
    n = len(rasters)
    if n == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2 * d_y + 1 + 2 * d_x + 1))
    y_t, x_t = np.shape(rasters[0])
    size = (y_t, x_t)

    def prof(r, axis):   # axis 0: row sums (length y_t); 1: column sums (length x_t)
        r = np.asarray(r, np.float32)
        if axis == 0:
            return [sum((float(r[i, j]) for j in range(x_t)), 0.0) for i in range(y_t)]
        return [sum((float(r[i, j]) for i in range(y_t)), 0.0) for j in range(x_t)]

    def r0_of(f, axis):
        if shifts is None:
            return 0
        a = int(shifts[f][axis])
        if H.UNITS[units] == H.RASTER:
            return a % size[axis]
        return ((2 * a * size[axis] + grid[axis]) // (2 * grid[axis])) % size[axis]

    out, sc = np.zeros((n, 2), np.int32), []
    for f in range(n):
        row_scores = []
        for axis, D in ((0, d_y), (1, d_x)):
            m = size[axis]
            p = None if ref is None else prof(ref, axis)
            if p is None or all(v == p[0] for v in p):
                p0, s0 = prof(rasters[0], axis), r0_of(0, axis)
                p = [p0[(j + s0) % m] for j in range(m)]
            q, r0 = prof(rasters[f], axis), r0_of(f, axis)
            s = []
            for d in range(-D, D + 1):
                acc = 0.0
                for j in range(m):
                    acc = acc + p[j] * q[(j + r0 + d) % m]
                s.append(acc)
            best, bd = s[D], 0
            for k in range(1, D + 1):
                if s[D - k] > best:
                    best, bd = s[D - k], -k
                if s[D + k] > best:
                    best, bd = s[D + k], k
            out[f, axis] = (r0 + bd) % m
            row_scores += s
        sc.append(row_scores)
    return out, np.array(sc, np.float64)


def margins(scores, d_y, d_x):
    """per frame and axis: (best - second) / |best| over the axis's candidates (inf with a single candidate)"""
    out = []
    for row in np.atleast_2d(scores):
        m = []
        for blk in (row[:2 * d_y + 1], row[2 * d_y + 1:]):
            s = np.sort(blk)[::-1]
            m.append(np.inf if s.size < 2 else (s[0] - s[1]) / abs(s[0]))
        out.append(m)
    return np.array(out)


def refined_loop(rasters, sync_idx, state, alpha, k, chunk=0, grid=(600, 800), refine=True):
    """the loop of tempest_hip_register.h (THE LOOP) on given rasters and sync indices: per chunk, register against the state as
    the chunk finds it (D from k), then hires_ref.accumulate with the refined raster-unit shifts.
    refine=False: the coarse shifts alone, resolved to raster units.
    -> (state, applied shifts (n, 2) in raster units, the scores of each chunk, (D_y, D_x))"""
    n = len(rasters)
    y_t, x_t = np.shape(state)
    d_y = min(-(-k * y_t // grid[0]), (y_t - 1) // 2)
    d_x = min(-(-k * x_t // grid[1]), (x_t - 1) // 2)
    st = np.array(state, np.float32, copy=True, order="F")
    step = n if chunk <= 0 else chunk
    applied, all_scores = [], []
    for f0 in range(0, n, step):
        rs, idx = rasters[f0:f0 + step], [tuple(int(v) for v in row) for row in sync_idx[f0:f0 + step]]
        if refine:
            sh, sc, _ = register(rs, st, d_y, d_x, idx, "image", grid)
            all_scores.append(sc)
        else:
            sh = np.array([coarse(idx, f, y_t, x_t, "image", grid) for f in range(len(rs))], np.int32).reshape(-1, 2)
        st = H.accumulate(rs, st, alpha, [tuple(int(v) for v in row) for row in sh], "raster")
        applied.append(sh)
    return st, np.concatenate(applied) if applied else np.zeros((0, 2), np.int32), all_scores, (d_y, d_x)
