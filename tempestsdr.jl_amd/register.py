"""Registration of the full-size rasters to the raster pixel -- column / row sums in f64, correlation scores against a reference
picture, the ordered choice -- through the entry points of include/tempest_hip_register.h.  Every call of their symbols is here;
api.Context.raster_profiles, Context.raster_register, Context.raster_register_d and Context.hires_shifts delegate to this module.
The frame loop uses the same registration under the context option "hires_refine" (Context.set_option)."""
import ctypes as C

import numpy as np

from ._lib import RENDER_H, RENDER_W
from .hires import _units


def _flat(rasters, y_t, x_t):
    n = len(rasters)
    flat = np.empty((n, y_t * x_t), np.float32)
    for f in range(n):
        r = np.asarray(rasters[f], np.float32)
        if r.shape != (y_t, x_t):
            raise AssertionError(f"raster {f} is {r.shape}, expected {(y_t, x_t)}")
        flat[f] = r.reshape(-1, order="F")
    return flat


def raster_profiles_d(ctx, rasters, n_frames, y_t, x_t, col=None, row=None):
    """device pointers: col (n_frames * x_t float64) and row (n_frames * y_t float64), either may be None, receive the column
    and row sums of n_frames rasters, P floats apart.  Enqueues on the context's stream and returns -- tsdr_raster_profiles_d"""
    from . import api
    ctx.call("tsdr_raster_profiles_d", api._ptr(rasters), int(n_frames), int(y_t), int(x_t), api._ptr(col), api._ptr(row))


def raster_profiles(ctx, rasters):
    """host arrays: rasters = n matrices (y_t, x_t) -> (col (n, x_t), row (n, y_t)) float64, the sums over rows and over columns"""
    n = len(rasters)
    if n == 0:
        return np.zeros((0, 0)), np.zeros((0, 0))
    y_t, x_t = np.shape(rasters[0])
    flat = _flat(rasters, y_t, x_t)
    bufs = []
    try:
        d_r = ctx.upload(flat); bufs.append(d_r)
        d_c = ctx.dev_alloc(n * x_t * 8); bufs.append(d_c)
        d_w = ctx.dev_alloc(n * y_t * 8); bufs.append(d_w)
        raster_profiles_d(ctx, d_r, n, y_t, x_t, d_c, d_w)
        return ctx.download(d_c, (n, x_t), np.float64), ctx.download(d_w, (n, y_t), np.float64)
    finally:
        ctx.synchronize()
        for p in bufs:
            ctx.dev_free(p)


def n_scores(d_y, d_x):
    """scores per frame: the y block (2*d_y + 1), then the x block (2*d_x + 1)"""
    return 2 * int(d_y) + 1 + 2 * int(d_x) + 1


def raster_register_d(ctx, rasters, n_frames, y_t, x_t, d_y, d_x, shifts_out, ref=None, shifts=None, units="raster",
                      grid=(RENDER_H, RENDER_W), scores=None):
    """device pointers: shifts_out (2 * n_frames int32, raster units) <- the coarse shifts (`shifts` in `units`, or None = 0)
    refined by at most d_y lines / d_x pixels against ref (a (y_t, x_t) raster, or None = frame 0); scores: None or
    n_frames * n_scores(d_y, d_x) float64.  Enqueues on the context's stream and returns -- tsdr_raster_register_d"""
    from . import api
    ctx.call("tsdr_raster_register_d", api._ptr(rasters), int(n_frames), int(y_t), int(x_t), api._ptr(ref), api._ptr(shifts), _units(units),
             int(grid[0]), int(grid[1]), int(d_y), int(d_x), api._ptr(shifts_out), api._ptr(scores))


def raster_register(ctx, rasters, d_y, d_x, ref=None, shifts=None, units="raster", grid=(RENDER_H, RENDER_W), want_scores=False):
    """host arrays: rasters = n matrices (y_t, x_t); ref a (y_t, x_t) matrix or None; shifts = n pairs (s_y, s_x) or None.
    -> the refined shifts, an (n, 2) int32 array in raster units (with want_scores: (shifts, scores (n, n_scores) float64))
    -- tsdr_raster_register"""
    from . import api
    n = len(rasters)
    y_t, x_t = np.shape(rasters[0]) if n else np.shape(ref) if ref is not None else (1, 1)
    flat = _flat(rasters, y_t, x_t)
    r = None
    if ref is not None:
        r = np.asarray(ref, np.float32)
        if r.shape != (y_t, x_t):
            raise AssertionError(f"ref is {r.shape}, the rasters {(y_t, x_t)}")
        r = np.ascontiguousarray(r.reshape(-1, order="F"))
    sh = None
    if shifts is not None:
        sh = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1)
        if sh.size != 2 * n:
            raise AssertionError(f"shifts must hold {n} (s_y, s_x) pairs")
    out = np.zeros((n, 2), np.int32)
    sc = np.zeros((n, n_scores(d_y, d_x)), np.float64) if want_scores else None
    ctx.call("tsdr_raster_register", api._ptr(flat), n, int(y_t), int(x_t), api._ptr(r), api._ptr(sh), _units(units), int(grid[0]),
             int(grid[1]), int(d_y), int(d_x), api._ptr(out), api._ptr(sc))
    return (out, sc) if want_scores else out


def hires_shifts(ctx, max_frames=1 << 16):
    """the (s_y, s_x) in raster units, one row per frame, that the most recent frames_hires call on this context averaged its
    rasters with -- refined under "hires_refine", the resolved sync indices otherwise; no rows when it ran without alignment.
    Synchronises -- tsdr_frames_hires_shifts"""
    n = C.c_int(0)
    ctx.call("tsdr_frames_hires_shifts", 0, None, C.byref(n))
    m = min(n.value, int(max_frames))
    out = np.zeros((m, 2), np.int32)
    if m:
        ctx.call("tsdr_frames_hires_shifts", m, out.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n))
    return out
