"""Display export -- the ROI of f32 pictures as bytes, stretched over a fixed range, the ROI's finite minimum / maximum, or two
percentiles of it -- through the entry points of include/tempest_hip_display.h.  Every call of their symbols is here;
api.Context.display_u8 and Context.display_u8_d delegate to this module.  The loop a viewer runs is frames_d -> display_u8_d ->
download the bytes: a quarter of the f32 download, less when cropped."""
import numpy as np

from ._lib import DISPLAY_INVERT, DISPLAY_SHARED, RANGE_FIXED, RANGE_MINMAX, RANGE_PERCENTILE

MODES = {"fixed": RANGE_FIXED, "minmax": RANGE_MINMAX, "percentile": RANGE_PERCENTILE}


def _mode(mode):
    if mode not in MODES:
        raise ValueError(f"unknown range mode {mode!r} (fixed, minmax, percentile)")
    return MODES[mode]


def _roi(roi, h, w):
    """(i0, j0, rh, rw); None = the whole picture"""
    return (0, 0, int(h), int(w)) if roi is None else tuple(int(v) for v in roi)


def _flags(invert, shared):
    return (DISPLAY_INVERT if invert else 0) | (DISPLAY_SHARED if shared else 0)


def display_u8_d(ctx, images, n_images, h, w, out, roi=None, mode="minmax", lo=0.0, hi=1.0, p=(0.01, 0.99), invert=False, shared=False,
                 ranges_out=None):
    """device pointers: images = n_images column-major (h, w) float32 pictures, h*w floats apart; out (n_images * rh * rw bytes, any
    alignment, or None) receives the ROI (i0, j0, rh, rw) of each as bytes, mapped over the range of `mode` ("fixed": (lo, hi);
    "minmax"; "percentile": the fractions p); ranges_out (2 * n_images float32, or None) the ranges used.  shared: one range for
    all pictures of the call.  Enqueues on the context's stream and returns -- tsdr_display_u8_d"""
    import ctypes as C

    from . import api
    i0, j0, rh, rw = _roi(roi, h, w)
    ctx.call("tsdr_display_u8_d", api._ptr(images), int(n_images), int(h), int(w), i0, j0, rh, rw, _mode(mode), C.c_float(lo), C.c_float(hi),
             C.c_double(p[0]), C.c_double(p[1]), _flags(invert, shared), api._ptr(out), api._ptr(ranges_out))


def display_u8(ctx, images, roi=None, mode="minmax", lo=0.0, hi=1.0, p=(0.01, 0.99), invert=False, shared=False):
    """host arrays: images = n matrices (h, w) -> (bytes (n, rh, rw) uint8, ranges (n, 2) float32) -- tsdr_display_u8"""
    import ctypes as C

    from . import api
    n = len(images)
    h, w = np.shape(images[0]) if n else (1, 1)
    flat = np.empty((n, h * w), np.float32)
    for f in range(n):
        m = np.asarray(images[f], np.float32)
        if m.shape != (h, w):
            raise AssertionError(f"picture {f} is {m.shape}, expected {(h, w)}")
        flat[f] = m.reshape(-1, order="F")
    i0, j0, rh, rw = _roi(roi, h, w)
    out = np.zeros((n, max(rh, 0) * max(rw, 0)), np.uint8)
    ranges = np.zeros((n, 2), np.float32)
    ctx.call("tsdr_display_u8", api._ptr(flat), n, int(h), int(w), i0, j0, rh, rw, _mode(mode), C.c_float(lo), C.c_float(hi), C.c_double(p[0]),
             C.c_double(p[1]), _flags(invert, shared), api._ptr(out), api._ptr(ranges))
    return np.stack([o.reshape((rh, rw), order="F") for o in out]) if n else out.reshape(0, rh, rw), ranges
