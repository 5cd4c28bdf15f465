"""Frame averaging at the monitor's own resolution -- the aligned one-pole IIR of GUI.jl:171-175 on the y_t x x_t rasters instead
of the 600x800 rendering image -- through the entry points of include/tempest_hip_hires.h.  Every call of their symbols is here;
api.Context.raster_accumulate, Context.raster_accumulate_d, Context.frames_hires and Context.frames_hires_d delegate to this
module."""
import ctypes as C

import numpy as np

from ._lib import RENDER_H, RENDER_W, SHIFT_IMAGE, SHIFT_RASTER

UNITS = {"raster": SHIFT_RASTER, "image": SHIFT_IMAGE}


def _units(units):
    if units in UNITS:
        return UNITS[units]
    if isinstance(units, (int, np.integer)) and not isinstance(units, bool):
        return int(units)      # (an unknown code is the library's TSDR_EINVAL)
    raise AssertionError(f"unknown shift units {units!r} ('raster', 'image')")


def _state(a, y_t, x_t, what):
    if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.f_contiguous and a.shape == (y_t, x_t)):
        raise AssertionError(f"{what} must be a Fortran-order float32 ({y_t},{x_t}) array")
    return a


def raster_accum_d(ctx, rasters, n_frames, y_t, x_t, alpha, state, shifts=None, units="raster", grid=(RENDER_H, RENDER_W)):
    """device pointers: state (y_t x x_t, column-major) <- the IIR over n_frames rasters, P floats apart, each shifted by its
    (s_y, s_x) of `shifts` (2*n_frames int32 on the device, or None) in `units`.  Enqueues on the context's stream and returns --
    tsdr_raster_accum_d"""
    from . import api
    ctx.call("tsdr_raster_accum_d", api._ptr(rasters), int(n_frames), int(y_t), int(x_t), api._ptr(shifts), _units(units), int(grid[0]),
             int(grid[1]), C.c_float(alpha), api._ptr(state))


def raster_accumulate(ctx, rasters, state, alpha, shifts=None, units="raster", grid=(RENDER_H, RENDER_W)):
    """host arrays: rasters = n matrices (y_t, x_t) (a list, or an (n, y_t, x_t) array), state a Fortran-order float32 (y_t, x_t)
    array updated in place and returned; shifts = n pairs (s_y, s_x) or None -- tsdr_raster_accum"""
    from . import api
    if not (isinstance(state, np.ndarray) and state.ndim == 2):
        raise AssertionError("state must be a Fortran-order float32 matrix")
    y_t, x_t = state.shape
    _state(state, y_t, x_t, "state")
    n = len(rasters)
    flat = np.empty((n, y_t * x_t), np.float32)
    for f in range(n):
        r = np.asarray(rasters[f], np.float32)
        if r.shape != (y_t, x_t):
            raise AssertionError(f"raster {f} is {r.shape}, the state {(y_t, x_t)}")
        flat[f] = r.reshape(-1, order="F")
    sh = None
    if shifts is not None:
        sh = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1)
        if sh.size != 2 * n:
            raise AssertionError(f"shifts must hold {n} (s_y, s_x) pairs")
    ctx.call("tsdr_raster_accum", api._ptr(flat), n, y_t, x_t, api._ptr(sh), _units(units), int(grid[0]), int(grid[1]), C.c_float(alpha),
             api._ptr(state))
    return state


def frames_hires_d(ctx, sync, iq, fmt, scale, nEch, S, y_t, x_t, alpha, do_align, state, alpha_hires, hires_state, frames_out=None,
                   sync_idx=None):
    """frames_iq_d plus the full-size average: device buffers throughout (iq: nEch samples of `fmt`; state 600x800; hires_state
    y_t x x_t; frames_out / sync_idx optional); enqueues and returns the number of frames -- tsdr_frames_hires_iq_d"""
    from . import api
    n = C.c_int(0)
    ctx.call("tsdr_frames_hires_iq_d", C.c_void_p(sync.h if sync is not None else 0), api._ptr(iq), api.iq_fmt_code(fmt), C.c_float(scale),
             int(nEch), int(S), int(y_t), int(x_t), C.c_float(alpha), int(bool(do_align)), api._ptr(state), api._ptr(frames_out),
             C.c_float(alpha_hires), api._ptr(hires_state), api._ptr(sync_idx), C.byref(n))
    return n.value


def frames_hires(ctx, sync, iq, S, y_t, x_t, alpha, imageOut, alpha_hires, hires_state, iq_fmt=None, iq_scale=1.0, do_align=True,
                 want_frames=True):
    """One SDR buffer through the steady-state loop AND the full-size average.  iq: a complex array, or with iq_fmt "sc16" / "sc8" /
    "uc8" an integer array of 2*n interleaved components (uploaded as stored).  imageOut (600x800) and hires_state (y_t x x_t),
    Fortran-order float32, are updated in place.  Returns dict(n_frames, frames, sync_idx) like Context.frames."""
    from . import api
    y_t, x_t, S = int(y_t), int(x_t), int(S)
    _state(imageOut, RENDER_H, RENDER_W, "imageOut")
    _state(hires_state, y_t, x_t, "hires_state")
    if iq_fmt is None:
        a, code, nEch = api._c64(iq), 0, np.size(iq)
    else:
        a, code, nEch = api._int_iq(iq, iq_fmt, "frames_hires")
    nb = nEch // S
    bufs = []
    try:
        d_iq = ctx.upload(a if a.size else np.zeros(1, a.dtype)); bufs.append(d_iq)
        d_state = ctx.upload(imageOut.reshape(-1, order="F")); bufs.append(d_state)
        d_hires = ctx.upload(hires_state.reshape(-1, order="F")); bufs.append(d_hires)
        d_frames = None
        if want_frames:
            d_frames = ctx.dev_alloc(max(nb, 1) * RENDER_H * RENDER_W * 4); bufs.append(d_frames)
        d_idx = ctx.upload(np.zeros(max(nb, 1) * 2, np.int32)); bufs.append(d_idx)
        n = frames_hires_d(ctx, sync, d_iq, code, iq_scale, nEch, S, y_t, x_t, alpha, do_align, d_state, alpha_hires, d_hires, d_frames, d_idx)
        imageOut[...] = ctx.download(d_state, (RENDER_H * RENDER_W,), np.float32).reshape((RENDER_H, RENDER_W), order="F")
        hires_state[...] = ctx.download(d_hires, (y_t * x_t,), np.float32).reshape((y_t, x_t), order="F")
        out = {"n_frames": n, "sync_idx": ctx.download(d_idx, (max(nb, 1), 2), np.int32)[:nb]}
        if want_frames:
            fr = ctx.download(d_frames, (max(nb, 1), RENDER_H * RENDER_W), np.float32)
            out["frames"] = [fr[f].reshape((RENDER_H, RENDER_W), order="F") for f in range(nb)]
        return out
    finally:
        ctx.synchronize()
        for p in bufs:
            ctx.dev_free(p)
