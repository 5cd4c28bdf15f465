"""numpy reference of the full-resolution frame average (include/tempest_hip_hires.h): the shift rule in 64-bit integers with
floored division, np.roll for the circshift, and the recurrence as three separately rounded float32 operations (numpy rounds every
array operation on its own: there is no fused multiply-add to fall into).  Shared by tests/test_hires_host.py (which checks it
against a brute-force triple loop) and tests/test_hires_gpu.py."""
import numpy as np

RASTER, IMAGE = 0, 1
UNITS = {"raster": RASTER, "image": IMAGE, RASTER: RASTER, IMAGE: IMAGE}


def unreduced(a, size, units="raster", img=None):
    """the shift in raster lines / pixels BEFORE the reduction mod size: a itself, or floor((2*a*size + img) / (2*img))"""
    a, size = np.int64(a), np.int64(size)
    if UNITS[units] == RASTER:
        return a
    img = np.int64(img)
    return np.floor_divide(np.int64(2) * a * size + img, np.int64(2) * img)   # floored, as the contract says


def resolve(a, size, units="raster", img=None):
    """0 <= r < size (np.mod is the floored modulus: negatives wrap as circshift does)"""
    return int(np.mod(unreduced(a, size, units, img), np.int64(size)))


def accumulate(rasters, state, alpha, shifts=None, units="raster", grid=(600, 800)):
    """-> the new state (float32, (y_t, x_t)); `state` and `rasters` are left unchanged.  rasters: n matrices (y_t, x_t);
    shifts: n pairs (s_y, s_x) or None"""
    acc = np.array(state, np.float32, copy=True, order="F")
    y_t, x_t = acc.shape
    a = np.float32(alpha)
    oma = np.float32(1.0) - a                         # fsub(1, alpha)
    with np.errstate(all="ignore"):
        for f in range(len(rasters)):
            r = np.asarray(rasters[f], np.float32)
            assert r.shape == (y_t, x_t)
            if shifts is not None:
                r_y = resolve(shifts[f][0], y_t, units, grid[0])
                r_x = resolve(shifts[f][1], x_t, units, grid[1])
                r = np.roll(r, (-r_y, -r_x), axis=(0, 1))   # out[i, j] = r[(i + r_y) mod y_t, (j + r_x) mod x_t]
            p = a * acc                               # fmul(alpha, A)
            q = oma * r                               # fmul(1 - alpha, R)
            acc = (p + q).astype(np.float32)          # fadd
    return np.asfortranarray(acc)


def brute(rasters, state, alpha, shifts=None, units="raster", grid=(600, 800)):
    """the definition, pixel by pixel (Python ints for the shift rule, one np.float32 scalar operation per rounding)"""
    y_t, x_t = np.shape(state)
    out = np.array(state, np.float32, copy=True)
    a = np.float32(alpha)
    oma = np.float32(np.float32(1.0) - a)
    for f in range(len(rasters)):
        r_y = r_x = 0
        if shifts is not None:
            sy, sx = int(shifts[f][0]), int(shifts[f][1])
            if UNITS[units] == RASTER:
                r_y, r_x = sy % y_t, sx % x_t         # (Python's % and // are floored)
            else:
                r_y = ((2 * sy * y_t + grid[0]) // (2 * grid[0])) % y_t
                r_x = ((2 * sx * x_t + grid[1]) // (2 * grid[1])) % x_t
        for i in range(y_t):
            for j in range(x_t):
                v = np.float32(rasters[f][(i + r_y) % y_t][(j + r_x) % x_t])
                out[i, j] = np.float32(np.float32(a * out[i, j]) + np.float32(oma * v))
    return out
