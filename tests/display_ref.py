"""numpy reference of the display export, written from the contract in include/tempest_hip_display.h (RANGE of a group, MAPPING of
a pixel) in np.float32 scalar and array operations: every f32 operation is one correctly rounded numpy operation on float32
operands (numpy never fuses), the counts are int64, k_lo / k_hi are f64.

    display(images, roi, mode, lo, hi, p, invert, shared) -> (bytes (n, rh, rw) uint8, ranges (n, 2) float32)

images: n matrices (h, w); roi = (i0, j0, rh, rw) or None."""
import numpy as np

FIXED, MINMAX, PERCENTILE = 0, 1, 2
INVERT, SHARED = 1, 2
B = 4096
F = np.float32


def finite_stats(px):
    """(mn, mx, N) over the finite values of px (any shape); N == 0: (0, 0, 0)"""
    v = px[np.isfinite(px)]
    if v.size == 0:
        return F(0), F(0), 0
    return F(v.min()), F(v.max()), int(v.size)


def bins(px, mn, invw):
    """bin(v) of every FINITE value of px, int64"""
    v = px[np.isfinite(px)].astype(F)
    with np.errstate(all="ignore"):
        q = np.floor((v - F(mn)) * F(invw))
    return np.minimum(B - 1, q.astype(np.int64))


def edge(b, mn, mx, wd):
    return F(mx) if b == B else F(F(mn) + F(F(b) * F(wd)))


def group_range(px, mode, lo=0.0, hi=1.0, p=(0.0, 1.0)):
    """the (lo, hi) of one group's ROI pixels px (any shape, float32)"""
    if mode == FIXED:
        return F(lo), F(hi)
    mn, mx, N = finite_stats(px)
    if mode == MINMAX:
        return mn, mx
    with np.errstate(all="ignore"):
        d = F(mx - mn)
        invw = F(F(B) / d)
        wd = F(d / F(B))
    if not (d > 0) or not np.isfinite(d) or not np.isfinite(invw):
        return mn, mx
    counts = np.bincount(bins(px, mn, invw), minlength=B)
    cum = np.cumsum(counts)
    k_lo = int(np.floor(np.float64(p[0]) * np.float64(N - 1)))
    k_hi = int(np.ceil(np.float64(p[1]) * np.float64(N - 1)))
    b_lo = int(np.argmax(cum > k_lo))
    b_hi = int(np.argmax(cum > k_hi))
    return edge(b_lo, mn, mx, wd), edge(b_hi + 1, mn, mx, wd)


def map_pixels(px, lo, hi, invert=False):
    """the bytes of px (float32 array) over (lo, hi)"""
    with np.errstate(all="ignore"):
        dd = F(F(hi) - F(lo))
        s = F(F(255.0) / dd)
        if not (dd > 0) or not np.isfinite(dd) or not np.isfinite(s):
            return np.zeros(px.shape, np.uint8)
        q = (px.astype(F) - F(lo)) * s
    nan = np.isnan(q)
    q = np.where(nan, F(0), q)
    q = np.rint(np.clip(q, F(0), F(255)))          # np.rint: round half to even
    out = q.astype(np.uint8)
    if invert:
        out = (255 - out).astype(np.uint8)
        out[nan] = 0
    return out


def crop(img, roi):
    img = np.asarray(img, F)
    if roi is None:
        return img
    i0, j0, rh, rw = roi
    return img[i0:i0 + rh, j0:j0 + rw]


def display(images, roi=None, mode=MINMAX, lo=0.0, hi=1.0, p=(0.0, 1.0), invert=False, shared=False):
    rois = [crop(m, roi) for m in images]
    n = len(rois)
    if shared and n:
        r = group_range(np.stack(rois), mode, lo, hi, p)
        rng = [r] * n
    else:
        rng = [group_range(x, mode, lo, hi, p) for x in rois]
    out = [map_pixels(x, r[0], r[1], invert) for x, r in zip(rois, rng)]
    return (np.stack(out) if n else np.zeros((0, 0, 0), np.uint8)), np.array(rng, F).reshape(n, 2)


def full_scale_255(img):
    """fullScale! (ScreenRenderer.jl:35-39) times 255, rounded: the definition MINMAX restates, in its own operation order
    ((v - min) * (255 / (max - min))), all finite input"""
    img = np.asarray(img, F)
    mn, mx = F(img.min()), F(img.max())
    return np.rint((img - mn) * F(F(255.0) / F(mx - mn))).astype(np.uint8)
