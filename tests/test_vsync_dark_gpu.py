"""Option "vsync_blank_dark": frame sync on a DARK blanking interval (the reference's arg_area_blank = findmin,
FrameSynchronisation.jl:51-53) -- standalone vsync (f32, f64), the frame loop in TSDR_EXACT and TSDR_FAST with the sync guard,
the pipelined / split / integer-IQ / group routes, and the default polarity left untouched.

The oracle has no findmin.  Expected indices are numpy's FIRST MINIMUM in column-major order over the oracle's beta
(tests/oracle_lib.py, bit-identical to the library's beta): np.argmin(beta.ravel(order="F")) // W + 1, which also returns
the first NaN -- Julia's findmin.  They never come from where a band was drawn.

Every input compared against numpy was checked on the CPU with the oracle before it was committed: either the pick is
unique with a relative top-2 column margin (second - best) / second >= 1e-3 (cases 1, 3, 4, 6), or it is an exact tie in a
tie case (case 2).  Figures of that check (oracle beta, numpy; f64_ref for case 3):
  case 1 / 3   margins 1.41e-2 .. 1.42e-2 (x), 7.27e-2 .. 7.29e-2 (y) at 600x800; 4.9e-2 .. 5.0e-2 (x), 0.147 (y) at 120x200
               in f32 and f64; 6.6e-2 .. 6.8e-2 (x), 0.143 .. 0.148 (y) at 77x131, where the pick on beta_y is column 2 for all
               three images -- the start-up transient of the causal FIR is the darkest band on that axis, not the drawn one
  case 2       flat bands: 16 columns of beta_x and 2 of beta_y hold the minimum bit for bit (margin 0), first columns
               x = 445, y = 217.  All-zero: every column ties.  All-one: 398 columns of beta_x tie (first: 1); beta_y has ONE
               minimum, column 85, 2.0e-7 below the next column -- neither a tie nor a clear margin; the case is kept because
               the issue names it, and the test also holds beta itself to the oracle's bits, which decide it.  One NaN pixel:
               every beta value is NaN; one +Inf pixel: 405 / 305 columns hold a NaN, the first of them column 1.
  case 4 / 6   "box_dark" at 2 MS/s, 1056 x 628: margins 1.3e-3 .. 2.1e-3 (x), 2.6e-2 .. 3.3e-2 (y) over the frames used
  case 5       "plateau_dark" is compared against the EXACT route only, never against numpy: its five frames have beta_x
               margins 4.9e-6, 2.1e-5, 1.3e-6, 2.6e-5, 2.7e-5 (beta_y: 3.6e-4 .. 3.0e-3) -- the flat black interval leaves
               near-ties, not exact f32 ties (the capture carries noise), two of them far enough below the guard's 2e-5 that
               FAST's 1e-7-level beta error cannot lift them over it: at least those are re-evaluated
The GPU tests set the option through Context.set_option and restore 0 in a `finally`; on a library without the option that
call answers TSDR_EINVAL (unknown option), so each of them fails there.
"""
import ctypes as C
import hashlib
import importlib

import numpy as np
import pytest

import oracle_lib as O

RTOL = 6e-7          # tests/test_fast_mode_gpu.py's bar for FAST pixels
NPX = 600 * 800
OPT = "vsync_blank_dark"


# ---------------------------------------------------------------- numpy's findmin and the margin the inputs were checked with
def argmin_col(beta):
    """findmin(beta)[2][2]: 1-based column of the first minimum in column-major order; NaN is minimal, the first NaN wins"""
    b = np.asarray(beta)
    return int(np.argmin(b.ravel(order="F"))) // b.shape[0] + 1


def dark_margin(beta):
    """(1-based argmin column, (second - best) / second over the column minima; 0 for ties, NaN / Inf / all-zero beta)"""
    with np.errstate(invalid="ignore"):
        colmin = np.min(np.asarray(beta, np.float64), axis=0)   # (np.min propagates NaN, as findmin does)
    c = argmin_col(beta) - 1
    best = colmin[c]
    second = np.min(np.delete(colmin, c))
    if not (np.isfinite(best) and np.isfinite(second)) or second == 0.0:
        return c + 1, 0.0
    return c + 1, float((second - best) / second)


def brute_first_min_col(beta):
    """the definition, element by element: walk the matrix column by column, keep the first strictly smaller value, stop at
    the first NaN"""
    b = np.asarray(beta)
    best, col = None, 0
    for c in range(b.shape[1]):
        for r in range(b.shape[0]):
            v = b[r, c]
            if v != v:
                return c + 1
            if best is None or v < best:
                best, col = v, c
    return col + 1


# ---------------------------------------------------------------- inputs
def dark_band_image(h, w, row_band, col_band, seed, noise=0.02):
    """background 0.6, one dark (0.05) row band and column band, uniform noise everywhere -- inside the bands too.
    0-based (offset, width) pairs, as band_image of tests/test_frame_path_gpu.py takes them."""
    r = np.random.default_rng(seed)
    img = 0.6 + noise * r.random((h, w), dtype=np.float32)
    r0, rw = row_band
    c0, cw = col_band
    img[np.arange(r0, r0 + rw) % h, :] = 0.05 + noise * r.random((rw, w), dtype=np.float32)
    img[:, np.arange(c0, c0 + cw) % w] = 0.05 + noise * r.random((h, cw), dtype=np.float32)
    return np.asfortranarray(img.astype(np.float32))


def dark_images(h, w):
    """three images per size, the bands at test_vsync_indices_and_stale_sy's offsets (the last one wraps around the right
    edge).  Each band is exactly as wide as the narrowest window vsync tries, 2 * w_min + 1: the window mean is then a
    triangle in the centre with one apex.  (Wider bands are a plateau: every window inside has the same mean up to the
    noise, and the margins of such images measured 4e-6 .. 1e-4 -- replaced, as the module docstring's condition asks.)"""
    import f64_ref
    wmin_y, _, wmin_x, _ = f64_ref.bounds(h, w)
    rw, cw = 2 * wmin_y + 1, 2 * wmin_x + 1
    return [dark_band_image(h, w, (h // 3, rw), (w // 2, cw), 1000 + h),
            dark_band_image(h, w, (h // 5, rw), (w // 7, cw), 2000 + h),
            dark_band_image(h, w, (2 * h // 3, rw), (w - 5, cw), 3000 + h)]


def flat_band_image(h=600, w=800):
    img = np.full((h, w), 0.6, np.float32)
    img[h // 3: h // 3 + max(2, h // 20), :] = 0.05
    img[:, w // 2: w // 2 + max(6, w // 8)] = 0.05
    return np.asfortranarray(img)


GEOM = dict(Fs=2.0e6, x_t=1056, y_t=628, fv=60.0)   # test_vsync_current_sy_option's geometry


def leak(synth, nfr, card, extra=3, n0=0):
    S = synth.samples_per_frame(GEOM["Fs"], GEOM["fv"])
    return S, synth.synth_leak(GEOM["Fs"], GEOM["x_t"], GEOM["y_t"], GEOM["fv"], S * nfr + extra, card=card, n0=n0)


class dark:
    """`with dark(ctx):` -- the option on one context (or group), restored to 0 on the way out"""

    def __init__(self, *holders, value=1):
        self.holders, self.value = holders, value

    def __enter__(self):
        for h in self.holders:
            h.set_option(OPT, self.value)

    def __exit__(self, *exc):
        for h in self.holders:
            h.set_option(OPT, 0)


class precision:
    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        self.ctx.set_precision(self.mode)

    def __exit__(self, *exc):
        self.ctx.set_precision("fast")


def frames(ctx, tsdr, iq, S, alpha=0.0, align=True, sync=None, state=None):
    st = np.zeros((600, 800), np.float32, order="F") if state is None else state
    r = ctx.frames(sync if sync is not None else tsdr.SyncXY(ctx, 600, 800), iq, S, GEOM["y_t"], GEOM["x_t"], np.float32(alpha), st,
                   do_align=align)
    r["state"] = st
    return r


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def numpy_picks(raw_frames):
    """per frame (argmin column of beta_y, argmin column of beta_x, margin_y, margin_x) of the oracle's beta of that image"""
    o = O.SyncXY(600, 800)
    out = []
    for im in raw_frames:
        o.vsync(np.asfortranarray(im))
        (cy, my), (cx, mx) = dark_margin(o.beta("y")), dark_margin(o.beta("x"))
        out.append((cy, cx, my, mx))
    return out


def expected_idx(picks, current_sy):
    """sync_idx rows (s_y, s_x): s_y lags one frame (1 at the start: findmin of the all-zero beta_y) unless current_sy"""
    sy_prev, rows = 1, []
    for cy, cx, _, _ in picks:
        rows.append((cy if current_sy else sy_prev, cx))
        sy_prev = cy
    return np.array(rows, np.int32)


_SHARED = {}


@pytest.fixture
def box_dark(ctx, tsdr, synth):
    """Five "box_dark" frames: the capture, the unaligned EXACT frames (alpha = 0: the 600x800 images themselves), the numpy
    picks over the oracle's beta of those images, and the EXACT frame loop's result under the option.  Computed once."""
    if "box" not in _SHARED:
        S, iq = leak(synth, 5, "box_dark")
        with precision(ctx, "exact"):
            raw = frames(ctx, tsdr, iq, S, align=False)
            with dark(ctx):
                exact = frames(ctx, tsdr, iq, S)
        _SHARED["box"] = dict(S=S, iq=iq, raw=raw, picks=numpy_picks(raw["frames"]), exact=exact)
    return _SHARED["box"]


# ================================================================ host tests (no GPU)
def test_numpy_first_minimum_helper_against_a_brute_force_scan():
    r = np.random.default_rng(7)
    for k in range(40):
        W, n = int(r.integers(1, 7)), int(r.integers(2, 12))
        b = r.integers(0, 4, (W, n)).astype(np.float32)          # few distinct values: ties everywhere
        if k % 3 == 1:
            b.ravel()[r.integers(0, b.size, 2)] = np.nan          # one or two NaN
        if k % 5 == 2:
            b[:] = b[0, 0]                                        # all equal
        b = np.asfortranarray(b)
        assert argmin_col(b) == brute_first_min_col(b), (k, b)
        assert dark_margin(b)[0] == brute_first_min_col(b)
    b = np.asfortranarray(np.array([[3, 1, 1], [2, 1, np.nan]], np.float32))
    assert argmin_col(b) == 3 and argmin_col(b[:, :2]) == 2
    assert dark_margin(np.asfortranarray(np.array([[4.0, 1.0, 2.0]])))[1] == 0.5
    assert dark_margin(np.zeros((3, 4)))[1] == 0.0 and argmin_col(np.zeros((3, 4))) == 1


@pytest.mark.parametrize("x_t,y_t", [(1056, 628), (300, 130)])
def test_dark_profiles_mirror_the_blanking_of_the_bright_ones(synth, x_t, y_t):
    aw, ah = int(round(x_t * 0.78)), int(round(y_t * 0.955))
    for base in ("box", "plateau"):
        a, d = synth.test_card(x_t, y_t, blank=base), synth.test_card(x_t, y_t, blank=base + "_dark")
        assert d.dtype == np.float32 and d.shape == a.shape
        assert np.array_equal(d[:ah, :aw], a[:ah, :aw])                                 # the card
        blank = np.ones(a.shape, bool)
        blank[:ah, :aw] = False
        assert np.array_equal(d[blank], np.float32(1.0) - a[blank])                     # every blanking level mirrored
        assert d[blank].min() == 0.0
        r = synth.test_card(x_t, y_t, row0=17, col0=29, blank=base + "_dark")
        assert np.array_equal(r, np.roll(d, (17, 29), axis=(0, 1)))
    with pytest.raises(ValueError):
        synth.test_card(x_t, y_t, blank="stripes_dark")
    n = 5000
    assert np.array_equal(synth.synth_leak(2.0e6, x_t, y_t, 60.0, n, card="box_dark"),
                          synth.synth_leak(2.0e6, x_t, y_t, 60.0, n, row0=int(round(400 / 1125 * y_t)), col0=int(round(1101 / 2576 * x_t)),
                                           card=synth.test_card(x_t, y_t, row0=int(round(400 / 1125 * y_t)), col0=int(round(1101 / 2576 * x_t)),
                                                                blank="box_dark")))


# sha256 of the existing profiles' output, computed on the commit before the dark profiles were added
PARENT_HASHES = {
    "card box 1056x628": "b48fa52ec89326b17516d4247fb588335bb9c45a246c6765fe2f3faae22cecb0",
    "card plateau 1056x628": "fc7c9b1f0aecf625dd607aa5a151b871a9cc419252a7bde8a6d227c54a9c1a0e",
    "card box 2576x1125 rolled": "de311cf819859763bfaac5e78d19411d6a01b3ca4be03f3313e870a65361cf39",
    "leak box": "27fb826f5f864f526bb3acdf17892ed53714e8e0ef2d5b9bf2d1229fbf7fc800",
    "leak plateau": "4eb69db30cc23d93024de66626e2e832ad006c6b9cf58a733185c9defa88f2f0",
    "leak default card": "f8e4e4229982280988fe47f4c84c01ff2bb2ab6fa44bd64276cf4a9a1a8b182d",
}


def existing_profile_hashes(synth):
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    return {
        "card box 1056x628": h(synth.test_card(1056, 628, blank="box")),
        "card plateau 1056x628": h(synth.test_card(1056, 628, blank="plateau")),
        "card box 2576x1125 rolled": h(synth.test_card(2576, 1125, row0=400, col0=1101)),
        "leak box": h(synth.synth_leak(2.0e6, 1056, 628, 60.0, 40000, card="box")),
        "leak plateau": h(synth.synth_leak(2.0e6, 1056, 628, 60.0, 40000, n0=12345, card="plateau")),
        "leak default card": h(synth.synth_leak(20e6, 2576, 1125, 60.0, 40000, card=None)),
    }


def test_existing_profiles_keep_their_bits(synth):
    assert existing_profile_hashes(synth) == PARENT_HASHES


def test_julia_shim_carries_the_binding():
    """static, in the style of tests/test_julia_shim_static.py (no Julia here): arg_area_blank! is exported, accepts only
    findmin / findmax and sets the option through hip_set_option, whose ccall that test already holds to the header"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "tempestsdr.jl_amd", "julia", "TempestHIP.jl")).read()
    assert re.search(r"^export .*\barg_area_blank!", src, flags=re.M)
    body = src[src.index("function arg_area_blank!("):]
    body = body[:body.index("\nend\n")]
    assert "f === findmin || f === findmax || throw(ArgumentError" in body
    assert 'hip_set_option("vsync_blank_dark", f === findmin ? 1 : 0)' in body
    assert '\\"vsync_blank_dark\\"' in src[:src.index("function hip_set_option(name")]       # the set_option docstring
    hdr = open(os.path.join(root, "include", "tempest_hip.h")).read()
    assert '"vsync_blank_dark"' in hdr and "tsdr_sync_reset restores reference-equal behaviour" in hdr


# ================================================================ GPU tests
# ---- 1. standalone vsync, EXACT
@pytest.mark.gpu
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("h,w", [(600, 800), (120, 200), (77, 131)])
def test_vsync_dark_indices_and_stale_sy(ctx, tsdr, h, w, waves):
    imgs = dark_images(h, w)
    g, o = tsdr.SyncXY(ctx, h, w), O.SyncXY(h, w)
    ctx.set_option("beta_waves", waves)
    try:
        with dark(ctx):
            sy_pending = 1                                   # findmin of the all-zero beta_y: index (1,1)
            for k, im in enumerate(imgs + [None] + imgs[1:2]):
                if im is None:
                    g.reset(); o.reset()
                    sy_pending = 1
                    continue
                got = g.vsync(im)
                o.vsync(im)
                bx, by = o.beta("x"), o.beta("y")
                assert same_bits(g.beta("x"), bx) and same_bits(g.beta("y"), by), f"beta after call {k}"
                assert got == (sy_pending, argmin_col(bx)), f"call {k}: {got}, numpy ({sy_pending}, {argmin_col(bx)})"
                sy_pending = argmin_col(by)
                if (h, w) == (77, 131):
                    assert sy_pending == 2                   # the FIR's start-up transient, not the drawn band (docstring)
    finally:
        ctx.set_option("beta_waves", 4)
        g.close()


# ---- 2. ties and degenerates
@pytest.mark.gpu
def test_vsync_dark_ties_and_degenerates(ctx, tsdr):
    nan_px, inf_px = flat_band_image(), flat_band_image()
    nan_px[301, 77] = np.nan
    inf_px[17, 640] = np.inf
    cases = {"flat bands": flat_band_image(), "zeros": np.zeros((600, 800), np.float32), "ones": np.ones((600, 800), np.float32),
             "one NaN": nan_px, "one +Inf": inf_px}
    g, o = tsdr.SyncXY(ctx, 600, 800), O.SyncXY(600, 800)
    try:
        with dark(ctx):
            for name, im in cases.items():
                im = np.asfortranarray(im)
                g.reset(); o.reset()
                sy_pending = 1
                for k in range(2):                           # the second call returns the first one's s_y
                    got = g.vsync(im)
                    o.vsync(im)
                    bx, by = o.beta("x"), o.beta("y")
                    for gb, ob in ((g.beta("x"), bx), (g.beta("y"), by)):     # bit for bit, NaN where the oracle has NaN
                        assert np.array_equal(np.isnan(gb), np.isnan(ob)) and same_bits(gb[~np.isnan(ob)], ob[~np.isnan(ob)]), name
                    assert got == (sy_pending, argmin_col(bx)), (name, k, got, (sy_pending, argmin_col(bx)))
                    sy_pending = argmin_col(by)
                if name == "flat bands":
                    # an exact tie on both axes, several columns at the minimum: the FIRST one is the answer
                    for b, first in ((bx, 445), (by, 217)):
                        colmin = b.min(axis=0)
                        assert dark_margin(b) == (first, 0.0) and np.count_nonzero(colmin == colmin.min()) >= 2
                    assert got == (217, 445)
    finally:
        g.close()


# ---- 3. f64
@pytest.mark.gpu
def test_vsync_dark_f64(ctx, tsdr):
    import f64_ref as R
    h, w = 120, 200
    s, r = tsdr.api.SyncXY(ctx, h, w, dtype=np.float64), R.SyncXY64(h, w)
    try:
        with dark(ctx):
            sy_pending = 1
            for k, im in enumerate(dark_images(h, w)):
                im64 = np.asfortranarray(im, np.float64)
                got = s.vsync(im64)
                r.vsync(im64)
                assert np.array_equal(s.beta("x"), r.beta_x) and np.array_equal(s.beta("y"), r.beta_y), k
                assert got == (sy_pending, argmin_col(r.beta_x)), (k, got)
                assert dark_margin(r.beta_x)[1] >= 1e-3 and dark_margin(r.beta_y)[1] >= 1e-3
                sy_pending = argmin_col(r.beta_y)
            s.reset()
            assert s.vsync(im64) == (1, argmin_col(r.beta_x))
    finally:
        s.close()


# ---- 4. frame loop, EXACT
@pytest.mark.gpu
@pytest.mark.parametrize("current_sy", [0, 1])
def test_frames_dark_exact(ctx, tsdr, box_dark, current_sy):
    d = box_dark
    for cy, cx, my, mx in d["picks"]:
        assert my >= 1e-3 and mx >= 1e-3, d["picks"]          # the condition on inputs compared against numpy
    if current_sy:
        ctx.set_option("vsync_current_sy", 1)
        try:
            with precision(ctx, "exact"), dark(ctx):
                got = frames(ctx, tsdr, d["iq"], d["S"])
        finally:
            ctx.set_option("vsync_current_sy", 0)
    else:
        got = d["exact"]
    want = expected_idx(d["picks"], current_sy)
    assert np.array_equal(got["sync_idx"], want), (got["sync_idx"].tolist(), want.tolist())
    for f, img in enumerate(d["raw"]["frames"]):
        sy, sx = (int(v) for v in want[f])
        assert same_bits(got["frames"][f], np.roll(img, (-sy, -sx), axis=(0, 1))), f   # circshift(image, (-s_y, -s_x)), alpha = 0


# ---- 5. FAST equals EXACT
def _relerr(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), 1e-30)))


@pytest.mark.gpu
@pytest.mark.parametrize("card", ["box_dark", "plateau_dark"])
def test_frames_dark_fast_equals_exact(ctx, tsdr, synth, box_dark, card):
    nfr = 5
    if card == "box_dark":
        S, iq, exact, picks = box_dark["S"], box_dark["iq"], box_dark["exact"], box_dark["picks"]
    else:
        S, iq = leak(synth, nfr, card)
        with precision(ctx, "exact"):
            raw = frames(ctx, tsdr, iq, S, align=False)
            with dark(ctx):
                exact = frames(ctx, tsdr, iq, S)
        picks = numpy_picks(raw["frames"])     # (for the margins only: this card's indices are EXACT's, not numpy's)
    # frames whose decision the oracle's own beta leaves closer than half the guard's 2e-5: FAST's 1e-7-level beta error
    # cannot lift them over it, so the guard must re-evaluate at least these
    close = sum(1 for _, _, my, mx in picks if min(my, mx) < 1e-5)
    assert close >= 1 if card == "plateau_dark" else close == 0, picks
    with dark(ctx):
        ctx.sync_guard_stats(reset=True)
        fast = frames(ctx, tsdr, iq, S)
        checked, reeval = ctx.sync_guard_stats()
        margins = np.asarray(ctx.sync_guard_margins())
        assert np.array_equal(fast["sync_idx"], exact["sync_idx"]), (fast["sync_idx"].tolist(), exact["sync_idx"].tolist())
        assert checked == nfr and close <= reeval <= nfr, (checked, reeval, close)
        for f in range(nfr):
            assert _relerr(fast["frames"][f], exact["frames"][f]) < RTOL, f
        assert margins.size == 2 * nfr and np.all((margins >= 0.0) & (margins <= 1.0)), margins
        # every frame flagged: the whole buffer is the exact sequence
        ctx.set_option("sync_guard_ppb", 100000000)
        try:
            ctx.sync_guard_stats(reset=True)
            allf = frames(ctx, tsdr, iq, S)
            checked, reeval = ctx.sync_guard_stats()
        finally:
            ctx.set_option("sync_guard_ppb", 20000)
        assert checked == reeval == nfr, (checked, reeval)
        assert np.array_equal(allf["sync_idx"], exact["sync_idx"])


# ---- 6. routes
def _device_run(ctx, tsdr, bufs, S, how, fmt=None, scale=None):
    """the buffers through tsdr_frames_d ("d"), tsdr_frames_submit_d + flush ("submit"), tsdr_frames_scan_d + combine ("split")
    or tsdr_frames_iq_d on raw integer samples ("iq"): (frames, sync_idx per buffer, final state) as bit patterns"""
    api = importlib.import_module("tempestsdr_jl_amd.api")
    y_t, x_t = GEOM["y_t"], GEOM["x_t"]
    sync = tsdr.SyncXY(ctx, 600, 800)
    cnt = [(b.size // 2 if how == "iq" else b.size) // S for b in bufs]
    d_state = ctx.upload(np.zeros(NPX, np.float32))
    d_iq = [ctx.upload(b if how == "iq" else b.view(np.float32)) for b in bufs]
    d_fr = [ctx.dev_alloc(c * NPX * 4) for c in cnt]
    d_ix = [ctx.dev_alloc(c * 8) for c in cnt]
    extra = []
    try:
        for b, c in enumerate(cnt):
            nEch = c * S + 1
            if how == "split":
                d_img, d_keys = ctx.dev_alloc(c * NPX * 4), ctx.dev_alloc(c * 16)
                extra += [d_img, d_keys]
                n = C.c_int(0)
                ctx.call("tsdr_frames_scan_d", C.c_void_p(sync.h), C.c_void_p(d_iq[b]), nEch, S, y_t, x_t, 1, C.c_void_p(d_img),
                         C.c_void_p(0), C.c_void_p(d_keys), C.byref(n))
                assert n.value == c
                ctx.call("tsdr_frames_combine_d", C.c_void_p(sync.h), C.c_void_p(d_img), C.c_void_p(d_keys), c, C.c_float(0.1), 1,
                         C.c_void_p(d_state), C.c_void_p(d_fr[b]), C.c_void_p(d_ix[b]))
            elif how == "iq":
                assert api.frames_iq_d(ctx, sync, d_iq[b], fmt, scale, nEch, S, y_t, x_t, np.float32(0.1), True, d_state, d_fr[b], None,
                                       d_ix[b]) == c
            else:
                f = api.frames_submit_d if how == "submit" else api.frames_d
                assert f(ctx, sync, d_iq[b], nEch, S, y_t, x_t, np.float32(0.1), True, d_state, d_fr[b], None, d_ix[b]) == c
        if how == "submit":
            api.frames_flush(ctx)
        ctx.synchronize()
        return ([ctx.download(p, (c * NPX,), np.uint32) for p, c in zip(d_fr, cnt)],
                [ctx.download(p, (c, 2), np.int32) for p, c in zip(d_ix, cnt)], ctx.download(d_state, (NPX,), np.uint32))
    finally:
        sync.close()
        for p in [d_state] + d_iq + d_fr + d_ix + extra:
            ctx.dev_free(p)


def _assert_runs_equal(a, b, what):
    for k, (x, y) in enumerate(zip(a[0] + a[1], b[0] + b[1])):
        assert np.array_equal(x, y), (what, k)
    assert np.array_equal(a[2], b[2]), what


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_dark_routes_equal_one_call_per_buffer(ctx, tsdr, synth, box_dark, mode):
    import iq8_ref as R
    S = box_dark["S"]
    per = 2 * S + 1
    bufs = [synth.synth_leak(GEOM["Fs"], GEOM["x_t"], GEOM["y_t"], GEOM["fv"], per, card="box_dark", n0=b * per) for b in range(3)]
    ctx.set_option("sync_guard_auto", 0)
    try:
        with precision(ctx, mode), dark(ctx):
            ref = _device_run(ctx, tsdr, bufs, S, "d")
            # the first buffer is the fixture's capture: its indices are the numpy picks (margins >= 1e-3, case 4)
            assert np.array_equal(ref[1][0], expected_idx(box_dark["picks"], 0)[:2])
            assert not np.array_equal(ref[1][0][:, 1], ref[1][0][:, 0]) and np.any(ref[0][0])
            _assert_runs_equal(ref, _device_run(ctx, tsdr, bufs, S, "submit"), "submit")
            _assert_runs_equal(ref, _device_run(ctx, tsdr, bufs, S, "split"), "scan + combine")
            # one sc8 buffer against its expanded ComplexF32 twin
            q, scale = R.quantise(bufs[0], "sc8")
            twin = R.expand(q, "sc8", scale)
            _assert_runs_equal(_device_run(ctx, tsdr, [twin], S, "d"), _device_run(ctx, tsdr, [q], S, "iq", "sc8", scale), "sc8")
    finally:
        ctx.set_option("sync_guard_auto", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_dark_group_of_one_equals_single_context(ctx, tsdr, box_dark, mode):
    S, iq = box_dark["S"], box_dark["iq"]
    g = tsdr.Group([0])
    try:
        g.set_precision(mode)
        with precision(ctx, mode), dark(ctx, g):
            a = frames(ctx, tsdr, iq, S, alpha=0.1)
            s2 = np.zeros((600, 800), np.float32, order="F")
            b = g.frames(iq, S, GEOM["y_t"], GEOM["x_t"], np.float32(0.1), s2)
        assert np.array_equal(a["sync_idx"], expected_idx(box_dark["picks"], 0))
        assert np.array_equal(a["sync_idx"], b["sync_idx"]) and same_bits(a["state"], s2)
        for fa, fb in zip(a["frames"], b["frames"]):
            assert same_bits(fa, fb)
        with pytest.raises(AssertionError):
            g.set_option("vsync_blank_darker", 1)
    finally:
        g.close()


# ---- 7. default untouched
@pytest.mark.gpu
def test_default_polarity_is_untouched_and_the_option_waits_for_submitted_buffers(ctx, tsdr, synth):
    api = importlib.import_module("tempestsdr_jl_amd.api")
    S, iq = leak(synth, 4, "box")                       # a WHITE blanking band
    img = np.asfortranarray(frames(ctx, tsdr, iq, S, align=False)["frames"][0])

    def run():
        sg = tsdr.SyncXY(ctx, 600, 800)
        try:
            r = frames(ctx, tsdr, iq, S, alpha=0.1)
            return r, [sg.vsync(img), sg.vsync(img)], (sg.beta("x"), sg.beta("y"))
        finally:
            sg.close()

    off0 = run()
    with dark(ctx):
        on = run()
    off1 = run()
    assert np.array_equal(off0[0]["sync_idx"], off1[0]["sync_idx"]) and off0[1] == off1[1]
    assert same_bits(off0[0]["state"], off1[0]["state"])
    for a, b in zip(off0[0]["frames"], off1[0]["frames"]):
        assert same_bits(a, b)
    # beta does not depend on the polarity; the indices do
    assert same_bits(off0[2][0], on[2][0]) and same_bits(off0[2][1], on[2][1])
    assert np.all(on[0]["sync_idx"][:, 1] != off0[0]["sync_idx"][:, 1]) and np.all(on[0]["sync_idx"][1:, 0] != off0[0]["sync_idx"][1:, 0])
    assert on[1][0][1] != off0[1][0][1] and on[1][1][0] != off0[1][1][0]
    # the option between two submissions: the first buffer keeps the polarity it was submitted with
    y_t, x_t = GEOM["y_t"], GEOM["x_t"]
    d_iq = ctx.upload(iq.view(np.float32))
    d_fr, d_ix = [ctx.dev_alloc(4 * NPX * 4) for _ in range(2)], [ctx.dev_alloc(4 * 8) for _ in range(2)]
    res = {}
    try:
        for name in ("bright then dark", "bright, bright", "dark, dark"):
            sync = tsdr.SyncXY(ctx, 600, 800)
            d_state = ctx.upload(np.zeros(NPX, np.float32))
            try:
                ctx.set_option(OPT, int(name.startswith("dark")))
                api.frames_submit_d(ctx, sync, d_iq, iq.size, S, y_t, x_t, np.float32(0.1), True, d_state, d_fr[0], None, d_ix[0])
                ctx.set_option(OPT, int(name.endswith("dark")))
                api.frames_submit_d(ctx, sync, d_iq, iq.size, S, y_t, x_t, np.float32(0.1), True, d_state, d_fr[1], None, d_ix[1])
                api.frames_flush(ctx)
                ctx.synchronize()
                res[name] = [ctx.download(p, (4, 2), np.int32) for p in d_ix] + [ctx.download(d_fr[0], (4 * NPX,), np.uint32)]
            finally:
                ctx.set_option(OPT, 0)
                sync.close()
                ctx.dev_free(d_state)
    finally:
        for p in [d_iq] + d_fr + d_ix:
            ctx.dev_free(p)
    mixed, bright, dk = res["bright then dark"], res["bright, bright"], res["dark, dark"]
    assert np.array_equal(mixed[0], bright[0]) and np.array_equal(mixed[2], bright[2])      # buffer 1: the old polarity
    assert np.array_equal(mixed[1][:, 1], dk[1][:, 1])                                      # buffer 2: s_x of the new one
    assert np.array_equal(mixed[1][1:, 0], dk[1][1:, 0])                                    # and its s_y from frame 2 on;
    assert mixed[1][0, 0] == bright[1][0, 0]                                                # the pending s_y is the old polarity's
