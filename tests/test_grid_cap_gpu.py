"""Every capped-grid launch of the library past its grid cap, against the reference and the bar its entry point already has.

One test per case of grid_cap_cases.py.  A case sizes itself from the device's CU count so that the launch sites it is listed for
get more work than a full grid covers (cap < work items <= 3 * cap, ragged: workgroup 0's tail exists and some threads take one
trip more than others), makes the call through the device-pointer entry point inside guarded arenas (dptr_util.py) with the
per-kernel profile on, and then
  * asserts that every kernel it names ran and that nothing outside the documented output was written;
  * compares the WHOLE output with the reference at the bar of the test named beside the runner -- no bar is introduced here;
  * on a mismatch names the first bad index and the trip of the grid-stride loop it belongs to (or workgroup 0's tail).
Each test prints, per launch site, the work items against the cap and the profile names seen (pytest -s / -rA shows them).
"""
import ctypes as C

import numpy as np
import pytest

import f64_ref as R64
import f64_spec_ref as S64
import grid_cap_cases as G
import iq8_ref as Q
import oracle_lib as O
from dptr_util import Arenas
from test_dptr_gpu import VALS32, VALS32_FM, _extremes_in_noise, _search_signal, _ulps, profiled
from test_fast_mode_gpu import RTOL                                 # 6e-7: the FAST frame loop against the oracle
from test_fft_path_gpu import CORR_TOL, FFT_TOL                     # 2e-5 / 5e-6, relative to the largest magnitude

pytestmark = pytest.mark.gpu

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
RUNNERS = {}       # case -> (runner(env, p), the profile names the case must leave behind)


def runner(cases, names):
    def deco(fn):
        for c in ([cases] if isinstance(cases, str) else cases):
            assert c not in RUNNERS, c
            RUNNERS[c] = (fn, tuple(names(c)) if callable(names) else tuple(names))
        return fn
    return deco


class Env:
    """what a runner gets: the context, the package, the case's name and where a bad index lies"""

    def __init__(self, ctx, tsdr, synth, case, cu):
        self.ctx, self.tsdr, self.synth, self.case, self.cu = ctx, tsdr, synth, case, cu
        self.cap = G.cap(cu)
        self.api = tsdr.api
        self.seen = {}

    def rng(self, *key):
        return np.random.default_rng([20261, sum(map(ord, self.case)), *[int(k) for k in key]])

    def where(self, idx, vec=1, tail_from=None, cap=None):
        """the trip of the grid-stride loop (1-based) that handles element idx of a kernel moving `vec` elements per work item"""
        if tail_from is not None and idx >= tail_from:
            return f"index {idx}: workgroup 0's tail (the {idx - tail_from + 1}. element behind the vector body)"
        return f"index {idx}: trip {idx // ((cap or self.cap) * vec) + 1} of the grid-stride loop ({(cap or self.cap) * vec} elements per trip)"

    def bits(self, got, want, what, vec=1, tail_from=None):
        got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
        assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
        u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
        bad = got.view(u) != want.view(u)
        if got.dtype.kind == "f":
            bad &= ~(np.isnan(got) & np.isnan(want))
        if bad.any():
            i = int(np.argmax(bad))
            raise AssertionError(f"{self.case}: {what}: {int(bad.sum())} of {bad.size} differ; first at {self.where(i, vec, tail_from)}: got {got[i]!r}, want {want[i]!r}")

    def within(self, err, bar, what, vec=1, tail_from=None, cap=None):
        """err: non-negative error per element (NaN counts as a miss); bar: scalar"""
        err = np.asarray(err).ravel()
        worst = float(np.nanmax(err)) if err.size else 0.0
        print(f"    {self.case}: {what}: {worst:.3e} (bar {bar:.3e})")
        bad = ~(err < bar)
        if bad.any():
            i = int(np.argmax(bad))
            raise AssertionError(f"{self.case}: {what}: {int(bad.sum())} of {bad.size} miss the bar {bar:g} (worst {worst:.3e}); first at {self.where(i, vec, tail_from, cap)}: {err[i]!r}")


@pytest.mark.parametrize("case", sorted(G.CASES))
def test_past_the_grid_cap(ctx, tsdr, synth, case):
    cu = ctx.device_info()["cu_count"]
    p = G.params(case, cu)
    fn, names = RUNNERS[case]
    sites = G.sites_of(case)
    env = Env(ctx, tsdr, synth, case, cu)
    # what the inventory says about this case holds on THIS device
    for site, work in sites:
        c, w = G.cap_of(site, cu), work(p)
        assert c < w <= 3 * c, (case, site.token, w, c)
        assert not site.names or set(site.names) & set(names), (case, site.names, names)
    assert set(names) <= {n for s, _ in sites for n in s.names} | {n for n, (_, cs) in G.ROW_STEPS.items() if case in cs}, (case, names)
    fn(env, p)
    for site, work in sites:
        c, w = G.cap_of(site, cu), work(p)
        seen = {n: env.seen.get(n, 0) for n in site.names if n in names}
        print(f"  {case}: {site.file} {site.token} [{site.expr}]: {w} work items / cap {c} = {w / c:.3f} (trips {w // c + (w % c > 0)}); launches {seen or '(no profile name)'}")
    if "grid" in p:
        print(f"  {case}: {p['ntiles']} tiles of {p['T']} rows on {p['grid']} workgroups; launches { {n: env.seen.get(n, 0) for n in names} }")
    for n in names:
        assert env.seen.get(n, 0) > 0, (case, n, env.seen)


class traced(profiled):
    """profiled, adding what ran to the environment's record on the way out"""

    def __init__(self, env, ctx=None):
        super().__init__(ctx or env.ctx)
        self.env = env

    def __exit__(self, *exc):
        if exc[0] is None:
            for k, v in self.names().items():
                self.env.seen[k] = self.env.seen.get(k, 0) + v
        return super().__exit__(*exc)


def _crandn(rng, n, dtype=C64, scale=1.0):
    out = np.empty(n, dtype)
    ft = F32 if dtype == C64 else F64
    out.real = rng.standard_normal(n, dtype=ft) * ft(scale)
    out.imag = rng.standard_normal(n, dtype=ft) * ft(scale)
    return out


def _quantised(rng, n, fmt, amp=None, clip=0.2, peak_at=None):
    """integer IQ of n samples: noise (times amp, an array or None) clipped to +-clip of full scale in either component; peak_at:
    that sample alone at full scale.  -> (components, scale, the samples as every loader expands them)"""
    z = _crandn(rng, n, C64, 0.07)
    if amp is not None:
        z *= amp.astype(F32)
    z.real = np.clip(z.real, -clip, clip)
    z.imag = np.clip(z.imag, -clip, clip)
    ref = np.concatenate([z, np.array([1.0 + 1.0j], C64)])      # fixes the scale: full scale = 1.0
    q, scale = Q.quantise(ref, fmt)
    q = q[: 2 * n].copy()
    if peak_at is not None:
        q[2 * peak_at: 2 * peak_at + 2] = Q.quantise(np.array([1.0 + 1.0j], C64), fmt)[0]
    return q, float(scale), Q.expand(q, fmt, scale)


def _raw(q, k, fill=55):
    """the integer buffer with k samples in front (the caller passes base + k samples) and padded to whole words"""
    buf = np.concatenate([np.full(2 * k, fill, q.dtype), q])
    pad = (-buf.nbytes) % 4
    return np.concatenate([buf, np.full(pad // buf.itemsize, fill, q.dtype)]) if pad else buf


# ============================================================================================================ demodulators
# bars: test_dptr_gpu.py:test_demod_f32_bitexact_at_every_phase (bit identity with the oracle), test_iq_demod_gpu.py (the integer forms have
# the bits of the ComplexF32 form on the expanded samples: here against the oracle on the host expansion, which says the same)
D32 = {"am": ("tsdr_am_demod_d", O.amDemod, ("am_demod", "am_demod1")), "abs2": ("tsdr_abs2_d", O.abs2, ("abs2", "abs2_1")),
       "invert": ("tsdr_invert_am_d", O.invert_amDemod, ("invert_am_abs", "invert_am_abs1"))}
IQ_KIND = {"am": "am", "abs2": "abs2", "invert": "invert_am"}


def _peaks(n, spv, cap):
    """(label, index) of the single largest sample: in the first trip, in the last trip of the vector body, in workgroup 0's tail
    (the one-sample-per-lane kernels have no tail: their last sample)"""
    body = n // spv * spv
    out = [("first trip", 5), ("last trip", body - 2)]
    assert body - 2 >= (G.cdiv(body, spv * cap) - 1) * spv * cap
    out.append(("workgroup 0's tail", n - 1) if spv > 1 else ("last sample", n - 1))
    assert spv == 1 or n - 1 >= body
    return out


def _demod_names(case):
    kind, fmt, route = case.split("-")
    if fmt == "cf32":
        k = D32[kind][2][route == "one"]
        return (k,) + (("invert_am_scale",) if kind == "invert" and route == "one" else ())
    k = ("demod_iq_" if route == "vec" else "demod1_iq_") + fmt
    return (k,) + (("invert_am_scale",) if kind == "invert" and route == "one" else ())


@runner([f"{k}-{f}-{r}" for k in D32 for f in ("cf32",) + G.FMTS for r in ("vec", "one")], _demod_names)
def run_demod(env, p):
    kind, fmt, route = env.case.split("-")
    n, spv = p["n"], p["spv"]
    body = n // spv * spv if spv > 1 else None
    ref = D32[kind][1]
    runs = _peaks(n, spv, env.cap) if kind == "invert" else [("random + extremes", None)]
    for label, peak in runs:
        rng = env.rng(peak or 0)
        if fmt == "cf32":
            if kind == "invert":      # finite data; the maximum unique by a factor of 4 and more (|noise| <= 0.29, |peak| = 2.8)
                z = _crandn(rng, n, C64, 0.07)
                z.real, z.imag = np.clip(z.real, -0.2, 0.2), np.clip(z.imag, -0.2, 0.2)
                z[peak] = 2.0 + 2.0j
            else:
                z = _extremes_in_noise(n, VALS32, C64, 1)
            data, k, want = z, 0, ref(z)
        else:
            q, scale, z = _quantised(rng, n, fmt, peak_at=peak)      # |noise| <= 0.29 of full scale, |peak| = 1.41
            k = 0 if route == "vec" else 1
            data, want = _raw(q, k), ref(z)
        if kind == "invert":
            a = np.abs(z.astype(C128))
            assert int(np.argmax(a)) == peak and a[peak] >= 4 * np.partition(a, -2)[-2], label
        with Arenas(env.ctx) as A, traced(env):
            # vector kernels: both pointers 16-byte aligned; the others: IQ at an odd sample, the output at an odd float
            i = A.input("iq", data, 0 if (route == "vec" or fmt != "cf32") else 8)
            o = A.output("out", 4 * n, 0 if route == "vec" else 4)
            if fmt == "cf32":
                env.ctx.call(D32[kind][0], i.ptr, n, o.ptr)
            else:
                env.api.demod_iq_d(IQ_KIND[kind], env.ctx, i.addr + k * Q.BYTES[fmt], fmt, scale, n, o.addr)
            A.check()
            got = o.get(F32)
        env.bits(got, want, f"{kind} of {fmt} ({label})", spv, body)
        if kind == "invert":
            assert got[peak] == 0.0 and np.count_nonzero(got == 0.0) == 1, label      # 1 - max / max, there alone


@runner(["am-f64", "abs2-f64", "invert-f64"], lambda c: {"am-f64": ("am_demod_f64",), "abs2-f64": ("abs2_f64",),
                                                         "invert-f64": ("invert_am_f64_abs", "invert_am_f64_scale")}[c])
def run_demod64(env, p):
    """test_dptr_gpu.py:test_demod_f64_at_every_phase / test_f64_gpu.py: am within 1 ulp of hypot, abs2 bit-exact against re*re + im*im,
    invert bit-exact against 1 - a / max(a) of the device's own a"""
    kind, n = env.case.split("-")[0], p["n"]
    runs = _peaks(n, 1, env.cap) if kind == "invert" else [("random", None)]
    for label, peak in runs:
        z = _crandn(env.rng(peak or 0), n, C128)
        if peak is not None:
            z[peak] = 40.0 + 40.0j       # |noise| stays below 8 at these sizes (eight standard deviations)
        with Arenas(env.ctx) as A, traced(env):
            i, o = A.input("iq", z, 16), A.output("out", 8 * n, 8)
            a = A.output("am", 8 * n, 0) if kind == "invert" else None
            env.ctx.call({"am": "tsdr_am_demod_f64_d", "abs2": "tsdr_abs2_f64_d", "invert": "tsdr_invert_am_f64_d"}[kind], i.ptr, n, o.ptr)
            if a:
                env.ctx.call("tsdr_am_demod_f64_d", i.ptr, n, a.ptr)
            A.check()
            got = o.get(F64)
        if kind == "am":
            want = np.hypot(z.real, z.imag)
            d = np.abs(got.view(np.int64) - want.view(np.int64))
            env.within(d.astype(F64), 1.5, "am_demod_f64, ulps from hypot")
        elif kind == "abs2":
            env.bits(got, R64.abs2(z), "abs2_f64")
        else:
            am = a.get(F64)
            assert _ulps(am, np.hypot(z.real, z.imag)) <= 1 and int(np.argmax(am)) == peak and am[peak] >= 4 * np.partition(am, -2)[-2]
            env.bits(got, 1.0 - am / am.max(), f"invert_am_f64 ({label})")
            assert got[peak] == 0.0 and np.count_nonzero(got == 0.0) == 1, label


@runner(["fm-cf32"] + [f"fm-{f}" for f in G.FMTS], lambda c: ("fm_demod",) if c == "fm-cf32" else ("fm_demod_iq_" + c[3:],))
def run_fm(env, p):
    """1e-6 on the angle against the oracle (test_fm_demod_close); the integer forms also bit for bit what the ComplexF32 form
    returns for the expanded samples (test_iq_demod_gpu.py)"""
    fmt, n = env.case[3:], p["n"]
    if fmt == "cf32":
        z = _extremes_in_noise(n, VALS32_FM, C64, 3)
        data, k = z, 0
    else:
        q, scale, z = _quantised(env.rng(), n, fmt)
        data, k = _raw(q, 1), 1
    want = O.fmDemod(z)
    with Arenas(env.ctx) as A, traced(env):
        i, o = A.input("iq", data, 8 if fmt == "cf32" else 0), A.output("out", 4 * n, 12)
        if fmt == "cf32":
            env.ctx.call("tsdr_fm_demod_d", i.ptr, n, o.ptr)
        else:
            env.api.demod_iq_d("fm", env.ctx, i.addr + k * Q.BYTES[fmt], fmt, scale, n, o.addr)
            e, t = A.input("expanded", z, 0), A.output("twin", 4 * n, 0)
            env.ctx.call("tsdr_fm_demod_d", e.ptr, n, t.ptr)
        A.check()
        got = o.get(F32)
        twin = t.get(F32) if fmt != "cf32" else None
    assert got[0] == 0.0
    env.within(np.abs(got.astype(F64) - want), 1e-6, "fmDemod against the oracle")
    if twin is not None:
        env.bits(got, twin, "fm_demod_iq against fm_demod of the expanded samples")


@runner("fm-f64", ("fm_demod_f64",))
def run_fm64(env, p):
    """within 2 ulp of atan2 of the unfused product (test_f64_gpu.py, test_demod_f64_at_every_phase)"""
    n = p["n"]
    z = _crandn(env.rng(), n, C128)
    re, im = R64.fm_product(z)
    with Arenas(env.ctx) as A, traced(env):
        i, o = A.input("iq", z, 16), A.output("out", 8 * n, 8)
        env.ctx.call("tsdr_fm_demod_f64_d", i.ptr, n, o.ptr)
        A.check()
        got = o.get(F64)
    assert got[0] == 0.0
    want = np.arctan2(im, re)
    ia, ib = got[1:].view(np.int64), want.view(np.int64)
    d = np.where((ia < 0) == (ib < 0), np.abs(ia - ib), np.int64(1) << 62)
    env.within(np.concatenate([[0.0], d.astype(F64)]), 2.5, "fm_demod_f64, ulps from atan2")


@runner(["expand-sc16"] + [f"expand-{f}-{r}" for f in ("sc8", "uc8") for r in ("pair", "one")],
        lambda c: ("iq_expand_" + c.split("-")[1] + ("_1" if c.endswith("-one") else ""),))
def run_expand(env, p):
    """tsdr_iq_expand_d: the bits of the host expansion (test_iq_demod_gpu.py:test_expand_equals_host_expansion)"""
    parts = env.case.split("-")
    fmt, one, n = parts[1], parts[-1] == "one", p["n"]
    q, scale, z = _quantised(env.rng(), n, fmt)
    k = 1 if one else 0
    with Arenas(env.ctx) as A, traced(env):
        i, o = A.input("iq", _raw(q, k), 0), A.output("cf32_out", 8 * n, 8 if one else 0)
        env.api.expand_iq_d(env.ctx, i.addr + k * Q.BYTES[fmt], fmt, scale, n, o.addr)
        A.check()
        got = o.get(np.uint32)
    pair = fmt != "sc16" and not one        # two samples, four words per work item; an odd last sample goes alone
    env.bits(got, z.view(np.uint32), f"iq_expand {fmt}", 4 if pair else 2, 4 * (n // 2) if pair else None)


@runner(["ring-sc16", "ring-sc8", "ring-uc8"], ())
def run_ring(env, p):
    """the staging ring's own expansion (no profile name: it runs on the ring's copy stream): what take_d hands out has the bits
    of the host expansion (test_ring_gpu.py, test_iq8_gpu.py)"""
    fmt, n = env.case[5:], p["n"]
    q, scale, z = _quantised(env.rng(), n, fmt)
    ring = env.api.StagingRing(env.ctx, n, depth=2, fmt=fmt, scale=scale)
    try:
        ring.put(q)
        d = ring.take_d(timeout_ms=10_000)
        env.ctx.synchronize()
        got = env.ctx.download(d, (2 * n,), np.uint32)
    finally:
        ring.close()
    pair = fmt != "sc16"
    env.bits(got, z.view(np.uint32), f"ring expansion {fmt}", 4 if pair else 2, 4 * (n // 2) if pair else None)


# ================================================================================================================ resizing
# bars: test_dptr_gpu.py (bit identity with the oracle / f64_ref.py)
@runner(["resize1d-f32", "resize1d-f64"], lambda c: ("resize1d" if c.endswith("f32") else "resize1d_f64",))
def run_resize1d(env, p):
    f64 = env.case.endswith("f64")
    x = env.rng().random(p["n_in"], dtype=F32)
    n_out = p["n_out"]
    with Arenas(env.ctx) as A, traced(env):
        i = A.input("sig", x.astype(F64) if f64 else x, 8 if f64 else 4)
        o = A.output("out", (8 if f64 else 4) * n_out, 8 if f64 else 12)
        env.ctx.call("tsdr_resize1d_f64_d" if f64 else "tsdr_resize1d_d", i.ptr, x.size, n_out, o.ptr)
        A.check()
        got = o.get(F64 if f64 else F32)
    env.bits(got, R64.resize1d(x.astype(F64), n_out) if f64 else O.imresize1d(x, n_out), env.case)


@runner(["naive-f32", "naive-f64"], lambda c: ("naive_resample" if c.endswith("f32") else "naive_resample_f64",))
def run_naive(env, p):
    f64 = env.case.endswith("f64")
    x = env.rng().random(p["n"], dtype=F32)
    up = p["up"]
    with Arenas(env.ctx) as A, traced(env):
        i = A.input("in", x.astype(F64) if f64 else x, 8 if f64 else 4)
        o = A.output("out", (8 if f64 else 4) * x.size * up, 8 if f64 else 12)
        env.ctx.call("tsdr_naive_resample_f64_d" if f64 else "tsdr_naive_resample_d", i.ptr, x.size, up, o.ptr)
        A.check()
        got = o.get(F64 if f64 else F32)
    env.bits(got, R64.naive_resample(x.astype(F64), up) if f64 else O.naiveResampler(x, up), env.case)


@runner(["resize2d-f32", "resize2d-f64"], lambda c: ("resize2d" if c.endswith("f32") else "resize2d_f64",))
def run_resize2d(env, p):
    f64 = env.case.endswith("f64")
    shape, size = (p["h_in"], p["w_in"]), (p["h_out"], p["w_out"])
    img = np.asfortranarray(env.rng().random(shape, dtype=F32))
    a = img.astype(F64, order="F") if f64 else img
    with Arenas(env.ctx) as A, traced(env):
        i = A.input("img", a.ravel(order="F"), 8 if f64 else 4)
        o = A.output("out", (8 if f64 else 4) * size[0] * size[1], 8 if f64 else 12)
        env.ctx.call("tsdr_resize2d_f64_d" if f64 else "tsdr_resize2d_d", i.ptr, shape[0], shape[1], size[0], size[1], o.ptr)
        A.check()
        got = o.get(F64 if f64 else F32)
    want = R64.resize2d(a, *size) if f64 else O.imresize2d(img, size)
    env.bits(got, want.ravel(order="F"), env.case)      # (column-major, as the kernel numbers its output pixels)


# ============================================================================================ f32 Bluestein and its helpers
@runner(["blu-batch3", "blu-L"], lambda c: ("blu_pre", "blu_mul", "blu_post") if c == "blu-batch3" else ("blu_b", "blu_pre", "blu_mul"))
def run_blu(env, p):
    """tsdr_fft_c2c_d on the chirp-z route, both directions: 2 * FFT_TOL against numpy in complex128 (test_fft_any_length,
    test_fft_c2c_at_every_phase).  On a context of its own: the chirp and its transform are made at a length's first use."""
    n, batch = p["n"], p["batch"]
    x = _crandn(env.rng(), n * batch).reshape(batch, n)
    x *= (1.0 + np.arange(batch, dtype=F32))[:, None]         # each row its own amplitude
    c = env.tsdr.Context(0)
    try:
        for dr, ref in ((-1, np.fft.fft(x.astype(C128), axis=1)), (1, np.fft.ifft(x.astype(C128), axis=1))):
            with Arenas(c) as A, traced(env, c):
                i, o = A.input("in", x, 8), A.output("out", 8 * n * batch, 8)
                c.call("tsdr_fft_c2c_d", i.ptr, o.ptr, n, batch, dr)
                A.check()
                got = o.get(C64, (batch, n))
            for b in range(batch):      # every row against its own largest value
                env.within(np.abs(got[b].astype(C128) - ref[b]) / np.max(np.abs(ref[b])), 2 * FFT_TOL, f"fft_c2c dir {dr} row {b}")
    finally:
        c.close()


@runner("cac-blu", ("blu_chirp", "blu_post", "cac_power", "cac_finish"))
def run_cac(env, p):
    """calculate_autocorrelation of complex IQ at a length with no native route: 2 * CORR_TOL of the largest lag against numpy in
    complex128 (test_autocorr_complex_gpu.py: LIN_BAR, lin_err).  On a context of its own (the chirp is made at first use)."""
    n, cnt = p["n"], p["cnt"]
    m = np.arange(n)
    z = (((1 + 0.5j) + 0.3 * _crandn(env.rng(), n, C128)) * np.exp(2j * np.pi * 37 * m / n) * 3e-3).astype(C64)      # carrier128
    F = np.fft.fft(z.astype(C128))
    want = np.abs(np.fft.ifft(F * np.conj(F))[:cnt]) ** 2
    c = env.tsdr.Context(0)
    try:
        with Arenas(c) as A, traced(env, c):
            i, o = A.input("z", z, 8), A.output("lags", 4 * cnt, 4)
            n_out = C.c_size_t(0)
            c.call("tsdr_autocorr_cplx_d", i.ptr, n, 1.0, 0.0, float(cnt), 0, o.ptr, C.byref(n_out))
            A.check()
            got = o.get(F32)
        assert n_out.value == cnt
    finally:
        c.close()
    env.within(np.abs(got.astype(F64) - want) / np.max(want), 2 * CORR_TOL, "complex autocorrelation, linear")


@runner("spectrum-blu-real", ("spectrum_out", "blu_post"))
def run_spectrum_blu(env, p):
    """getSpectrum of real samples at a chirp-z length: 2 * FFT_TOL on the magnitudes (test_spectrum_vs_oracle, test_spectrum_at_every_phase)"""
    N = p["n"]
    sig = (env.rng().standard_normal(N + 10, dtype=F32) + F32(3.0)).astype(F32)
    want = R64.spectrum(sig, N, log_scale=False)
    with Arenas(env.ctx) as A, traced(env):
        i, y = A.input("sig", sig, 4), A.output("y", 4 * N, 12)
        env.ctx.call("tsdr_spectrum_d", i.ptr, 0, N, 1, y.ptr)
        A.check()
        got = y.get(F32)
    env.within(np.abs(np.sqrt(got.astype(F64)) - np.sqrt(want)) / np.sqrt(want.max()), 2 * FFT_TOL, "spectrum magnitudes")


@runner("waterfall-960-real", ("r2c", "waterfall_out"))
def run_waterfall_generic(env, p):
    """getWaterfall of real samples at a length the whole-row launch declines: r2c, batched passes, the writer; 4 * FFT_TOL on
    the magnitudes (test_welch_and_waterfall), every segment against its own largest value"""
    N, nb = p["N"], p["nb"]
    rng = env.rng()
    sig = rng.standard_normal(N * nb + 123, dtype=F32)
    sig[: N * nb] *= np.repeat(1.0 + np.arange(nb, dtype=F32) / nb, N)
    want = S64.waterfall(sig, N)
    with Arenas(env.ctx) as A, traced(env):
        i, m = A.input("sig", sig, 4), A.output("waterfall", 8 * N * nb, 8)
        env.ctx.call("tsdr_waterfall_d", i.ptr, 0, sig.size, N, m.ptr)
        A.check()
        got = m.get(F64, (N, nb), "F")
    err = np.abs(np.sqrt(got) - np.sqrt(want)) / np.sqrt(want.max(axis=0))[None, :]
    env.within(err.ravel(order="F"), 4 * FFT_TOL, "waterfall magnitudes, per segment")


# ================================================================================================= autocorrelation helpers
def _ac(env, entry, x, phase, Fs, mind, maxd, log, cnt, out_phase=4):
    with Arenas(env.ctx) as A, traced(env):
        i, o = A.input("x", x, phase), A.output("lags", 4 * cnt, out_phase)
        n_out = C.c_size_t(0)
        env.ctx.call(entry, i.ptr, x.size, Fs, mind, maxd, log, o.ptr, C.byref(n_out))
        A.check()
        assert n_out.value == cnt, (n_out.value, cnt)
        return o.get(F32)


@runner("ac-pow2", ("ac_power", "ac_finish"))
def run_ac_pow2(env, p):
    """n = 2 * 2^k real samples: 2e-4 dB against the oracle (test_autocorr_real_at_every_phase)"""
    x = O.abs2(_search_signal(p["n"]))
    k0, cnt = p["k0"], p["cnt"]
    want, _ = O.calculate_autocorrelation(x, 1.0, float(k0), float(k0 + cnt))
    got = _ac(env, "tsdr_autocorr_d", x, 4, 1.0, float(k0), float(k0 + cnt), 1, cnt)
    env.within(np.abs(got.astype(F64) - want), 2e-4, "lags in dB")


@runner("ac-pack-iq-odd", ("ac_pack",))
def run_ac_pack(env, p):
    """IQ from an odd sample: 2e-4 dB against the oracle (test_autocorr_iq_at_both_phases_takes_its_route)"""
    z = _search_signal(p["n"], key=1)
    cnt = p["cnt"]
    want, _ = O.calculate_autocorrelation(O.abs2(z), 1.0, 0.0, float(cnt))
    got = _ac(env, "tsdr_autocorr_iq_d", z, 8, 1.0, 0.0, float(cnt), 1, cnt)
    assert env.seen.get("ac_fold", 0) == 1
    env.within(np.abs(got.astype(F64) - want), 2e-4, "lags in dB")


@runner("ac-fold-odd", ("ac_fold",))
def run_ac_fold(env, p):
    """an odd number of real samples: 2e-4 dB against the oracle (test_autocorr_real_at_every_phase, n = 100 003)"""
    x = O.abs2(_search_signal(p["n"], key=2))
    cnt = p["cnt"]
    want, _ = O.calculate_autocorrelation(x, 1.0, 0.0, float(cnt))
    got = _ac(env, "tsdr_autocorr_d", x, 12, 1.0, 0.0, float(cnt), 1, cnt, 8)
    assert "ac_pack" not in env.seen
    env.within(np.abs(got.astype(F64) - want), 2e-4, "lags in dB")


@runner("ac-finish", ("ac_finish",))
def run_ac_finish(env, p):
    """tsdr_autocorr_finish_d: 2e-4 dB against 10 log10(r^2) in double (test_autocorr_partial_finish_argmax_at_offsets)"""
    k0, cnt = p["k0"], p["cnt"]
    corr = (0.5 + env.rng().random(k0 + cnt, dtype=F32)).astype(F32)
    with Arenas(env.ctx) as A, traced(env):
        i, o = A.input("corr", corr, 4), A.output("dB", 4 * cnt, 12)
        env.ctx.call("tsdr_autocorr_finish_d", i.ptr, k0, cnt, 1, o.ptr)
        A.check()
        got = o.get(F32)
    env.within(np.abs(got.astype(F64) - 20 * np.log10(np.abs(corr[k0:].astype(F64)))), 2e-4, "dB")


@runner("pc", ("pc_pack", "pc_cross", "pc_real"))
def run_pc(env, p):
    """tsdr_autocorr_partial_d over a segment that wraps around the end of the signal: CORR_TOL of the largest lag against the same
    sums in complex128 (test_autocorr_partial_finish_argmax_at_offsets)"""
    n, m0, cnt, n_lags = p["n"], p["m0"], p["cnt"], p["n_lags"]
    x = (env.rng().random(n) ** 2).astype(F32)
    vlen = cnt + n_lags - 1
    u, v = x[(m0 + np.arange(cnt)) % n].astype(F64), x[(m0 + np.arange(vlen)) % n].astype(F64)
    M2 = G.pow2_at_least(cnt + vlen)
    want = np.fft.irfft(np.conj(np.fft.rfft(u, M2)) * np.fft.rfft(v, M2), M2)[:n_lags]
    with Arenas(env.ctx) as A, traced(env):
        i, o = A.input("x", x, 4), A.output("part", 4 * n_lags, 12)
        env.ctx.call("tsdr_autocorr_partial_d", i.ptr, 0, n, m0, cnt, n_lags, o.ptr)
        A.check()
        got = o.get(F32)
    env.within(np.abs(got.astype(F64) - want) / np.max(np.abs(want)), CORR_TOL, "partial sums")


@runner("group-acc", ())
def run_group_acc(env, p):
    """the sharded search of two members sharing the device adds the second member's partial sums with k_acc (no profile name: it
    runs on the root's stream): the lags of the one-context search within 2e-4 dB, the same findmax
    (test_members_sharing_one_device_run_the_split_logic)"""
    cnt = p["cnt"]
    Fs = 1e6
    x = O.abs2(_search_signal(2 * cnt, key=3))
    G1, p1, _ = env.ctx.autocorr_search(x, Fs, 0.0, cnt / Fs, 50, 90)
    g = env.tsdr.Group([0, 0])
    try:
        G2, p2, _ = g.autocorr_search(x, Fs, 0.0, cnt / Fs, 50, 90, route="sharded")
        assert g.timing()[0] == "sharded"
    finally:
        g.close()
    assert G1.size == G2.size == cnt and p1 == p2
    env.within(np.abs(G1.astype(F64) - G2), 2e-4, "sharded lags against the one-context search, dB", cap=G.ACC_BLOCKS * G.BLOCK)


# ================================================================================================================== Float64
@runner("spectrum-f64-blu", ("spectrum_f64_load", "spectrum_f64_out", "fft64_blue_post", "fft64_pass"))
@runner("spectrum-f64-blu-L", ("fft64_blue_prep", "fft64_blue_mul"))
def run_spectrum64(env, p):
    """tsdr_spectrum_f64_d: 1e-11 of the largest bin against numpy in complex128 (test_spectrum_f64, test_spectra_f64_at_offsets)"""
    N = p["N"]
    sig = env.rng().standard_normal(N + 3)
    want = R64.spectrum(sig, N, log_scale=False)
    with Arenas(env.ctx) as A, traced(env):
        i, y = A.input("sig", sig, 8), A.output("y", 8 * N, 8)
        env.ctx.call("tsdr_spectrum_f64_d", i.ptr, 0, N, 1, y.ptr)
        A.check()
        got = y.get(F64)
    env.within(np.abs(got - want) / np.max(want), 1e-11, "spectrum_f64")


@runner("autocorr-f64", ("autocorr_f64_load", "autocorr_f64_power", "autocorr_f64_out", "fft64_scale"))
def run_autocorr64(env, p):
    """tsdr_autocorr_f64_d: 1e-11 of the largest value against the complex128 restatement (test_autocorr_f64)"""
    n, cnt = p["n"], p["cnt"]
    x = np.abs(_crandn(env.rng(), p["len"], C128)) ** 2
    want = R64.autocorr(x, 1.0, 0, float(cnt), log_scale=False)
    with Arenas(env.ctx) as A, traced(env):
        i, o = A.input("x", x, 8), A.output("lags", 8 * cnt, 8)
        n_out = C.c_size_t(0)
        env.ctx.call("tsdr_autocorr_f64_d", i.ptr, x.size, 1.0, 0.0, float(cnt), 0, o.ptr, C.byref(n_out))
        A.check()
        got = o.get(F64)
    assert n_out.value == cnt == want.size and n == 2 * cnt
    env.within(np.abs(got - want) / np.max(want), 1e-11, "autocorr_f64")


@runner(["welch-f64-big", "seg64-blu-post", "seg64-blu-prep"],
        lambda c: {"welch-f64-big": ("seg64_widen", "welch64_acc", "waterfall64_rows"), "seg64-blu-post": ("seg64_blue_post", "waterfall64_rows"),
                   "seg64-blu-prep": ("seg64_blue_prep", "seg64_blue_mul")}[c])
def run_spectra64(env, p):
    """tsdr_welch_f64_d / tsdr_waterfall_f64_d on the chunked route: 1e-12 of the largest value against numpy in complex128
    (test_welch_waterfall_f64); every segment carries its own amplitude"""
    N, nb = p["N"], p["nb"]
    sig = env.rng().standard_normal(N * nb + N // 7)
    sig[: N * nb] *= np.repeat(1.0 + np.arange(nb) / nb, N)
    ww, wm = S64.welch(sig, N, lin=True), S64.waterfall(sig, N)
    with Arenas(env.ctx) as A, traced(env):
        i, y, m = A.input("sig", sig, 8), A.output("welch", 8 * N, 8), A.output("waterfall", 8 * N * nb, 0)
        env.ctx.call("tsdr_welch_f64_d", i.ptr, 0, sig.size, N, 1, y.ptr)
        env.ctx.call("tsdr_waterfall_f64_d", i.ptr, 0, sig.size, N, m.ptr)
        A.check()
        gy, gm = y.get(F64), m.get(F64, (N, nb), "F")
    env.within(np.abs(gy - ww) / np.max(ww), 1e-12, "welch_f64")
    env.within((np.abs(gm - wm) / np.max(wm)).ravel(order="F"), 1e-12, "waterfall_f64")


def _resampler_run(env, r, x, dtype):
    b = 8 if dtype == F64 else 4
    n_out = x.size * r.upCoeff
    with Arenas(env.ctx) as A, traced(env):
        i, o = A.input("in", x, 0), A.output("out", b * n_out, 0)
        fn = env.ctx.lib.tsdr_resampler_run_f64_d if dtype == F64 else env.ctx.lib.tsdr_resampler_run_d
        env.api.check(env.ctx.h, fn(C.c_void_p(r.h), i.ptr, x.size, o.ptr), "tsdr_resampler_run")
        A.check()
        return o.get(dtype)


@runner("resampler-f64", ("lpf_window64", "lpf_altsign64", "resampler64_stuff", "resampler64_filter", "resampler64_out"))
def run_resampler64(env, p):
    """init_resampler(Float64, ...) and resampler!: 1e-12 * log2(N) of the largest output against numpy with the object's own filter
    (test_resampler_f64); the filter itself is held to the oracle's in resampler-f32-odd, which builds it with the same launches"""
    bs, up = p["bufferSize"], p["up"]
    N = bs * up
    x = env.rng().standard_normal(bs)
    with traced(env):
        r = env.ctx.init_resampler(F64, bs, up)
    try:
        want = S64.resampler(x, up, r.lpf64())
        got = _resampler_run(env, r, x, F64)
    finally:
        r.close()
    env.within(np.abs(got - want), 1e-12 * max(1.0, np.log2(N)) * np.max(np.abs(want)), "resampler! (Float64)")


@runner(["resampler-f32-odd", "resampler-f32-mid"],
        lambda c: ("lpf_window64", "lpf_altsign64", "lpf_c32", "resampler_stuff", "resampler_filter", "resampler_out") if c.endswith("odd")
        else ("lpf_herm_half", "resampler_mid"))
def run_resampler32(env, p):
    """test_init_resampler: the filter within 2e-7 of the oracle's, resampler! within 4e-6 of the largest output"""
    bs, up = p["bufferSize"], p["up"]
    o = O.Resampler(bs, up)
    Ho = o.lpf()
    x = env.rng().standard_normal(bs).astype(F32)
    want = np.empty(bs * up, F32)
    o(want, x)
    with traced(env):
        r = env.ctx.init_resampler(F32, bs, up)
        H64, H32 = r.lpf64(), r.lpf()
    try:
        got = _resampler_run(env, r, x, F32)
    finally:
        r.close()
    env.within(np.abs(H64 - Ho) / np.max(np.abs(Ho)), 2e-7, "the filter (ComplexF64)")
    env.within(np.abs(H32.astype(C128) - Ho) / np.max(np.abs(Ho)), 2e-7, "the filter as ComplexF32")
    env.within(np.abs(got.astype(F64) - want) / np.max(np.abs(want)), 4e-6, "resampler!")


# ==================================================================================================== the direct raster kernel
@runner("raster-direct", ("raster_direct_iq",))
def run_raster_direct(env, p):
    """one frame of 8-bit IQ at 16 samples per raster pixel through the FAST frame loop with rasters: no tile fits, the raster comes
    from k_raster_direct; within RTOL of the oracle's sig_to_image (test_frames_fast, test_frames_fast_at_offsets)"""
    S, y_t, x_t, fmt = p["S"], p["y_t"], p["x_t"], p["fmt"]
    assert env.ctx.precision == "fast"
    nE = S + 321
    q, scale, z = _quantised(env.rng(), nE, fmt, clip=0.9)
    P, npx = y_t * x_t, 480000
    o_state = np.zeros((600, 800), F32, order="F")
    o = O.frames(O.SyncXY(600, 800), z, S, y_t, x_t, F32(0.1), o_state, want_raster=True)
    sync = env.tsdr.SyncXY(env.ctx, 600, 800)
    try:
        with Arenas(env.ctx) as A, traced(env):
            i = A.input("iq", _raw(q, 0), 0)
            st = A.input("imageOut_state", np.zeros(npx, F32), 0)
            st.data = None     # in / out: only its surroundings are guarded
            fr, ix, ra = A.output("frames_out", 4 * npx, 0), A.output("sync_idx", 8, 0), A.output("raster_out", 4 * P, 0)
            n = env.api.frames_iq_d(env.ctx, sync, i.addr, fmt, scale, nE, S, y_t, x_t, F32(0.1), True, st.addr, fr.addr, ra.addr, ix.addr)
            A.check()
            got = ra.get(F32)
    finally:
        sync.close()
    assert n == 1 == o["n_frames"]
    want = o["raster"][0].ravel(order="F").astype(F64)       # pixel l + y_t * p of the column-major raster
    # the kernel walks 64-line strips: work item w is line w % 64 of strip (w / 64) % strips, pixel w / (64 * strips) ... reported per pixel
    env.within(np.abs(got.astype(F64) - want) / np.maximum(np.abs(want), 1e-30), RTOL, "raster, relative")


# ===================================================================================================== whole-row FFT launches
def _row_signal(env, mode, N, rows, kind):
    """rows of noise, row r at amplitude 1 + r / rows, and a tail that is no whole segment (the store takes whole rows only)
    -> (what goes up, entry-point arguments' scale, the rows as the kernels see them: (rows, N) complex128)"""
    rng = env.rng()
    amp = 1.0 + np.arange(rows) / rows
    tail = 0 if mode == "store" else 17
    n = rows * N + tail
    if kind == "real":
        sig = rng.standard_normal(n, dtype=F32)
        sig[: rows * N] *= np.repeat(amp.astype(F32), N)
        return sig, None, sig[: rows * N].astype(F64).reshape(rows, N)
    if kind == "cf32":
        sig = _crandn(rng, n)
        sig[: rows * N] *= np.repeat(amp.astype(F32), N)
        return sig, None, sig[: rows * N].astype(C128).reshape(rows, N)
    q, scale, z = _quantised(rng, n, kind, amp=np.concatenate([np.repeat(amp, N), np.ones(tail)]), clip=0.9)
    return q, scale, z[: rows * N].astype(C128).reshape(rows, N)


def _row_names(case):
    _, mode, N, _ = case.split("-")
    return ("welch_rows_acc",) if N == "960" else (G.ROW_NAMES[mode],)


@runner([c for c, *_ in G.ROW_CASES], _row_names)
def run_rows(env, p):
    """getWelch / getWaterfall / batched tsdr_fft_c2c_d with more tiles of rows than the launch has workgroups.  Bars of
    test_fft_path_gpu.py against numpy in complex128: 4 * FFT_TOL for Welch (of the largest bin) and the waterfall (magnitudes),
    FFT_TOL for the stored rows (test_fft_rows_one_launch) -- the waterfall and the stored rows every row against its own largest
    value, since every row has its own amplitude."""
    _, mode, _, kind = env.case.split("-")
    N, rows, T, grid = p["N"], p["rows"], p["T"], p["grid"]
    up, scale, seg = _row_signal(env, mode, N, rows, kind)
    X = np.fft.fft(seg, axis=1)
    cplx = int(kind != "real")
    n = up.size // 2 if scale is not None else up.size
    trip = lambda r: f"row {r}: tile {r // T}, trip {r // T // grid + 1} of its workgroup's tile loop"      # noqa: E731
    with Arenas(env.ctx) as A, traced(env):
        i = A.input("sig", up if scale is None else _raw(up, 0), 8 if kind == "cf32" else 4 if kind == "real" else 0)
        if mode == "welch":
            y = A.output("welch", 4 * N, 4)
            if scale is None:
                env.ctx.call("tsdr_welch_d", i.ptr, cplx, n, N, 1, y.ptr)
            else:
                env.api.welch_iq_d(env.ctx, i.addr, kind, scale, n, N, True, y.addr)
        elif mode == "wfall":
            y = A.output("waterfall", 8 * N * rows, 8)
            if scale is None:
                env.ctx.call("tsdr_waterfall_d", i.ptr, cplx, n, N, y.ptr)
            else:
                env.api.waterfall_iq_d(env.ctx, i.addr, kind, scale, n, N, y.addr)
        else:
            y = A.output("rows", 8 * N * rows, 8)
            env.ctx.call("tsdr_fft_c2c_d", i.ptr, y.ptr, N, rows, -1)
        A.check()
        if mode == "welch":
            got = y.get(F32)
        elif mode == "wfall":
            got = y.get(F64, (N, rows), "F").T
        else:
            got = y.get(C64, (rows, N))
    if mode == "welch":
        bar = 4 * FFT_TOL
        P = X.real * X.real + X.imag * X.imag
        total = P.sum(axis=0)
        # a tile dropped (or added twice) must move the sum by ten bars at least: the largest bin of every single tile's sum
        tiles = np.add.reduceat(P, np.arange(0, rows, T), axis=0)
        weakest = float(np.min(tiles.max(axis=1)) / total.max())
        print(f"    {env.case}: dropping any one of the {tiles.shape[0]} tiles moves relmax by >= {weakest:.3e} (bar {bar:.1e})")
        assert tiles.shape[0] == p["ntiles"] and weakest >= 10 * bar, (weakest, bar)
        env.within(np.abs(got.astype(F64) - np.fft.fftshift(total)) / total.max(), bar, "welch", cap=N)
        return
    if mode == "wfall":
        want = np.sqrt(np.fft.fftshift(X.real * X.real + X.imag * X.imag, axes=1))
        err, bar = np.abs(np.sqrt(got) - want) / want.max(axis=1)[:, None], 4 * FFT_TOL
    else:
        err, bar = np.abs(got.astype(C128) - X) / np.abs(X).max(axis=1)[:, None], FFT_TOL
    worst = err.max(axis=1)
    print(f"    {env.case}: worst row {float(worst.max()):.3e} (bar {bar:.1e})")
    bad = ~(worst < bar)
    assert not bad.any(), f"{env.case}: {int(bad.sum())} of {rows} rows miss {bar:g}; first {trip(int(np.argmax(bad)))}: {float(worst[np.argmax(bad)]):.3e}"
