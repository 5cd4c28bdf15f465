"""GPU tests of the tuner (include/tempest_hip_tune.h): tsdr_tune_iq_d against tests/tune_ref.py within the header's bound, and bit for
bit against itself -- a stream cut into calls three ways, the integer formats against the host-expanded ComplexF32, repeats, pointers at
offsets inside larger buffers, the host form --, the identity against tsdr_iq_expand_d, every refusal with nothing enqueued, and the
capability the feature exists for: the jammed wideband capture of tests/test_tune_host.py tuned on the GPU and folded by tsdr_fold_iq_d.

Shapes are the smallest at which the kernel can go wrong: every n is a little over two tiles of tsdr_tune_tile(L, D) outputs (the last
tile holds one output), so the largest case reads 2 * 1024 * 64 samples; the stream starts at m0 = 2^40 + 12345 with an odd nu_fix, so
the 64-bit phase wraps many times.  Every device pointer sits inside a guarded arena (tests/dptr_util.py): A.check() proves the words
around out[0 .. n_out) and around hist intact.  The "tune" kernel has NO grid cap (one workgroup per tile, fewer than 2^31 tiles by the
refusal of n >= 2^31), so no case has to run past one.  References are made once per case (functools caches); nothing modifies them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import dptr_util as D
import test_hires_host as HH
import tune_ref as R

pytestmark = pytest.mark.gpu

F32, C64 = np.float32, np.complex64
M0 = (1 << 40) + 12345
NU = 0xD1B54A32D192ED03          # odd, about 0.82 turns per sample
PHI = 0x0123456789ABCDEF
EINVAL = -1


def _pkg(name):
    return HH._pkg(name)


def _null():
    return C.c_void_p(0)


def _ceil_div(a, b):
    return -((-a) // b)


def _tune_raw(ctx, form, iq, fmt, scale, n, m0, nu, phi, taps, L, Dm, j0, hist, n_hist, out, cap):
    """(rc, n_out, message) of one call, no exception"""
    n_out = C.c_size_t(12345678)
    rc = getattr(ctx.lib, form)(ctx.h, iq, fmt, C.c_float(scale), n, m0, nu, phi, taps, L, Dm, j0, hist, n_hist, out, cap, C.byref(n_out))
    return rc, n_out.value, ctx.lib.tsdr_last_error(ctx.h).decode()


def _tune_d(ctx, iq, fmt, scale, n, m0, nu, phi, taps, L, Dm, j0, hist, n_hist, out, cap):
    rc, n_out, msg = _tune_raw(ctx, "tsdr_tune_iq_d", iq, fmt, scale, n, m0, nu, phi, taps, L, Dm, j0, hist, n_hist, out, cap)
    assert rc == 0, msg
    return n_out


@functools.lru_cache(maxsize=None)
def _noise(n, seed=5):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(C64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _taps(L, Dm):
    """a low-pass with a few taps made negative and unequal, so that no symmetry hides an index error"""
    h = _pkg("tune").design_lowpass(L, Dm).astype(np.float64)
    h = h * (1.0 + 0.25 * np.cos(0.7 * np.arange(L))) - (0.01 if L > 1 else 0.0) * ((np.arange(L) % 5) == 2)
    h = h.astype(F32)
    h.setflags(write=False)
    return h


def _ptr(addr):
    return C.c_void_p(addr)


def _run_whole(ctx, x, fmt, scale, taps, Dm, m0=M0, nu=NU, phi=PHI, iq_phase=0, out_phase=0, hist_phase=0, with_hist=True, iq_skip=0, n=None):
    """one call on the whole stream, no history -> (out uint32[n_out, 2], hist uint32[L - 1, 2] or None).  iq_skip: the stream starts
    that many bytes into the uploaded array (an 8-bit buffer at an odd sample: 2 bytes, which no arena phase can be)"""
    L = taps.size
    n = (x.nbytes - iq_skip) // (8, 4, 2, 2)[fmt] if n is None else n
    j0 = _ceil_div(m0, Dm)
    want = R.n_out(m0, n, L, Dm, j0)
    with D.Arenas(ctx) as A:
        d_iq, d_taps = A.input("iq", x, iq_phase), A.input("taps", taps, 4)
        d_out = A.output("out", 8 * want, out_phase)
        d_hist = A.output("hist", 8 * (L - 1), hist_phase) if with_hist else None
        got = _tune_d(ctx, _ptr(d_iq.addr + iq_skip), fmt, scale, n, m0, nu, phi, d_taps.ptr, L, Dm, j0, d_hist.ptr if with_hist else _null(), 0,
                      d_out.ptr, want)
        A.check()
        assert got == want
        return d_out.get(np.uint32).reshape(-1, 2), (d_hist.get(np.uint32).reshape(-1, 2) if with_hist else None)


def _as_c64(words):
    return words.reshape(-1).view(F32).view(C64)


# ---------------------------------------------------------------- identity against tsdr_iq_expand_d
@pytest.mark.parametrize("Dm", [1, 3])
@pytest.mark.parametrize("fmt", ["cf32", "sc16", "sc8", "uc8"])
def test_identity_is_the_expansion(ctx, fmt, Dm):
    """L = 1, h = [1], nu_fix = phi_fix = 0: the outputs are tsdr_iq_expand_d's values, every D-th of them -- all four formats"""
    api = _pkg("api")
    n, rng = 3002, np.random.default_rng(3)   # (even: an arena holds whole words)
    code, dt, _ = api.IQ_FORMATS[fmt]
    if fmt == "cf32":
        q, scale = _noise(n), 1.0
    else:
        info = np.iinfo(dt)
        q, scale = rng.integers(info.min, info.max + 1, 2 * n).astype(dt), 1.0 / 1024.0
    one = np.ones(1, F32)
    m0 = 7
    j0 = _ceil_div(m0, Dm)
    want = R.n_out(m0, n, 1, Dm, j0)
    with D.Arenas(ctx) as A:
        d_iq, d_taps = A.input("iq", q, 0), A.input("taps", one, 4)
        d_out, d_exp = A.output("out", 8 * want, 8), A.output("expanded", 8 * n, 0)
        assert _tune_d(ctx, d_iq.ptr, code, scale, n, m0, 0, 0, d_taps.ptr, 1, Dm, j0, _null(), 0, d_out.ptr, want) == want
        ctx.call("tsdr_iq_expand_d", d_iq.ptr, code, C.c_float(scale), n, d_exp.ptr)
        A.check()
        got, exp = d_out.get(F32).reshape(-1, 2), d_exp.get(F32).reshape(-1, 2)
    first = j0 * Dm - m0
    assert want == len(range(first, n, Dm)) and np.array_equal(got, exp[first::Dm])
    assert np.array_equal(exp.reshape(-1).view(C64), api.expand_iq(q, fmt, scale) if fmt != "cf32" else q)


# ---------------------------------------------------------------- the bound against the f64 reference
@functools.lru_cache(maxsize=None)
def _bound_case(L, Dm, n_out_want):
    """(x, reference outputs, bound) of the stream that gives n_out_want outputs from m0 = M0"""
    j0 = _ceil_div(M0, Dm)
    n = (j0 + n_out_want - 1) * Dm + L - M0 + (Dm - 1 if n_out_want else 0)   # the last window complete, the next one not
    if n_out_want == 0:
        n = L - 1
    x = _noise(max(n, 1))[:n]
    ref = R.whole(x, M0, NU, PHI, _taps(L, Dm), Dm)
    assert ref.size == n_out_want, (ref.size, n_out_want)
    ref.setflags(write=False)
    return x, ref, R.bound(L, float(np.abs(x).max()) if n else 0.0, _taps(L, Dm))


def _check_bound(ctx, L, Dm, n_out_want, label):
    x, ref, bound = _bound_case(L, Dm, n_out_want)
    out, hist = _run_whole(ctx, x, 0, 1.0, _taps(L, Dm), Dm, out_phase=8 if L % 2 else 4, hist_phase=4)
    got = _as_c64(out).astype(np.complex128)
    assert got.size == n_out_want and np.isfinite(got.view(np.float64)).all()
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    print(f"tune {label} L {L} D {Dm} n {x.size} n_out {n_out_want}: max |y - ref| / bound {err / bound if bound else 0.0:.4f}")
    assert err <= bound, (L, Dm, err, bound)
    if got.size > 8:
        assert np.abs(ref).max() > 100.0 * bound, "the comparison means something"
    keep = min(L - 1, x.size)   # the history: the last mixed samples, within the bound of one product
    if keep:
        u = R.mixed(x, M0, NU, PHI)[-keep:]
        assert np.abs(_as_c64(hist)[L - 1 - keep:].astype(np.complex128) - u).max() <= 8 * R.ULP * float(np.abs(x).max())


@pytest.mark.parametrize("Dm", [1, 2, 3, 4, 7, 64])
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 1024])
def test_within_the_bound(ctx, L, Dm):
    """two tiles and one output: |y - y_ref| <= (L + 8) 2^-24 A H1 for every pair of L and D, D > L among them (samples no window uses)"""
    _check_bound(ctx, L, Dm, 2 * _pkg("tune").tune_tile(L, Dm) + 1, "two tiles + 1")


@pytest.mark.parametrize("L,Dm", [(63, 4), (65, 3), (3, 7), (1024, 64)])
@pytest.mark.parametrize("edge", [-1, 0, 1])
def test_tile_edges(ctx, L, Dm, edge):
    """n_out = one tile - 1, one tile, one tile + 1"""
    _check_bound(ctx, L, Dm, _pkg("tune").tune_tile(L, Dm) + edge, f"tile {edge:+d}")


@pytest.mark.parametrize("L,Dm", [(2, 1), (63, 4), (3, 7), (1024, 64)])
def test_one_output_and_none(ctx, L, Dm):
    """n = L - 1: no output, TSDR_OK, out untouched, the history is the whole call; n = L (+ D - 1): one output"""
    _check_bound(ctx, L, Dm, 1, "one output")
    x = _noise(L - 1)
    j0 = _ceil_div(M0, Dm)
    with D.Arenas(ctx) as A:
        d_iq, d_taps = A.input("iq", x, 0), A.input("taps", _taps(L, Dm), 4)
        d_out, d_hist = A.output("out", 64, 8), A.output("hist", 8 * (L - 1), 8)
        assert _tune_d(ctx, d_iq.ptr, 0, 1.0, L - 1, M0, NU, PHI, d_taps.ptr, L, Dm, j0, d_hist.ptr, 0, d_out.ptr, 0) == 0
        A.check()
        lo = d_out.lead // 4
        assert np.array_equal(d_out.get(np.uint32), D.sentinel_words(d_out.size // 4)[lo:lo + 16]), "out untouched"
        hist = _as_c64(d_hist.get(np.uint32)).astype(np.complex128)
    assert np.abs(hist - R.mixed(x, M0, NU, PHI)).max() <= 8 * R.ULP * float(np.abs(x).max())


# ---------------------------------------------------------------- chaining, bit for bit
CH = dict(L=65, Dm=4, n=40013)


_WHOLE = {}   # the single call on the chaining stream, made once


def _whole_bits(ctx):
    if "w" not in _WHOLE:
        _WHOLE["w"] = _run_whole(ctx, _noise(CH["n"], 9), 0, 1.0, _taps(CH["L"], CH["Dm"]), CH["Dm"], hist_phase=8)
    return _WHOLE["w"]


def _cuts(kind):
    L, n = CH["L"], CH["n"]
    if kind == "ones":
        c = [1] * (L + 3)
    elif kind == "short":
        c = [L - 2] * (n // (L - 2))
    else:
        c = [int(v) | 1 for v in np.random.default_rng(17).integers(1, 3000, 200)]   # odd: no multiple of D
    out, pos = [], 0
    for v in c:
        v = min(v, n - pos)
        if v:
            out.append(v)
            pos += v
    if pos < n:
        out.append(n - pos)
    return out


@pytest.mark.parametrize("kind", ["ones", "short", "random"])
def test_chained_calls_are_the_single_call(ctx, kind):
    """one stream of 40 013 samples at L = 65, D = 4 cut into single samples (L + 3 of them, then the rest), into chunks of L - 2, into
    random odd chunks: the outputs AND the final history have the bits of the single call; tune_plan carries m0, j0, n_hist"""
    mod = _pkg("tune")
    L, Dm, n = CH["L"], CH["Dm"], CH["n"]
    x, taps = _noise(n, 9), _taps(L, Dm)
    want_out, want_hist = _whole_bits(ctx)
    with D.Arenas(ctx) as A:
        d_iq, d_taps = A.input("iq", x, 0), A.input("taps", taps, 4)
        d_out, d_hist = A.output("out", 8 * want_out.shape[0], 8), A.output("hist", 8 * (L - 1), 4)
        m0, j0, nh, pos, done = M0, _ceil_div(M0, Dm), 0, 0, 0
        for c in _cuts(kind):
            k, nxt = mod.tune_plan(m0, c, L, Dm, j0, nh)
            got = _tune_d(ctx, _ptr(d_iq.addr + 8 * pos), 0, 1.0, c, m0, NU, PHI, d_taps.ptr, L, Dm, j0, d_hist.ptr, nh, _ptr(d_out.addr + 8 * done),
                          want_out.shape[0] - done)
            assert got == k
            m0, j0, nh, pos, done = nxt["m0"], nxt["j0"], nxt["n_hist"], pos + c, done + k
        A.check()
        assert pos == n and done == want_out.shape[0] and nh == L - 1
        assert np.array_equal(d_out.get(np.uint32).reshape(-1, 2), want_out), "outputs bit for bit"
        assert np.array_equal(d_hist.get(np.uint32).reshape(-1, 2), want_hist), "final history bit for bit"


def test_tuner_class_and_host_form_chain(ctx):
    """Tuner.push_d over three buffers and Context.tune over two host calls: the bits of the single call"""
    mod, api = _pkg("tune"), _pkg("api")
    L, Dm, n = CH["L"], CH["Dm"], CH["n"]
    x, taps = _noise(n, 9), _taps(L, Dm)
    want_out, want_hist = _whole_bits(ctx)
    t = ctx.tuner(NU, taps, Dm, phi_fix=PHI, m0=M0)
    with D.Arenas(ctx) as A:
        d_iq, d_out = A.input("iq", x, 0), A.output("out", 8 * want_out.shape[0], 0)
        pos = done = 0
        for c in (1000, 33, n - 1033):
            done += t.push_d(d_iq.addr + 8 * pos, "cf32", 1.0, c, d_out.addr + 8 * done)
            pos += c
        A.check()
        assert np.array_equal(d_out.get(np.uint32).reshape(-1, 2), want_out)
    assert (t.m0, t.j0, t.n_hist) == (M0 + n, _ceil_div(M0, Dm) + want_out.shape[0], L - 1)
    assert np.array_equal(ctx.download(t.d_hist, (L - 1, 2), np.uint32), want_hist)
    t.close()
    y1, h1, nx = ctx.tune(x[:777], NU, taps, Dm, m0=M0, phi_fix=PHI)
    y2, h2, nx2 = ctx.tune(x[777:], NU, taps, Dm, m0=nx["m0"], phi_fix=PHI, j0=nx["j0"], hist=h1, n_hist=nx["n_hist"])
    assert np.array_equal(np.concatenate([y1, y2]).view(np.uint32).reshape(-1, 2), want_out)
    assert np.array_equal(h2.view(np.uint32).reshape(-1, 2), want_hist) and nx2["m0"] == M0 + n
    assert isinstance(t, mod.Tuner) and api is not None


# ---------------------------------------------------------------- formats, repeats, pointers
@pytest.mark.parametrize("fmt", ["sc16", "sc8", "uc8"])
def test_integer_formats_have_the_bits_of_the_expanded_call(ctx, fmt):
    """sc16 / sc8 / uc8 against the ComplexF32 call on (f32(q) - offset) * f32(scale), outputs and history; a repeat returns the same
    bits; an 8-bit buffer that starts at an odd sample"""
    api = _pkg("api")
    L, Dm, n = 63, 4, 20012
    code, dt, _ = api.IQ_FORMATS[fmt]
    info = np.iinfo(dt)
    q = np.random.default_rng(21).integers(info.min, info.max + 1, 2 * n).astype(dt)
    scale = 3.0 / 32768.0 if fmt == "sc16" else 1.0 / 100.0
    taps = _taps(L, Dm)
    a = _run_whole(ctx, np.concatenate([q[:2], q, q[:2]]), code, scale, taps, Dm, iq_skip=q.itemsize * 2, n=n)   # one sample into a larger buffer
    b = _run_whole(ctx, np.ascontiguousarray(api.expand_iq(q, fmt, scale)), 0, 1.0, taps, Dm)
    c = _run_whole(ctx, q, code, scale, taps, Dm, iq_phase=0, out_phase=8)
    for u, v in ((a, b), (a, c)):
        assert np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1])
    assert a[0].shape[0] > 4 * 1024 and np.abs(_as_c64(a[0])).max() > 0


@pytest.mark.parametrize("iq_phase,out_phase,hist_phase", [(8, 8, 8), (8, 4, 4), (0, 12, 12)])
def test_pointers_inside_larger_buffers(ctx, iq_phase, out_phase, hist_phase):
    """iq and out one sample into larger buffers, out and hist float-aligned only: the bits of fresh allocations, every guard intact"""
    L, Dm = 64, 3
    x, taps = _noise(9001, 13), _taps(L, Dm)
    base = _run_whole(ctx, x, 0, 1.0, taps, Dm)
    got = _run_whole(ctx, x, 0, 1.0, taps, Dm, iq_phase=iq_phase, out_phase=out_phase, hist_phase=hist_phase)
    assert np.array_equal(base[0], got[0]) and np.array_equal(base[1], got[1])
    none = _run_whole(ctx, x, 0, 1.0, taps, Dm, with_hist=False)   # hist == NULL with n_hist == 0: the same outputs, no history written
    assert np.array_equal(base[0], none[0])


# ---------------------------------------------------------------- refusals
def test_every_refusal_names_its_argument_and_enqueues_nothing(ctx):
    L, Dm, n = 5, 2, 64
    x, taps = _noise(n), _taps(L, Dm)
    with D.Arenas(ctx) as A:
        d_iq, d_taps = A.input("iq", x, 0), A.input("taps", taps, 4)
        d_out, d_hist = A.output("out", 8 * 64, 0), A.output("hist", 8 * (L - 1), 0)
        ok = dict(iq=d_iq.ptr, fmt=0, scale=1.0, n=n, m0=100, nu=NU, phi=PHI, taps=d_taps.ptr, L=L, Dm=Dm, j0=50, hist=d_hist.ptr, n_hist=0,
                  out=d_out.ptr, cap=64)
        bad = [("iq", dict(iq=_null())), ("taps", dict(taps=_null())), ("out", dict(out=_null())), ("iq_fmt", dict(fmt=4)), ("iq_fmt", dict(fmt=-1)),
               ("n_taps", dict(L=0)), ("n_taps", dict(L=1025)), ("decim", dict(Dm=0)), ("decim", dict(Dm=65)), ("n ", dict(n=1 << 31)),
               ("n_hist", dict(n_hist=-1)), ("n_hist", dict(n_hist=L)), ("n_hist", dict(n_hist=3, m0=2, j0=0)), ("hist", dict(hist=_null(), n_hist=2, j0=49)),
               ("j0", dict(j0=49)), ("j0", dict(j0=47, n_hist=4)), ("out_cap", dict(cap=29)), ("m0", dict(m0=(1 << 64) - 10, j0=(1 << 63) - 5)),
               ("iq", dict(iq=_ptr(d_iq.addr + 4))), ("taps", dict(taps=_ptr(d_taps.addr + 2))), ("hist", dict(hist=_ptr(d_hist.addr + 2))),
               ("out", dict(out=_ptr(d_out.addr + 2)))]
        for name, change in bad:
            a = dict(ok, **change)
            rc, n_out, msg = _tune_raw(ctx, "tsdr_tune_iq_d", a["iq"], a["fmt"], a["scale"], a["n"], a["m0"], a["nu"], a["phi"], a["taps"], a["L"],
                                       a["Dm"], a["j0"], a["hist"], a["n_hist"], a["out"], a["cap"])
            assert rc == EINVAL and name in msg and msg.startswith("tune_iq:"), (name, change, rc, msg)
            assert n_out == 12345678, "n_out is written only by a call that is accepted"
        n_out = C.c_size_t(1)
        assert ctx.lib.tsdr_tune_iq_d(ctx.h, d_iq.ptr, 0, C.c_float(1.0), n, 100, NU, PHI, d_taps.ptr, L, Dm, 50, d_hist.ptr, 0, d_out.ptr, 64,
                                      None) == EINVAL and "n_out" in ctx.lib.tsdr_last_error(ctx.h).decode()
        assert ctx.lib.tsdr_tune_iq_d(None, d_iq.ptr, 0, C.c_float(1.0), n, 100, NU, PHI, d_taps.ptr, L, Dm, 50, d_hist.ptr, 0, d_out.ptr, 64,
                                      C.byref(n_out)) == EINVAL
        # the host form refuses the same (it checks no alignment)
        hx, ht, ho, hh = x.copy(), taps.copy(), np.zeros(64, C64), np.zeros(L - 1, C64)
        for name, change in (("decim", dict(Dm=65)), ("j0", dict(j0=49)), ("out_cap", dict(cap=29)), ("n_hist", dict(n_hist=L))):
            a = dict(ok, **change)
            rc, _, msg = _tune_raw(ctx, "tsdr_tune_iq", hx.ctypes.data, 0, 1.0, n, a["m0"], NU, PHI, ht.ctypes.data, a["L"], a["Dm"], a["j0"],
                                   hh.ctypes.data, a["n_hist"], ho.ctypes.data, a["cap"])
            assert rc == EINVAL and name in msg, (name, msg)
        assert not ho.any() and not hh.any()
        A.check()   # tsdr_synchronize, then every arena: the sentinels of out and hist survive, nothing was enqueued
        lo = d_out.lead // 4
        assert np.array_equal(d_out.get(np.uint32), D.sentinel_words(d_out.size // 4)[lo:lo + 128])
        lo = d_hist.lead // 4
        assert np.array_equal(d_hist.get(np.uint32), D.sentinel_words(d_hist.size // 4)[lo:lo + 2 * (L - 1)])
        # ... and the accepted call: j0 = 50, 30 outputs; then n == 0: TSDR_OK, nothing moves
        assert _tune_d(ctx, **{k: ok[k] for k in ("iq", "fmt", "scale", "n", "m0", "nu", "phi", "taps", "L", "Dm", "j0", "hist", "n_hist", "out", "cap")}) == 30
        ctx.synchronize()
        h_before = ctx.download(d_hist.addr, (L - 1, 2), np.uint32)
        assert _tune_d(ctx, d_iq.ptr, 0, 1.0, 0, 164, NU, PHI, d_taps.ptr, L, Dm, 80, d_hist.ptr, 4, d_out.ptr, 0) == 0
        ctx.synchronize()
        assert np.array_equal(ctx.download(d_hist.addr, (L - 1, 2), np.uint32), h_before)
        A.check()


# ---------------------------------------------------------------- the capability
def test_capability_tuned_fold_recovers_the_card(ctx):
    """the 66 x 160 capture at Fs = 60 * 4 * T with the leak at +0.23 Fs and a carrier 20 dB stronger at -0.31 Fs: shifted by -0.23 Fs,
    low-passed (L = 63) and decimated by 4 on the GPU, folded by tsdr_fold_iq_d (11 frames from t0 = T - 31 / 4 at period T) it
    correlates with the card as the reference's 0.931 does, within 0.01; the raw capture folded at 4 T stays below 0.2"""
    synth = _pkg("synth")
    cap = R.CAP
    _, jammed = R.cap_captures(synth)
    card, taps = R.cap_card(synth), R.cap_taps()
    y, x, T, Dm, L, F = cap["y"], cap["x"], cap["T"], cap["D"], cap["L"], cap["F"]
    ref_tuned = R.corr(R.cap_fold_tuned(R.whole(jammed, 0, R.cap_nu(), 0, taps, Dm)), card)
    n = jammed.size
    want = R.n_out(0, n, L, Dm, 0)
    t = ctx.tuner(R.cap_nu(), taps, Dm)
    with D.Arenas(ctx) as A:
        d_iq, d_out = A.input("iq", jammed, 0), A.output("tuned", 8 * want, 0)
        d_pic, d_raw = A.output("picture", 4 * y * x, 0), A.output("raw picture", 4 * y * x, 0)
        pos = done = 0
        for c in (150001, 150002, n - 300003):          # three buffers of a ring
            done += t.push_d(d_iq.addr + 8 * pos, "cf32", 1.0, c, d_out.addr + 8 * done)
            pos += c
        assert done == want
        ctx.call("tsdr_fold_iq_d", d_out.ptr, 0, C.c_float(1.0), want, C.c_double(T - (L - 1) / 2.0 / Dm), C.c_double(T), F, y, x, C.c_float(0.0),
                 d_pic.ptr)
        ctx.call("tsdr_fold_iq_d", d_iq.ptr, 0, C.c_float(1.0), n, C.c_double(Dm * T), C.c_double(Dm * T), F, y, x, C.c_float(0.0), d_raw.ptr)
        A.check()
        tuned, raw = R.corr(d_pic.get(F32), card), R.corr(d_raw.get(F32), card)
    t.close()
    print(f"capability (GPU): tuned {tuned:.4f} (reference {ref_tuned:.4f}), raw {raw:.4f}")
    assert tuned >= 0.85 and raw <= 0.2
    assert abs(tuned - ref_tuned) <= 0.01
    assert math.isfinite(tuned)
