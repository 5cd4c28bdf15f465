"""GPU tests of the frame Gram matrix (include/tempest_hip_gram.h): tsdr_ctrack_gram_iq_d against tests/gram_ref.py within the header's
bound, its Hermitian bits, its ties to the kernels that exist (the carrier scan's scores, the probe's rho_f and E_f), a constant turn
per frame against the plain matrix, repeats / integer formats / the host form bit for bit, every refusal, F == 0, and the two things
the matrix is for: blind_track on the capability inputs of tests/test_gram_host.py and coherent_period_scan around the true period.

Shapes: tests/test_cstack_gpu.py's CASES U, M, D, S, R, X (F 3 - 7, both kernels, y_t = 70 with a ragged second line tile, 8 x 16) and
    X1   8 x 16, T 5000.5,  F 1,  t0 0.5    gram_direct   a single frame
    B33  70 x 48, T 2450.3, F 33, t0 3.25   gram_tile     crosses the 32-row block: two blocks per component, 81.5 KiB of LDS
    B64  20 x 48, T 1500.7, F 64, t0 0.5    gram_direct   the maximum
with n = ceil((F + 1) T) + 7 for the three new ones.  Every device pointer sits inside a guarded arena (tests/dptr_util.py), `gram` and
the track at 8 mod 16 or 0 mod 16; A.check() proves the guard words around them intact.  Which case reaches which kernel is asserted
by profile name.  Captures and references are made once per case (functools caches); nothing modifies them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cfold_ref as CF
import cstack_ref as CS
import ctrack_ref as R
import dptr_util as D
import gram_ref as GR
import test_ctrack_host as TH
import test_gram_host as H
from test_cstack_gpu import CASES, IQ_PHASE, KAPPA_TRUE, KERNEL, ZS_PHASE, _capture, _n, _null, _pkg, _profiled, _quantised, _report
from test_ctrack_gpu import _case_probe, _case_stack, _track

pytestmark = pytest.mark.gpu

F32, C64 = np.float32, np.complex64
NEW = {
    "X1": dict(y=8, x=16, T=5000.5, F=1, t0=0.5, kernel="direct", iq_phase=8),
    "B33": dict(y=70, x=48, T=2450.3, F=33, t0=3.25, kernel="tile", iq_phase=0),
    "B64": dict(y=20, x=48, T=1500.7, F=64, t0=0.5, kernel="direct", iq_phase=8),
}
ALL = list(CASES) + list(NEW)


def _case(name):
    if not isinstance(name, str):   # the case itself: a dict with y, x, T, F, t0 (tests/fold_domain_cases.py's rows)
        return name
    if name in CASES:
        return dict(CASES[name], kernel=KERNEL[name], iq_phase=IQ_PHASE[name], n=_n(CASES[name]))
    c = NEW[name]
    return dict(c, n=int(math.ceil((c["F"] + 1) * c["T"])) + 7)


@functools.lru_cache(maxsize=None)
def _cap(name):
    """(iq complex64[n], amax) of a case"""
    if name in CASES:
        return _capture(name)
    c = _case(name)
    iq = _pkg("synth").synth_leak(60.0 * c["T"], c["x"], c["y"], 60.0, c["n"], snr_db=20.0)
    iq.setflags(write=False)
    return iq, float(np.abs(CS.samples(iq)).max())


def _trk(name):
    """the test track of a case: test_ctrack_gpu._track's formula, a_f = 0.37 + f kappa_true + 0.01 f^2, b_f = 0.02 f - 0.03"""
    if name in CASES:
        return _track(name)
    f = np.arange(_case(name)["F"], dtype=np.float64)
    return np.ascontiguousarray(np.stack([0.37 + f * KAPPA_TRUE + 0.01 * f * f, 0.02 * f - 0.03], axis=1))


@functools.lru_cache(maxsize=None)
def _ref(name, tracked):
    """(G of the reference, the bound of every entry)"""
    c = _case(name)
    iq, amax = _cap(name)
    G = GR.gram(CS.samples(iq), c["t0"], c["T"], _trk(name) if tracked else None, c["F"], c["y"], c["x"])
    B = GR.eps_matrix(amax, c["y"] * c["x"], G)
    G.setflags(write=False)
    B.setflags(write=False)
    return G, B


def _gram_d(ctx, iq, fmt, scale, n, t0, T, track, F, y, x, gram):
    ctx.call("tsdr_ctrack_gram_iq_d", iq, fmt, C.c_float(scale), n, C.c_double(t0), C.c_double(T), track, F, y, x, gram)


def _case_gram(ctx, name, d_iq, n, d_track, gram, fmt=0, scale=1.0):
    c = _case(name)
    _gram_d(ctx, d_iq, fmt, scale, n, c["t0"], c["T"], d_track, c["F"], c["y"], c["x"], gram)


def _matrix(arena, F):
    return _pkg("gram").gram_matrix(arena.get(np.float64), F)


# ---------------------------------------------------------------- 1., 2. against the reference; the Hermitian bits
@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_matches_the_reference(ctx, name, tracked):
    """every entry within the header's bound (ACCURACY); G[g][f] has the bits of conj(G[f][g]), Im of the diagonal is +0; the kernel
    by profile name; the NULL track and the test track"""
    c = _case(name)
    iq = _cap(name)[0]
    F = c["F"]
    G, B = _ref(name, tracked)
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, c["iq_phase"])
        d_tr = A.input("track", _trk(name), 8).ptr if tracked else _null()
        d_g = A.output("gram", 16 * F * F, 8)
        names = _profiled(ctx, lambda: _case_gram(ctx, name, d_iq.ptr, iq.size, d_tr, d_g.ptr))
        A.check()
        raw = d_g.get(np.uint64).reshape(F, F, 2)
        got = _matrix(d_g, F)
    assert names == {"gram_" + c["kernel"], "gram_sum"}, names
    assert np.isfinite(got.view(np.float64)).all()
    ratio = np.abs(got - G) / B
    print(f"gram {name} {'track' if tracked else 'NULL'}: max |G - ref| / bound {ratio.max():.4f} (diagonal {np.diag(ratio).max():.4f}); "
          f"max |G - ref| / sqrt(E_f E_g) {np.max(np.abs(got - G) / np.sqrt(np.outer(np.diag(G).real, np.diag(G).real))):.3g}")
    assert np.all(ratio <= 1.0), (name, tracked, float(ratio.max()))
    sign = np.uint64(1) << np.uint64(63)
    for f in range(F):
        assert raw[f, f, 1] == 0, "Im G[f][f] is +0"
        assert got[f, f].real > 0
        for g in range(f):
            assert raw[g, f, 0] == raw[f, g, 0] and raw[g, f, 1] == raw[f, g, 1] ^ sign, (f, g)
    if F > 1:
        off = got - np.diag(np.diag(got))
        assert np.abs(off.imag).max() > 100.0 * B.max() or np.abs(off.real).max() > 100.0 * B.max(), "the comparison means something"


# ---------------------------------------------------------------- 3. ties to the kernels that exist
@pytest.mark.parametrize("name", ["U", "D", "X"])
def test_energy_is_the_carrier_scans_score(ctx, name):
    """tsdr_cfold_scan_iq_d's score at 5 values of kappa against gram_energy(G, f kappa) of the NULL-track matrix, within the sum of
    the two contracts' bounds: the score's 2 eps_z sqrt(P ref) + P eps_z^2 and the mean of the entries' bounds"""
    c = _case(name)
    iq, amax = _cap(name)
    F, P = c["F"], c["y"] * c["x"]
    kappas = [KAPPA_TRUE + 0.11 * k for k in range(5)]
    with D.Arenas(ctx) as A:
        d_iq, d_g, d_sc = A.input("iq", iq, c["iq_phase"]), A.output("gram", 16 * F * F, 0), A.output("score", 8 * 5, 8)
        _case_gram(ctx, name, d_iq.ptr, iq.size, _null(), d_g.ptr)
        ctx.call("tsdr_cfold_scan_iq_d", d_iq.ptr, 0, C.c_float(1.0), iq.size, C.c_double(c["t0"]), C.c_double(c["T"]), C.c_double(kappas[0]),
                 C.c_double(0.11), 5, F, c["y"], c["x"], d_sc.ptr)
        A.check()
        G, score = _matrix(d_g, F), d_sc.get(np.float64)
    B = _ref(name, False)[1]
    f = np.arange(F, dtype=np.float64)
    for k, kappa in enumerate(kappas):
        e = ctx.gram_energy(G, f * (kappas[0] + k * 0.11))
        ez = CF.eps_z(F, amax)
        bound = 2.0 * ez * math.sqrt(P * score[k]) + P * ez * ez + GR.eps_energy(B, F)
        _report(f"gram {name}: energy at kappa {kappa:.3f} against the scan's score", abs(e - score[k]), bound)
        assert abs(e - score[k]) <= bound
    assert score.max() > 3.0 * score.min(), "the scan has a peak: the five energies differ"


@pytest.mark.parametrize("name", ["U", "D"])
def test_rows_are_the_probes_rho_and_the_diagonal_its_energy(ctx, name):
    """the probe of every frame against the zstate of a stack along the same track (alpha 0, GIVEN) measures (1/F) sum_g G[f][g], and
    its E_f is G[f][f]: within the probe's bounds + the stack's eps_s through Cauchy-Schwarz + the entries' bounds"""
    c = _case(name)
    iq, amax = _cap(name)
    F, P = c["F"], c["y"] * c["x"]
    with D.Arenas(ctx) as A:
        d_iq, d_tr = A.input("iq", iq, c["iq_phase"]), A.input("track", _trk(name), 8)
        d_zs, d_out, d_g = A.output("zstate", 8 * P, ZS_PHASE[name]), A.output("out", 8 * (4 * F + 1), 8), A.output("gram", 16 * F * F, 8)
        _case_stack(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, 0.0, CS.GIVEN, d_zs.ptr, _null(), _null())
        _case_probe(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, d_zs.ptr, d_out.ptr)
        _case_gram(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, d_g.ptr)
        A.check()
        rho, E_f, _, E_s = _pkg("ctrack").probe_record(d_out.get(np.float64), F)
        G = _matrix(d_g, F)
    B = _ref(name, True)[1]
    worst = [0.0, 0.0]
    for f in range(F):
        b_rho = R.eps_rho(amax, P, E_f[f], E_s) + math.sqrt(E_f[f] * P) * CS.eps_s(F, amax) + float(np.sum(B[f])) / F
        b_E = R.eps_ef(amax, P, E_f[f]) + B[f, f]
        e_rho, e_E = abs(rho[f] - np.sum(G[f]) / F), abs(E_f[f] - G[f, f].real)
        worst = [max(worst[0], e_rho / b_rho), max(worst[1], e_E / b_E)]
        assert e_rho <= b_rho and e_E <= b_E, (name, f, e_rho, b_rho, e_E, b_E)
        assert abs(rho[f]) > 100.0 * b_rho
    print(f"gram {name}: max |rho_f - row mean| / bound {worst[0]:.4f}, max |E_f - G[f][f]| / bound {worst[1]:.4f}")


# ---------------------------------------------------------------- 4. a constant turn per frame
@pytest.mark.parametrize("name", ["U", "R", "B33"])
def test_a_track_without_slopes_turns_the_plain_matrix(ctx, name):
    """along a track with b = 0 the matrix is the NULL-track matrix with entry (f, g) turned by exp(-2 pi i (a_f - a_g)), within the bound"""
    c = _case(name)
    iq = _cap(name)[0]
    F = c["F"]
    track = _trk(name).copy()
    track[:, 1] = 0.0
    with D.Arenas(ctx) as A:
        d_iq, d_tr = A.input("iq", iq, c["iq_phase"]), A.input("track", track, 0)
        a, b = A.output("gram NULL", 16 * F * F, 8), A.output("gram track", 16 * F * F, 0)
        _case_gram(ctx, name, d_iq.ptr, iq.size, _null(), a.ptr)
        _case_gram(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, b.ptr)
        A.check()
        plain, turned = _matrix(a, F), _matrix(b, F)
    w = np.exp(-2j * np.pi * track[:, 0])
    ratio = np.abs(turned - plain * np.outer(w, w.conj())) / _ref(name, False)[1]
    print(f"gram {name}: constant turns, max difference / bound {ratio.max():.4f}")
    assert np.all(ratio <= 1.0)
    assert np.abs(turned - plain).max() > 100.0 * _ref(name, False)[1].max(), "the turn matters"


# ---------------------------------------------------------------- 5. repeats, formats, the host form
@pytest.mark.parametrize("name", ["U", "D", "B33", "B64"])
def test_two_calls_leave_identical_bits(ctx, name):
    c = _case(name)
    iq = _cap(name)[0]
    F = c["F"]
    with D.Arenas(ctx) as A:
        d_iq, d_tr = A.input("iq", iq, c["iq_phase"]), A.input("track", _trk(name), 8)
        outs = [A.output(f"gram {k}", 16 * F * F, 8 * k) for k in range(2)]
        for o in outs:
            _case_gram(ctx, name, d_iq.ptr, iq.size, d_tr.ptr, o.ptr)
        A.check()
        assert np.array_equal(outs[0].get(np.uint64), outs[1].get(np.uint64))
        assert np.isfinite(outs[0].get(np.float64)).all()


@pytest.mark.parametrize("fmt", ["sc16", "sc8", "uc8"])
def test_integer_formats_give_the_bits_of_the_expanded_buffer(ctx, fmt):
    """cases U (tiled) and D (direct): sc16 / sc8 / uc8 in, the bits of the same call on the host-expanded ComplexF32"""
    code = {"sc16": 1, "sc8": 2, "uc8": 3}[fmt]
    for name in ("U", "D"):
        F = CASES[name]["F"]
        raw, scale, z = _quantised(name, fmt)
        with D.Arenas(ctx) as A:
            d_raw, d_z, d_tr = A.input("raw", raw, 0), A.input("expanded", z, 8), A.input("track", _trk(name), 8)
            a, b = A.output("gram raw", 16 * F * F, 8), A.output("gram expanded", 16 * F * F, 8)
            _case_gram(ctx, name, d_raw.ptr, z.size, d_tr.ptr, a.ptr, fmt=code, scale=scale)
            _case_gram(ctx, name, d_z.ptr, z.size, d_tr.ptr, b.ptr)
            A.check()
            assert np.array_equal(a.get(np.uint64), b.get(np.uint64)), (name, fmt)
            assert np.isfinite(a.get(np.float64)).all() and np.all(np.diag(_matrix(a, F)).real > 0)


def test_host_form_has_the_bits_of_the_device_form(ctx):
    """Context.ctrack_gram (host arrays) and ctrack_gram_d give the same bits, with and without a track; the caller's arrays are inputs"""
    for name in ("U", "B64"):
        c = _case(name)
        iq = _cap(name)[0]
        F = c["F"]
        track = _trk(name)
        keep = track.copy()
        for tr in (None, track):
            G = ctx.ctrack_gram(iq, c["t0"], c["T"], tr, F, c["y"], c["x"])
            assert G.shape == (F, F) and G.dtype == np.complex128 and np.array_equal(track, keep)
            with D.Arenas(ctx) as A:
                d_iq, d_g = A.input("iq", iq, 8), A.output("gram", 16 * F * F, 8)
                d_tr = A.input("track", tr, 8).addr if tr is not None else None
                ctx.ctrack_gram_d(d_iq.addr, "cf32", 1.0, iq.size, c["t0"], c["T"], d_tr, F, c["y"], c["x"], d_g.addr)
                A.check()
                assert np.array_equal(G.view(np.float64).view(np.uint64).reshape(-1), d_g.get(np.uint64)), (name, tr is None)
    # the raw host symbol
    c, iq = _case("X"), _cap("X")[0]
    out = np.zeros(2 * 9)
    rc = ctx.lib.tsdr_ctrack_gram_iq(ctx.h, C.c_void_p(iq.ctypes.data), 0, 1.0, iq.size, c["t0"], c["T"], None, 3, c["y"], c["x"],
                                     C.c_void_p(out.ctypes.data))
    assert rc == 0 and np.array_equal(_pkg("gram").gram_matrix(out, 3), ctx.ctrack_gram(iq, c["t0"], c["T"], None, 3, c["y"], c["x"]))


# ---------------------------------------------------------------- 6. - 8. refusals, F == 0, untouched memory
def test_refusals_leave_everything_untouched(ctx):
    """every TSDR_EINVAL of the header (REFUSALS), F = 65, 2^16 tiles and a misaligned gram and track among them, and F == 0 (TSDR_OK): nothing is
    launched, and the sentinel-filled output is as uploaded"""
    c = _case("U")
    iq = _cap("U")[0]
    raw = np.zeros(2 * 4096, np.int16)
    n, y, x, F, t0, T = iq.size, c["y"], c["x"], c["F"], c["t0"], c["T"]
    nan, inf = float("nan"), float("inf")
    track = _trk("U")
    long_iq = np.zeros(int(math.ceil(66 * 40.5)) + 8, C64)
    with D.Arenas(ctx) as A:
        d_iq, d_raw, d_tr, d_long = A.input("iq", iq, 8), A.input("raw", raw, 0), A.input("track", track, 8), A.input("long", long_iq, 8)
        d_g = A.output("gram", 16 * 65 * 65, 8)
        good = dict(iq=d_iq.addr, fmt=0, n=n, t0=t0, T=T, tr=d_tr.addr, F=F, y=y, x=x, g=d_g.addr)

        def gram(**kw):
            k = dict(good, **kw)
            _gram_d(ctx, C.c_void_p(k["iq"]), k["fmt"], 1.0, k["n"], k["t0"], k["T"], C.c_void_p(k["tr"]), k["F"], k["y"], k["x"], C.c_void_p(k["g"]))

        bad = [dict(iq=0), dict(fmt=4), dict(fmt=-1), dict(y=0), dict(x=-3), dict(y=65536, x=32768), dict(n=1), dict(n=1 << 31), dict(F=-1),
               dict(T=nan), dict(T=inf), dict(t0=nan), dict(t0=inf), dict(T=1.5), dict(t0=-0.5), dict(F=F + 1), dict(t0=t0 + 20.0),
               dict(n=n - 20), dict(iq=d_iq.addr + 4), dict(iq=d_raw.addr + 8, fmt=1, n=2048, F=1), dict(iq=d_raw.addr + 4, fmt=2, n=2048, F=1),
               dict(tr=d_tr.addr + 4), dict(g=0), dict(g=d_g.addr + 4), dict(y=64 * 65536, x=16),
               dict(iq=d_long.addr, n=long_iq.size, T=40.5, t0=0.0, F=65, y=4, x=4, tr=0)]

        def refused():
            for kw in bad:
                with pytest.raises(AssertionError, match="invalid|ctrack_gram"):
                    gram(**kw)
            gram(F=0)
            gram(F=0, tr=0)
            assert ctx.lib.tsdr_ctrack_gram_iq_d(None, d_iq.ptr, 0, 1.0, n, t0, T, d_tr.ptr, F, y, x, d_g.ptr) == -1

        assert _profiled(ctx, refused) == set(), "nothing is enqueued"
        A.check()
        assert np.array_equal(d_g.get(np.uint32), D.sentinel_words(d_g.size // 4)[d_g.lead // 4: (d_g.lead + d_g.payload) // 4])
        # the context still serves valid calls afterwards: 64 frames of the same buffer pass where 65 did not, and the NULL track
        gram(iq=d_long.addr, n=long_iq.size, T=40.5, t0=0.0, F=64, y=4, x=4, tr=0)
        gram(tr=0)
        A.check()
        assert np.all(np.isfinite(d_g.get(np.float64)[:2 * F * F]))
    # the host form: the same refusals and a non-finite track entry, host arrays untouched; F == 0 touches nothing
    out = np.full(2 * 65 * 65, 7.0)
    z = iq.copy()
    bad_nan, bad_inf = track.copy(), track.copy()
    bad_nan[F - 1, 0], bad_inf[2, 1] = nan, inf
    host = dict(good, tr=track.ctypes.data, g=out.ctypes.data)
    for kw in (dict(T=nan), dict(F=F + 1), dict(fmt=5), dict(y=0), dict(tr=bad_nan.ctypes.data), dict(tr=bad_inf.ctypes.data), dict(g=0),
               dict(F=65), dict(F=0), dict(F=0, tr=0)):
        k = dict(host, **kw)
        rc = ctx.lib.tsdr_ctrack_gram_iq(ctx.h, C.c_void_p(z.ctypes.data), k["fmt"], 1.0, n, k["t0"], k["T"], C.c_void_p(k["tr"]), k["F"],
                                         k["y"], k["x"], C.c_void_p(k["g"]))
        assert rc == (0 if kw.get("F") == 0 else -1), kw
    assert np.all(out == 7.0) and np.array_equal(z, iq)
    with pytest.raises(AssertionError):
        ctx.ctrack_gram(iq, t0, T, track[:-1], F, y, x)


# ---------------------------------------------------------------- 9. the capabilities
@pytest.mark.parametrize("which", [0, 1])
def test_blind_track_on_the_capability_inputs(ctx, which):
    """The inputs of tests/test_gram_host.py: 66 x 160, T 9150.37, t0 3.25, -10 dB, 24 frames, (0) a ramp of 0.06 turns/frame per
    frame, on which ladder + refine_track never locks (0.133), (1) a random walk of 0.12 turns per frame (0.475).  blind_track, two
    passes, then the correlation of its stack's magnitude with the noiseless card: the CPU reference gives 0.554 for both.
    Asserted: within 0.01 of the reference, and >= 0.52."""
    y, x, T, t0, F = TH.CAP["y"], TH.CAP["x"], TH.CAP["T"], TH.CAP["t0"], H.RAMP["frames"]
    P = y * x
    iq = H.hard_captures()[which]
    ref_tracked, ref_blind = H.hard_reference(which)
    card = TH.cap_card()
    with D.Arenas(ctx) as A:
        d_iq, d_zs, d_mag = A.input("iq", iq, 8), A.output("zstate", 8 * P, 8), A.output("mag", 4 * P, 4)
        track, rho = ctx.blind_track(d_iq.addr, "cf32", 1.0, iq.size, t0, T, F, y, x, passes=2, zstate=d_zs.addr, mag=d_mag.addr)
        A.check()
        blind = TH.corr(d_mag.get(F32), card)
    print(f"blind track {'ramp' if which == 0 else 'walk'}: {blind:.3f} (reference {ref_blind:.3f}; ladder + refine_track {ref_tracked:.3f}); "
          f"mean |rho| {rho.mean():.4g}")
    assert abs(blind - ref_blind) <= 0.01 and blind >= 0.52, (blind, ref_blind)
    assert track.shape == (F, 2) and rho.shape == (F,) and np.all(rho > 0)


# ---------------------------------------------------------------- 10. the joint (T, kappa) search
def test_period_scan_picks_the_references_period(ctx):
    """coherent_period_scan over 9 periods 2 samples apart around 9150.37 on the drift-free capture picks the index the numpy
    reference picks (the true period); the reference's runner-up has 0.882 of its maximum's energy (tests/test_gram_host.py).  Every
    energy agrees with the reference's within the mean of the entries' bounds (every |w_f conj(w_g)| is 1) plus 1e-9 of it for the
    carrier's own error (the energy is flat at its maximum); kappa at the maximum within one step of the 16 F grid both refine from."""
    y, x, t0 = TH.CAP["y"], TH.CAP["x"], TH.CAP["t0"]
    iq = TH.drift_captures()[0]
    z, amax = CF.samples(iq), float(np.abs(CF.samples(iq)).max())
    periods = H.scan_periods()
    e_ref, k_ref, best_ref = H.scan_reference()
    out = []
    with D.Arenas(ctx) as A:
        d_iq = A.input("iq", iq, 8)
        names = _profiled(ctx, lambda: out.append(ctx.coherent_period_scan(d_iq.addr, "cf32", 1.0, iq.size, t0, y, x, periods)))
        A.check()
    e, kappas, best = out[0]
    print(f"period scan: best {best} (reference {best_ref}); energies / reference {np.round(e / e_ref, 7)}; kappa {kappas[best]:.5f}")
    assert names == {"gram_tile", "gram_sum"}, names
    assert best == best_ref == len(periods) // 2
    for k, T in enumerate(periods):
        F = min(CS.fold_plan(iq.size, t0, T)[0], GR.MAX_FRAMES)
        bound = GR.eps_energy(GR.eps_matrix(amax, y * x, GR.gram(z, t0, T, None, F, y, x)), F) + 1e-9 * e_ref[k]
        assert abs(e[k] - e_ref[k]) <= bound, (k, e[k], e_ref[k], bound)
    assert abs(kappas[best] - k_ref[best]) <= 1.0 / (16 * H.RAMP["frames"])
