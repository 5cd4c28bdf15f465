"""Host-side checks of the fold family's domain table (no GPU): every column of tests/fold_domain_cases.py is recomputed from the
references' own coordinates, so the conditions that make tests/test_fold_domain_gpu.py's comparisons mean something -- a clamp that
binds, a tap at n - 1, a weight of exactly 1, the kernel a case reaches -- are asserted and not assumed; and the window that FAR's
reference runs on is checked against the whole-buffer reference."""
import math

import numpy as np
import pytest

import cfold_ref as CF
import fold_domain_cases as K
import fold_ref as FR
from test_cstack_gpu import CASES as OLD_CASES, _n as old_n

ENTRY_PREFIXES = ["fold", "fold_scan", "cfold", "cfold_scan", "cstack", "ctrack_stack", "ctrack_probe", "gram"]


@pytest.mark.parametrize("name", K.ALL)
def test_every_case_is_accepted_and_ends_where_the_table_says(name):
    """the headers' refusal rules restated: T >= 2, t0 >= 0, t0 + F T <= n in f64, n in [2, 2^31), P < 2^31; n = ceil(t0 + F T); an
    `end` case has t0 + F T == n exactly, so one sample less is refused"""
    c = K.CASES[name]
    assert K.accepted(c) and c["n"] == K.n_of(c)
    assert not K.accepted(c, n=c["n"] - 1), "n is the smallest buffer the call fits"
    end = c["t0"] + float(c["F"]) * c["T"]
    assert (end == float(c["n"])) == c["end"], (end, c["n"])
    # the period scan's three trials T - 0.25, T - 0.125, T are exact in f64, and the largest one is the table's T
    assert [c["T"] - 0.25 + k * 0.125 for k in range(3)][2] == c["T"]
    assert K.accepted(c, T=c["T"] - 0.25) == (name != "P1"), "P1's smallest trial is below T = 2: the scan refuses it"


@pytest.mark.parametrize("name", K.ALL)
def test_routes_and_clamp_counts_are_the_tables(name):
    """W and both routes by the headers' rule; low / high clamped pixels and d == 0 / d == 1 from the references' coordinates"""
    c = K.CASES[name]
    assert K.span(c) == c["W"]
    assert K.route(c, K.FOLD_STAGE_MAX) == c["envelope"] and K.route(c, K.CFOLD_STAGE_MAX) == c["coherent"]
    got, last = K.counts(c)
    assert got == (c["low"], c["high"], c["d0"], c["d1"]), (name, got)
    assert last <= c["n"] - 1
    if c["high"] or c["d1"]:
        assert last == c["n"] - 1, "the last sample of the buffer is a tap"
    if c["envelope"] == "direct":
        assert c["low"] == c["high"] == 0, "the envelope fold's direct kernel cannot clamp (fold_domain_cases)"


def test_the_table_reaches_every_kernel_and_every_clamp():
    """all sixteen fold kernels; and the tile and the direct route of the coherent family each see a low clamp, a high clamp and d == 1"""
    seen = set()
    for c in K.CASES.values():
        for prefix in ENTRY_PREFIXES:
            seen.add(prefix + "_" + (c["envelope"] if prefix.startswith("fold") else c["coherent"]))
    assert seen == {p + "_" + r for p in ENTRY_PREFIXES for r in ("tile", "direct")}
    for r in ("tile", "direct"):
        rows = [c for c in K.CASES.values() if c["coherent"] == r]
        assert any(c["low"] for c in rows) and any(c["high"] for c in rows) and any(c["d1"] for c in rows), r
    assert any(c["low"] and c["high"] for c in K.CASES.values() if c["envelope"] == "tile")
    assert K.CASES["LONG"]["F"] > K.GRAM_MAX_FRAMES and K.CASES["G32"]["F"] == 32
    assert K.CASES["FAR"]["t0"] > 2.0 ** 24 and K.CASES["FAR"]["t0"] == 16778450.625


def test_the_data_is_what_the_table_says():
    for name in K.ALL:
        c = K.CASES[name]
        z = K.samples(name)
        assert z.dtype == K.C64 and z.size == c["n"] - K.window(c)[0] and np.isfinite(z.view(K.F32)).all()
        assert np.array_equal(z, K.samples(name)) and K.seed(name) != K.seed("U")
    raw = K.raw_sc8("FAR")
    assert raw.dtype == np.int8 and raw.size == 2 * K.CASES["FAR"]["n"] and raw.min() == -127 and raw.max() == 127
    assert np.array_equal(K.samples("FAR")[:3], (raw[2 * K.window(K.CASES["FAR"])[0]:][:6].astype(np.float64) / 128.0).astype(K.F32).view(K.C64))
    for fmt in ("sc16", "sc8", "uc8"):
        q, scale, z = K.quantise(K.samples("UPS"), fmt)
        assert z.size == K.CASES["UPS"]["n"] and np.max(np.abs(z - K.samples("UPS"))) <= 1.01 * scale * math.sqrt(2.0)
        if fmt in K.PAD_CODE:
            assert not np.any(q == K.PAD_CODE[fmt]), "the pad code is not data"
            p = K.padded(q, fmt)
            assert p.nbytes % 4 == 0 and p.size == q.size + 2 and np.array_equal(p[:q.size], q) and np.all(p[q.size:] == K.PAD_CODE[fmt])
    assert not np.any(raw == K.PAD_CODE["sc8"])
    t = K.track(K.CASES["LONG"])
    assert t.shape == (1500, 2) and np.all((t[:, 0] >= 0) & (t[:, 0] < 1)) and t[3, 1] == 0.02 * 3 - 0.03
    assert K.track(K.CASES["UPS"])[1, 0] == 0.37 + K.KAPPA_TRUE + 0.01


# ---------------------------------------------------------------- the window
def test_far_window_moves_no_coordinate_by_more_than_n_ulp():
    """FAR on z[w0:] at t0 - w0: the subtraction is exact, the clamps are the whole buffer's, and every coordinate lies within
    n 2^-52 samples of the whole-buffer one (the rounding of t0 + f T + ... at 2^24) -- the term fold_domain_cases.far_term carries
    into the GPU test's bounds"""
    c = K.CASES["FAR"]
    w0, t0w = K.window(c)
    assert w0 == int(math.floor(c["t0"])) - 2 and t0w + w0 == c["t0"] and t0w == 2.625
    cw = K.windowed(c)
    assert cw["n"] == c["n"] - w0 and K.accepted(cw)
    worst = 0.0
    for f in range(c["F"]):
        raw, k, d = K.coordinates(c, f)
        raw_w, k_w, d_w = K.coordinates(cw, f)
        assert raw_w.min() > 0.0, "the window's own start never clamps"
        u, u_w = np.clip(raw, 0.0, c["n"] - 1.0), np.clip(raw_w, 0.0, cw["n"] - 1.0)
        worst = max(worst, float(np.max(np.abs((u - w0) - u_w))))     # u - w0 is exact: u is a multiple of 2^-28 below 2^25
        assert np.array_equal(raw > c["n"] - 1.0, raw_w > cw["n"] - 1.0), "the same pixels clamp"
    print(f"FAR: windowed against whole-buffer coordinates, max difference {worst:.3g} samples, n 2^-52 = {c['n'] * 2.0 ** -52:.3g}")
    assert 0.0 < worst <= c["n"] * 2.0 ** -52
    assert K.far_term(c, 1.0) == 2.0 * c["n"] * 2.0 ** -52 and K.far_term(K.CASES["LONG"], 1.0) == 0.0


@pytest.mark.parametrize("name", ["U", "D"])
def test_windowed_reference_is_the_whole_buffer_reference(name):
    """the window helper on the old cases U (t0 3.25) and D (t0 11599.9): the envelope and the coherent reference on z[w0:] at t0 - w0
    equal the whole-buffer ones -- U to 1e-12 relative; D, whose whole-buffer coordinates round at 2^16, to the bound that rounding
    sets: the largest slope 2 amax times n 2^-52 samples (far_term's rule)"""
    c = dict(OLD_CASES[name], name=name)
    c["n"] = old_n(c)
    rng = np.random.default_rng(K.seed(name))
    z = (rng.standard_normal(c["n"]) + 1j * rng.standard_normal(c["n"]) + 0.5).astype(K.C64)
    w0, t0w = K.window(c)
    assert w0 == {"U": 1, "D": 11597}[name]
    a = FR.amplitudes(z)
    whole = FR.fold(a, c["t0"], c["T"], c["F"], c["y"], c["x"])
    win = FR.fold(a[w0:], t0w, c["T"], c["F"], c["y"], c["x"])
    tol = 1e-12 * float(np.max(np.abs(whole))) if name == "U" else K.far_term(c, a.max())
    print(f"window {name}: envelope, max difference {np.max(np.abs(win - whole)):.3g}, bound {tol:.3g}")
    assert np.max(np.abs(win - whole)) <= tol
    zz = CF.samples(z)
    whole = CF.zfold_mean(zz, c["t0"], c["T"], K.KAPPA_TRUE, c["F"], c["y"], c["x"])
    win = CF.zfold_mean(zz[w0:], t0w, c["T"], K.KAPPA_TRUE, c["F"], c["y"], c["x"])
    tol = 1e-12 * float(np.max(np.abs(whole))) if name == "U" else math.sqrt(2.0) * K.far_term(c, a.max())
    print(f"window {name}: coherent, max difference {np.max(np.abs(win - whole)):.3g}, bound {tol:.3g}")
    assert np.max(np.abs(win - whole)) <= tol
