"""The inventory of capped launches (grid_cap_cases.py) against the sources, its own size arithmetic, and the planners.

  * completeness: every launch of csrc/ whose grid comes from stream_grid / stream_blocks, every step plan_rows adds, argmax_launch
    and group.hip's k_acc has an entry with the text of its work-item expression, and every entry has such a launch: a new capped
    launch without a case, or a launch site that changed, fails here;
  * size arithmetic: for 256 CUs and for 64, every case puts every site it is listed for at cap < work items <= 3 * cap, at a ragged
    size wherever the site can have one;
  * plans: the whole-row cases have more tiles than workgroups -- asked of fft_plan.h itself through tools/host_plan/fft_plan_dump
    --rows, not of a copy of it --, and the frame-loop case reaches k_raster_direct with more work than its grid covers
    (tools/host_plan/plan_dump --one).
No GPU is needed or touched.
"""
import collections
import os
import re
import subprocess

import pytest

import grid_cap_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_EXEMPT = 4


# ---- the scan ----------------------------------------------------------------------------------------------------------------------
def _balanced(text, i):
    """text[i] == '(' -> (the text between it and its closing parenthesis, index past that)"""
    assert text[i] == "("
    depth, j = 0, i
    while True:
        depth += {"(": 1, ")": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1: j], j + 1
        j += 1


def _args(inner):
    """top-level comma split"""
    out, depth, cur = [], 0, ""
    for ch in inner:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    out.append(cur.strip())
    return out


def _squeeze(s):
    return re.sub(r"\s+", " ", s).strip()


def _strip_comments(text):
    """// comments blanked (string literals of these sources hold no //); offsets and line breaks are kept"""
    return re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), text)


def scan_stream_sites(text):
    """[(token, work-item expression)] of every stream_grid( / stream_blocks( call in `text` (their definitions apart)"""
    text = _strip_comments(text)
    found = []
    for m in re.finditer(r"\bstream_(grid|blocks)\(", text):
        line_start = text.rfind("\n", 0, m.start()) + 1
        if re.match(r"\s*static inline int stream_", text[line_start:]) or "return stream_blocks(" in text[line_start: m.end()]:
            continue    # common.h: the two definitions
        inner, _ = _balanced(text, m.end() - 1)
        expr = _squeeze(",".join(_args(inner)[1:]))     # without ctx / cu_count
        start = max(text.rfind(c, 0, m.start()) for c in ";{}") + 1
        stmt = text[start: m.start()]
        launch = re.search(r"\b(TSDR_LAUNCH|hipLaunchKernelGGL)\(", stmt)
        if launch:
            largs = _args(_balanced(text, start + launch.end() - 1)[0])
            token = _squeeze(largs[1] if launch.group(1) == "TSDR_LAUNCH" else largs[0])
        else:       # the grid is formed in a statement of its own: its left-hand side
            token = _squeeze(re.sub(r"(\(unsigned\)|[=(\s])+$", "", stmt))
        found.append((token, expr))
    return found


def scan_tree(csrc=CSRC):
    out = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(csrc, name)) as f:
                out += [(name, tok, expr) for tok, expr in scan_stream_sites(f.read())]
    return out


def scan_plan_rows(csrc=CSRC):
    """{profile name: grid expression} of the steps plan_rows adds"""
    with open(os.path.join(csrc, "fft_plan.h")) as f:
        text = _strip_comments(f.read())
    body = text[text.index("inline void plan_rows("):]
    out = {}
    for m in re.finditer(r"\bpl\.add\(", body):
        a = _args(_balanced(body, m.end() - 1)[0])
        names = re.findall(r'"(\w+)"', a[3])
        grid = a[4]
        if not grid.startswith("std::min"):     # a variable: its last capping assignment above the call
            grid = re.findall(r"unsigned %s = (std::min\(.*?\));" % re.escape(grid), body[: m.start()])[-1]
        for n in names:
            out[n] = _squeeze(grid)
    return out


def scan_own_caps(csrc=CSRC):
    out = {}
    with open(os.path.join(csrc, "autocorr.hip")) as f:
        t = _strip_comments(f.read())
    body = t[t.index("int argmax_launch(tsdr_ctx *ctx"):]
    m = re.search(r"const int ablocks = \(int\)(.*?);", body)
    assert m and re.search(r'TSDR_LAUNCH\(ctx, "argmax", k_argmax, dim3\(ablocks\)', body)
    out["argmax"] = ("autocorr.hip", '"argmax"', _squeeze(m.group(1)))
    with open(os.path.join(csrc, "group.hip")) as f:
        t = _strip_comments(f.read())
    sites = [m for m in re.finditer(r"hipLaunchKernelGGL\(k_acc,", t)]
    assert len(sites) == 1
    a = _args(_balanced(t, sites[0].end() - len("k_acc,") - 1)[0])
    out["k_acc"] = ("group.hip", "k_acc", _squeeze(re.fullmatch(r"dim3\(\(unsigned\)(.*)\)", a[1]).group(1)))
    return out


def check_inventory(csrc=CSRC, sites=None):
    """AssertionError unless the table and the sources under `csrc` name the same launches"""
    sites = G.SITES if sites is None else sites
    have = collections.Counter((s.file, s.token, s.expr) for s in sites)
    want = collections.Counter(scan_tree(csrc))
    missing, stale = want - have, have - want
    assert not missing, "capped launches without an inventory entry (tests/grid_cap_cases.py):\n  " + "\n  ".join(map(str, sorted(missing.elements())))
    assert not stale, "inventory entries without a launch site (changed or removed?):\n  " + "\n  ".join(map(str, sorted(stale.elements())))
    rows = scan_plan_rows(csrc)
    assert rows == {k: v[0] for k, v in G.ROW_STEPS.items()}, (rows, G.ROW_STEPS)
    own = scan_own_caps(csrc)
    assert own == {k: (v["file"], v["token"], v["expr"]) for k, v in G.OWN_CAP.items()}, own


# ---- completeness ------------------------------------------------------------------------------------------------------------------
def test_every_capped_launch_has_an_entry_and_every_entry_a_launch():
    check_inventory()
    assert len(G.SITES) >= 70      # (the scan finds them at all: about 65 TSDR_LAUNCH sites and the statements that form a grid first)


def test_profile_names_are_literals_of_the_entry_s_file():
    for s in G.SITES:
        with open(os.path.join(CSRC, s.file)) as f:
            text = f.read()
        for n in s.names:
            assert f'"{n}"' in text, (s.file, n)
    with open(os.path.join(CSRC, "fft_plan.h")) as f:
        text = f.read()
    for n in G.ROW_STEPS:
        assert f'"{n}"' in text, n


def test_every_entry_has_a_case_or_an_accepted_exemption():
    exempt = [s for s in G.SITES if s.exempt]
    assert len(exempt) <= MAX_EXEMPT
    for s in G.SITES:
        if s.exempt:
            assert s.exempt in G.EXEMPT_REASONS and s.note and not s.cases, s
        else:
            assert s.cases and set(s.cases) <= set(G.CASES), s
    used = {c for s in G.SITES for c in s.cases} | {c for o in G.OWN_CAP.values() for c in o.get("cases", {})} | {c for _, cs in G.ROW_STEPS.values() for c in cs}
    assert used == set(G.CASES), used ^ set(G.CASES)
    for name, (_, cases) in G.ROW_STEPS.items():
        assert cases, name
    # k_argmax is covered where it already was
    f, test, size = G.OWN_CAP["argmax"]["covered_by"]
    with open(os.path.join(ROOT, "tests", f)) as fh:
        text = fh.read()
    m = re.search(r"@pytest\.mark\.parametrize\(\"n\", \[([^\]]*)\]\)\ndef %s\(" % test, text)
    assert m and size in m.group(1) and int(size.replace("_", "")) > G.OWN_CAP["argmax"]["cap"]


def test_the_gpu_module_runs_every_case():
    import test_grid_cap_gpu as T
    assert set(T.RUNNERS) == set(G.CASES), set(T.RUNNERS) ^ set(G.CASES)


# ---- size arithmetic -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cu", G.CU_COUNTS)
def test_every_case_is_past_the_cap_and_ragged(cu):
    for case in G.CASES:
        p = G.params(case, cu)
        for site, work in G.sites_of(case):
            c, w = G.cap_of(site, cu), work(p)
            assert c < w <= 3 * c, (cu, case, site.token, w, c)
            if not site.fixed:
                assert w % G.BLOCK, (cu, case, site.token, w)
        if case.endswith("-vec"):      # the tail that workgroup 0 handles alone: SPV - 1 samples
            assert p["n"] % p["spv"] == p["spv"] - 1, (case, p)
    # three trips for some threads and two for the others wherever the data allows (w3)
    c = G.cap(cu)
    assert 2 * c < G.w3(cu) < 3 * c and G.w3(cu) % 2 == 1 and c < G.w2(cu) < 2 * c


def test_lengths_take_the_route_their_case_names():
    for cu in G.CU_COUNTS:
        for case in ("blu-batch3", "blu-L", "spectrum-blu-real", "cac-blu"):
            p = G.params(case, cu)
            assert not G.is_smooth(p["n"]) and p["L"] == G.pow2_at_least(2 * p["n"] - 1), (case, p)
        b, l = G.params("blu-batch3", cu), G.params("blu-L", cu)
        assert b["L"] <= G.cap(cu) < b["L"] * b["batch"] and l["L"] > G.cap(cu) and l["batch"] == 1
        for case in ("spectrum-f64-blu", "spectrum-f64-blu-L"):
            assert not G.is_smooth(G.params(case, cu)["N"], G.P13)
        assert G.is_smooth(G.params("autocorr-f64", cu)["n"], G.P13)
        assert G.is_smooth(G.params("welch-f64-big", cu)["N"]) and G.params("welch-f64-big", cu)["N"] > 4096
        assert not G.is_smooth(4093, G.P13) and G.pow2_at_least(2 * 4093 - 1) == 8192
        for case in ("seg64-blu-post", "seg64-blu-prep"):       # one chunk: B = nbSeg (spectra64.hip: B <= 2^22 / L)
            assert G.params(case, cu)["nb"] <= (1 << 22) // 8192
        for case in ("resampler-f32-odd", "resampler-f64"):
            p = G.params(case, cu)
            N = p["bufferSize"] * p["up"]
            assert p["bufferSize"] % 2 == 1 and not G.is_smooth(N) and G.is_smooth(N, G.P13), (case, p)
        p = G.params("resampler-f32-mid", cu)
        assert p["bufferSize"] % 2 == 0 and G.is_smooth(p["bufferSize"] // 2) and p["bufferSize"] * p["up"] != 4096
        p = G.params("ac-pow2", cu)
        assert p["n"] == 2 * p["Mc"] and p["Mc"] & (p["Mc"] - 1) == 0 and p["k0"] + p["cnt"] == p["n"] // 2
        p = G.params("pc", cu)
        assert p["cnt"] + p["n_lags"] - 1 <= p["M"] and p["n_lags"] <= p["n"] and p["m0"] < p["n"] < p["m0"] + p["cnt"]   # the segment wraps


# ---- the planners ----------------------------------------------------------------------------------------------------------------------
def _build(tmp, src, exe):
    exe = str(tmp / exe)
    cmd = [HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "host_plan", src), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def fft_plan_dump(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("host_plan"), "fft_plan_dump_main.hip", "fft_plan_dump")


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("host_plan"), "plan_dump_main.hip", "plan_dump")


def _mix3_entries():
    with open(os.path.join(CSRC, "fft_plan.h")) as f:
        text = f.read().replace("\\\n", " ")
    body = re.search(r"#define TSDR_MIX3_LIST\(X\)(.*)", text).group(1)
    return [tuple(int(v) for v in a.split(",")) for a in re.findall(r"X\(([^)]*)\)", body)]


@pytest.mark.parametrize("cu", G.CU_COUNTS)
def test_row_cases_walk_more_tiles_than_workgroups(fft_plan_dump, cu):
    kernels = collections.defaultdict(set)
    for case, mode, N, kind in G.ROW_CASES:
        p = G.params(case, cu)
        r = subprocess.run([fft_plan_dump, "--rows", mode, str(G.ROW_SIG_KIND[kind]), str(N), str(p["rows"]), str(cu)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        m = re.fullmatch(r"(\w+) (\S+) grid=(\d+) block=\d+ rows_per_tile=(\d+) ntiles=(\d+)\n", r.stdout)
        assert m, (case, r.stdout)
        name, kernel, grid, per_tile, ntiles = m.group(1), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))
        assert name == ("welch_rows_acc" if N == 960 else G.ROW_NAMES[mode]) and case in G.ROW_STEPS[name][1], (case, name)
        assert (per_tile, grid, ntiles) == (p["T"], p["grid"], p["ntiles"]), (case, r.stdout, p)      # the table restates the planner
        assert grid < ntiles <= 3 * grid and p["rows"] % per_tile, (case, grid, ntiles)
        kernels[mode].add(kernel)
    # every length of TSDR_MIX3_LIST in every mode, on ComplexF32 / real rows and on integer ones (modes 10 .. 12 and 13 .. 15)
    lengths = {a * b * c for a, b, c, _ in _mix3_entries()}
    assert lengths == {N for _, _, N, _ in G.ROW_CASES if N != 960}
    for mode, base in (("welch", 10), ("wfall", 11), ("store", 12)):
        got = collections.defaultdict(set)
        for k in kernels[mode]:
            if k.startswith("k_fft_mix3<"):
                a = [int(v) for v in k[len("k_fft_mix3<"):-1].split(",")]
                got[a[0] * a[1] * a[2]].add(a[4])
        for N in lengths:
            assert base in got[N], (mode, N, got)
            if mode != "store":
                assert base + 3 in got[N], (mode, N, got)
    # getWelch takes the pass kernels' own instantiations (the entries of TSDR_MIX3_LIST) in its mode
    for a in _mix3_entries():
        assert "k_fft_mix3<%d,%d,%d,%d,10>" % a in kernels["welch"], (a, kernels["welch"])
    assert "k_fft_mix" in kernels["welch"]


@pytest.mark.parametrize("cu", G.CU_COUNTS)
def test_frame_loop_case_reaches_the_direct_raster_kernel_past_its_grid(plan_dump, cu):
    p = G.params("raster-direct", cu)
    fmt = {"cf32": 0, "sc16": 1, "sc8": 2, "uc8": 3}[p["fmt"]]
    r = subprocess.run([plan_dump, "--one", str(fmt), "0", str(p["S"]), str(p["y_t"]), str(p["x_t"]), "1", "1", "1", str(cu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m = re.search(r"\| raster_direct_iq k_raster_direct<true> grid=(\d+),1,1 ", r.stdout)
    assert m and " status=0 raster=1 images=1 " in r.stdout, r.stdout
    work = G.cdiv(p["y_t"], 64) * 64 * p["x_t"]
    assert int(m.group(1)) == cu * G.BLOCKS_PER_CU < G.cdiv(work, G.BLOCK), (r.stdout, work)


# ---- the scan itself ---------------------------------------------------------------------------------------------------------------------
def test_the_scan_sees_a_new_launch_and_a_missing_entry(tmp_path):
    """what `Done when` asks to be tried by hand, kept: a copy of the sources with one more stream_grid launch fails the check, and
    so does the table without any one of its entries"""
    import shutil
    src = tmp_path / "csrc"
    shutil.copytree(CSRC, src)
    check_inventory(str(src))
    with open(src / "demod.hip", "a") as f:
        f.write('\nstatic int extra(tsdr_ctx *ctx, float *p, size_t m) {\n  TSDR_LAUNCH(ctx, "extra", k_extra, dim3(stream_grid(ctx, m * 2)), dim3(256), 0, p, m);\n  return 0;\n}\n')
    with pytest.raises(AssertionError, match=r"without an inventory entry[^$]*\('demod.hip', '\"extra\"', 'm \* 2'\)"):
        check_inventory(str(src))
    for i in range(len(G.SITES)):
        with pytest.raises(AssertionError, match="without an inventory entry"):
            check_inventory(CSRC, G.SITES[:i] + G.SITES[i + 1:])
    # a changed work-item expression makes the entry stale
    text = (src / "demod.hip").read_text().replace("extra", "extra2").replace('dim3(stream_grid(ctx, n)), dim3(256), 0, reinterpret_cast<const float2 *>(iq), n, out);',
                                                                            'dim3(stream_grid(ctx, n + 1)), dim3(256), 0, reinterpret_cast<const float2 *>(iq), n, out);')
    (src / "demod.hip").write_text(text)
    with pytest.raises(AssertionError):
        check_inventory(str(src))
