"""The FFT planner (csrc/fft_plan.h) against a record of what the library did before the planner existed.

tools/host_plan/fft_plan_dump_main.hip is built host-only (no GPU, a few seconds) and prints, for each case of its built-in list,
what plan_fft / plan_autocorr / plan_rows decide: status or error text, the WS_FFT_B bytes, and per step the profile name, the
kernel instantiation, grid, block, LDS bytes, the buffers read and written as roles, the tables needed and a hash over every
non-pointer field of the kernel's parameters (pointers count as set / not set; one exception: MixDesc::twg counts for strided
steps only -- no other kernel reads it, and the old running descriptor carried the previous pass's pointer into the last pass).  tests/golden/fft_plans_v1.txt holds the same
lines as made from commit b2315c9, where fft_pow2, fft_mixed_ex, fft_mixed_autocorr and the three fft_rows_* functions decided
all this while they launched: its launch macro was replaced by a recorder and those functions were driven with the same case
list (NOTEBOOK.md, "FFT plans", says how to make the file again after an intended planning change).  Equal lines mean: same
kernels, same launch shapes, same buffers and tables, same parameters, bit for bit.

What no 2^a 3^b 5^c length below 2^31 reaches, in the old code or the new (every one of the 1691 was planned, with "fft_big" on and
off, as a transform and as a fused autocorrelation), and so has no line:
  "fft: grid too large" of the power-of-two engine   a pass's grid is at most (points in all) / 512 -- a tile is R x T >= 512
                                                      points, the smallest being the 32 x 16 of a 512-point transform -- and
                                                      "fft: batch too large" has refused 2^40 points before
  k_fft_mix2<25,8>, <25,4>, <25,2> (both modes)       200, 100 and 50 are listed before them as 10 x 20, 10 x 10 and 10 x 5, and for
                                                      a size listed twice the first entry wins
  k_fft_pass<1..4, FFT_STRIDED>, <1..3, FFT_LAST>     the bits of a multi-pass length (2^9 and up) are dealt evenly: a strided pass
                                                      gets 5 .. 8 of them, a last pass 4 .. 8
  "fftm_strided6"                                     six passes are five strided ones and the last (MIX_MAX_PASS = 6)
The whole-row modes of k_fft_mix3 are recorded for every entry, each mode for at least one entry of either tile family, not for
every (entry, mode) pair: the mode moves nothing in the plan but the instantiation's last template argument.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fft_plans_v1.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_CASES = 600

PROFILE_NAMES = """fft_rows fft_strided1 fft_strided2 fft_strided3 fft_last fftm_rows fftm_strided1 fftm_strided2 fftm_strided3 fftm_strided4
fftm_strided5 fftm_last fftm_mid welch_rows_acc welch_rows_acc3 fft_rows3 waterfall_rows3""".split()
UNREACHABLE_NAMES = ["fftm_strided6"]                                                     # (module docstring)
UNREACHABLE_MIX2 = ["25,8", "25,4", "25,2"]
UNREACHABLE_PASS = [(1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (2, 1), (3, 1)]
ERROR_TEXTS = ["fft: unsupported power-of-two length 2^32", "fft_mixed: length 7000 is not 2^a*3^b*5^c", "fft: batch too large",
               "fft: fused loader / epilogue needs one multi-pass transform", "fft: fused loader needs one multi-pass transform",
               "fft: epilogue needs one multi-pass transform", "fft: too many rows", "fft: grid too large"]


def golden_lines():
    with open(GOLDEN) as f:
        return f.read().splitlines()


def parse(line):
    """-> (id, head, [(profile name, kernel, {grid, block, lds, hash}, "reads>writes", tables)])"""
    head, *steps = line.split(" | ")
    cid, *rest = head.split(" ")
    out = []
    for s in steps:
        name, kernel, *kv = s.split(" ")
        out.append((name, kernel, dict(x.split("=", 1) for x in kv if "=" in x), kv[3], kv[4]))
    return cid, " ".join(rest), out


def table_entries():
    """{family: [template arguments]} of the entry lists of fft_plan.h"""
    with open(os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "fft_plan.h")) as f:
        text = f.read().replace("\\\n", " ")
    out = {}
    for fam in ("MIX2", "MIX3", "WELCH3", "MID", "MID3"):
        body = re.search(r"#define TSDR_%s_LIST\(X\)(.*)" % fam, text).group(1)
        out[fam] = [re.sub(r"\s", "", a) for a in re.findall(r"X\(([^)]*)\)", re.sub(r"/\*.*?\*/", "", body))]
    return out


@pytest.fixture(scope="module")
def fft_plan_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_plan") / "fft_plan_dump")
    cmd = [HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "host_plan", "fft_plan_dump_main.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_plans_equal_the_record(fft_plan_dump):
    r = subprocess.run([fft_plan_dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, want = r.stdout.splitlines(), golden_lines()
    assert len(got) == len(want) <= MAX_CASES, (len(got), len(want))
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(want)} cases differ; the first:\n  got  {bad[0][0]}\n  want {bad[0][1]}"


def test_full_dump_of_one_case(fft_plan_dump):
    """--full ID: the line, then every field of every step's parameters"""
    r = subprocess.run([fft_plan_dump, "--full", "ac-mid-2000000-real"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] in golden_lines()
    assert lines[1].startswith("--- fftm_strided1 k_fft_mix3<") and any(x.startswith("R=2000 Bc=1000 ") for x in lines)
    assert subprocess.run([fft_plan_dump, "--full", "no-such-case"], capture_output=True).returncode == 1


def test_the_record_reaches_every_route():
    lines = golden_lines()
    assert len(lines) <= MAX_CASES and len({parse(x)[0] for x in lines}) == len(lines)
    assert max(len(x) for x in lines) < 1000
    steps = [s for x in lines for s in parse(x)[2]]
    names = {s[0] for s in steps}
    assert names == set(PROFILE_NAMES) and not names & set(UNREACHABLE_NAMES), names ^ set(PROFILE_NAMES)
    kernels = {s[1] for s in steps}
    T = table_entries()
    # every table entry a length can reach, the pass kernels in both modes
    want = {"k_fft_mix2<%s,%d>" % (a, m) for a in T["MIX2"] if a not in UNREACHABLE_MIX2 for m in (0, 1)}
    want |= {"k_fft_mix3<%s,%d>" % (a, m) for a in T["MIX3"] for m in (0, 1)}
    want |= {"k_fft_mid<%s>" % a for a in T["MID"]} | {"k_fft_mid3<%s>" % a for a in T["MID3"]}
    want |= {"k_fft_pass<%d,%d>" % (r, m) for r in range(1, 9) for m in (0, 1, 2) if (r, m) not in UNREACHABLE_PASS} | {"k_fft_mix"}
    assert want <= kernels, sorted(want - kernels)
    assert not {k for k in kernels if k.startswith(("k_fft_mix2<", "k_fft_pass<"))} - want
    # ... the whole-row modes: every entry of both tile families in some mode, every mode on some entry of either family
    for fam in ("MIX3", "WELCH3"):
        rows = {tuple(k[len("k_fft_mix3<"):-1].rsplit(",", 1)) for k in kernels if k.startswith("k_fft_mix3<") and int(k[:-1].rsplit(",", 1)[1]) >= 10}
        assert {a for a, _ in rows} >= set(T[fam]), set(T[fam]) - {a for a, _ in rows}
        assert {m for a, m in rows if a in T[fam]} == {"10", "11", "12", "13", "14", "15"}, fam
    # all three twiddle deliveries of the strided two-step kernel: sets in LDS (one, or 2 .. 4), the column table, per-output evaluation
    strided2 = [s for s in steps if s[1].startswith("k_fft_mix2<") and s[1].endswith(",0>")]
    assert any(s[4].startswith("twg(") for s in strided2)
    for a in ("10,10", "5,5"):   # (no table: the LDS bytes of one kernel differ by its twiddle sets alone -- 0 or 1, 2, 3, 4)
        assert len({s[2]["lds"] for s in strided2 if s[1] == "k_fft_mix2<%s,0>" % a and s[4] == "-"}) >= 2, a
    # one-pass rows of both engines, the one-point copy, a batch of 0, a length without a fused middle
    assert any(x.endswith(" copy") for x in lines)
    assert sum(bool(re.fullmatch(r"zero-batch-\w+ status=0 work=0", x)) for x in lines) == 2
    assert any(re.fullmatch(r"ac-mid-\d+-none status=0 work=0", x) for x in lines)
    bufs = {s[3] for s in steps}
    assert bufs == {"in>out", "in>work", "work>work", "work>out", "work>mid", "mid>mid", "mid>out", "in>-"}, bufs
    assert {t for s in steps for t in s[4].split("+") if not t.startswith("twg(")} == {"tw4096", "optin", "-"}
    errs = [re.search(r'err="(.*)"$', x).group(1) for x in lines if " status=0" not in x]
    for text in ERROR_TEXTS:
        assert text in errs, text
