"""The image planner (csrc/image_plan.h) against a record of what the library did before the planner existed.

tools/host_plan/plan_dump_main.hip is built host-only (no GPU, a few seconds) and prints, for each case of its built-in list,
what plan_images decides: status, what is produced, and per step the profile name, the kernel instantiation, grid, block, LDS
bytes and a hash over every field of the kernel's parameters.  tests/golden/image_plans_v1.txt holds the same lines as made
from commit 9995fb2, where raster_and_down_d / raster_frames_d / down_frames_d / raster_shear_d decided all this while they
launched: its launch macro was replaced by a recorder and the four functions were driven with the same case list (NOTEBOOK.md,
"image plans", says how to make the file again after an intended planning change).  Equal lines mean: same kernels, same
launch shapes, same parameters, bit for bit.

Two error texts of the planner cannot be reached by any input, in the old code or the new, and so have no line:
  "raster: candidate table overflow"             needs more than 128 candidate rows (192 columns) per 64-line (TP-pixel) tile,
                                                  i.e. a ratio below 0.52 (0.35) on an axis; the fused downgrade is only planned
                                                  for ratios >= 1, where there are at most 69 of either
  "raster: tile plan needs the f32-sample walk"  guards a tile wider than 47 samples without the f32-sample walk; the tile
                                                  search falls back to the 47-sample budget exactly when that walk is not planned
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_plans_v1.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_CASES = 600

PROFILE_NAMES = """raster_down_iq raster_iq down_walk_iq raster_down_iq_exact raster_down_f32_exact raster_iq_exact raster_f32_exact
raster_direct_iq raster_direct_f32 down_fused_iq down_fused_iq_sums down_fused_iq_exact down_fused_f32_exact raster_sheared_iq
raster_unsheared_iq resize2d""".split()
ERROR_TEXTS = ["y_t and x_t must be positive", "frame larger than 2^31 samples/pixels", "imresize needs at least 2 input samples",
               "output size must be positive", "imresize needs at least a 2x2 raster",
               "raster: too many tiles for one launch (split the buffer)"]
UNREACHABLE = ["raster: candidate table overflow", "raster: tile plan needs the f32-sample walk"]   # (module docstring)


def golden_lines():
    with open(GOLDEN) as f:
        return f.read().splitlines()


def parse(line):
    """-> (id, head fields, [(profile name, kernel, fields)])"""
    head, *steps = line.split(" | ")
    cid, *rest = head.split(" ")
    out = []
    for s in steps:
        name, kernel, *kv = s.split(" ")
        out.append((name, kernel, dict(x.split("=", 1) for x in kv)))
    return cid, " ".join(rest), out


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_plan") / "plan_dump")
    cmd = [HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "host_plan", "plan_dump_main.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_plans_equal_the_record(plan_dump):
    r = subprocess.run([plan_dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, want = r.stdout.splitlines(), golden_lines()
    assert len(got) == len(want) <= MAX_CASES, (len(got), len(want))
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(want)} cases differ; the first:\n  got  {bad[0][0]}\n  want {bad[0][1]}"


def test_full_dump_of_one_case(plan_dump):
    """--full ID: the line, then every field of every step's parameters"""
    r = subprocess.run([plan_dump, "--full", "wl-C2-ras-fast-cf32-sums"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] in golden_lines()
    assert lines[1].startswith("--- raster_down_iq k_raster_fast<") and any(x.startswith("fi.qL=") for x in lines)
    assert subprocess.run([plan_dump, "--full", "no-such-case"], capture_output=True).returncode == 1


def test_the_record_reaches_every_route():
    lines = golden_lines()
    assert len(lines) <= MAX_CASES and len({parse(x)[0] for x in lines}) == len(lines)
    steps = [s for x in lines for s in parse(x)[2]]
    names = {s[0] for s in steps}
    assert names == set(PROFILE_NAMES), (names ^ set(PROFILE_NAMES))
    assert any(" fallback ws_raster=" in x for x in lines)
    # the walk's position advance: 32-bit (f32 walk) and 64-bit
    walks = {re.match(r"k_raster_fast<true,(true|false),", s[1]).group(1) for s in steps if s[1].startswith("k_raster_fast<")}
    assert walks == {"true", "false"}
    taps = [s[2] for s in steps if s[1].startswith("k_down_fused<")]
    assert {t["sparse"] for t in taps} == {"0", "1"} and {t["ld16"] for t in taps} == {"0", "1"}
    assert any(s[1].startswith("k_down_fused<") and s[1].split(",")[3] == "16" for s in steps)   # ... and its LD = 16 kernels
    assert {int(s[2]["TP"]) for s in steps if "TP" in s[2]} == {128, 64, 32, 16, 8, 4}
    assert {s[1] for s in steps if s[1].startswith("k_raster_fast4<")} == {"k_raster_fast4<0,16>", "k_raster_fast4<1,16>", "k_raster_fast4<0,32>",
                                                                           "k_raster_fast4<1,32>"}
    errs = [re.search(r'err="(.*)"$', x).group(1) for x in lines if " status=0" not in x]
    for text in ERROR_TEXTS:
        assert text in errs, text
    for text in UNREACHABLE:
        assert text not in errs

