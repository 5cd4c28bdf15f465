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
and a third one guards the set of k_raster_fast instantiations that the planner may name and the launcher builds
(image_plan.h:fast_instance):
  "raster: the tile plan names a kernel that is not built"   the step's template arguments fail fast_instance, whose rules are
                                                  the planner's own conditions; test_planner_and_table_name_the_same_kernels
                                                  sweeps for a counterexample

That set is held from three sides: `plan_dump --table` prints it, `plan_dump --reach` prints what a sweep over plan_images met,
and the device code of resample.hip is compiled and its kernel symbols are read.  All three must be the same list.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_plans_v1.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_CASES = 640

PROFILE_NAMES = """raster_down_iq raster_iq down_walk_iq raster_down_iq_exact raster_down_f32_exact raster_iq_exact raster_f32_exact
raster_direct_iq raster_direct_f32 down_fused_iq down_fused_iq_sums down_fused_iq_exact down_fused_f32_exact raster_sheared_iq
raster_unsheared_iq resize2d""".split()
ERROR_TEXTS = ["y_t and x_t must be positive", "frame larger than 2^31 samples/pixels", "imresize needs at least 2 input samples",
               "output size must be positive", "imresize needs at least a 2x2 raster",
               "raster: too many tiles for one launch (split the buffer)"]
UNREACHABLE = ["raster: candidate table overflow", "raster: tile plan needs the f32-sample walk",
               "raster: the tile plan names a kernel that is not built"]   # (module docstring)
# k_raster_fast instantiations that fast_instance admits and the sweep of `plan_dump --reach` does not meet: {name: why it stays}.
# At most 8; none so far.
TABLE_NOT_REACHED = {}


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



def _lines(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.split()


def test_planner_and_table_name_the_same_kernels(plan_dump):
    table = _lines(plan_dump, "--table")
    reach = _lines(plan_dump, "--reach")
    assert table == sorted(set(table)) and reach == sorted(set(reach))
    walks = {x for x in reach if x.startswith("k_raster_fast<")}
    assert set(table) and all(x.startswith("k_raster_fast<") for x in table)
    assert not walks - set(table), "the planner names kernels the launcher lacks"
    assert len(TABLE_NOT_REACHED) <= 8 and set(TABLE_NOT_REACHED) <= set(table)
    assert set(table) - walks == set(TABLE_NOT_REACHED), "the launcher builds kernels no plan of the sweep names"
    # the record's own steps lie in the table too, the gpu-inst-* cases of tests/test_raster_instances_gpu.py among them
    recorded = {s[1] for x in golden_lines() for s in parse(x)[2] if s[1].startswith("k_raster_fast<")}
    assert recorded <= set(table)
    # the tap kernel has no table: the sweep meets every one of its 34 instantiations (2 EXACT: IQ and real input; FAST: fixed-point
    # or f64 taps x sums or not x 4 or 16 loads in flight x four input formats), so resample.hip:launch_down has nothing to drop
    assert len([x for x in reach if x.startswith("k_down_fused<")]) == 34


def test_the_code_object_holds_exactly_the_table(plan_dump, tmp_path):
    """resample.hip compiled for the device alone, with the library's flags (about 40 s): its k_raster_fast symbols are the table"""
    import importlib.util
    import shutil
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if filt is None:
        pytest.skip("no demangler (c++filt, llvm-cxxfilt) on this machine")
    spec = importlib.util.spec_from_file_location("tsdr_build_flags", os.path.join(ROOT, "tempestsdr.jl_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    elf = str(tmp_path / "resample.elf")
    r = subprocess.run([HIPCC] + build.FLAGS + ["-w", "--cuda-device-only", "--no-gpu-bundle-output", "-c",
                        os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "resample.hip"), "-o", elf], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # kernel descriptors: one 64-byte object `<kernel symbol>.kd` per kernel, in the ELF's symbol table
    data = open(elf, "rb").read()
    syms = sorted({m.group(1).decode() for m in re.finditer(rb"(_Z[A-Za-z0-9_]+)\.kd\0", data)})
    assert syms
    r = subprocess.run([filt], input="\n".join(syms), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    built = {re.sub(r"\(.*$", "", x).replace("void tsdr::", "").replace(" ", "") for x in r.stdout.splitlines()}
    walks = {x for x in built if x.startswith("k_raster_fast<")}
    table = set(_lines(plan_dump, "--table"))
    assert walks == table, (sorted(walks - table)[:4], sorted(table - walks)[:4])
    assert len([x for x in built if x.startswith("k_down_fused<")]) == 34
