"""The pipeline's lane bookkeeping (csrc/loop_policy.h: LaneBusy -- which internal streams a host wait has to touch -- and
overlap_allowed, the rule of option "frames_overlap") on the host: tools/host_plan/lane_busy_main.cpp replays the transitions
frames.hip and ctx.hip make, scenario by scenario, and checks its own expectations.  No GPU; a few seconds to build."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_lane_busy_scenarios(tmp_path):
    exe = str(tmp_path / "lane_busy")
    r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "host_plan", "lane_busy_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("0 expectation(s) failed"), r.stdout + r.stderr
    assert r.stdout.count("\n") >= 11
