"""The frame loop's host-side policy (csrc/loop_policy.h: PipeTuner, GuardRoute) against a record of what the library did
before that header existed.

tools/host_plan/loop_policy_main.cpp is built host-only (no GPU, a few seconds) and replays the scenario list of
tools/host_plan/loop_policy_scenarios.h: histories of submissions, options, scripted trial boundaries (did the waits succeed,
what did the timer read) and guard ring entries.  One line per step: the event; the arrangement of every submission, run-length
coded; before which submissions the pipeline was run empty for a trial boundary; which timing events were recorded; and the
whole of tsdr_frames_pipeline_info afterwards (floats as their bits), or the guard route's counters.
tests/golden/loop_policy_v1.txt holds the same lines as made from commit 001972f, where frames.hip:pipe_pick, the trial
bookkeeping of frames_submit, tsdr_frames_pipeline_info, tsdr_set_option's branches and the fold inside guard_auto_update did
all this: those bodies, unchanged, were compiled against a stub context whose drain, lane wait and elapsed time were scripted,
and driven by the same scenario list (NOTEBOOK.md, "loop policy", says how to make the file again after an intended change).
"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loop_policy_v1.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_LINES = 600
SEQ, TAKEN = "one stream (sequential order)", "taken over from a neighbouring configuration's measurement: "


def golden_lines():
    with open(GOLDEN) as f:
        return f.read().splitlines()


def parse(line):
    """-> (scenario, step, event, {what happened}, state text)"""
    head, what, state = line.split(" | ", 2)
    sid, event = head.split(" ", 1)
    scenario, step = sid.rsplit(".", 1)
    return scenario, int(step), event, dict(x.split("=", 1) for x in what.split(" ") if "=" in x), state


def info(state):
    """-> trials_left, chosen, [ms bits], text"""
    m = re.match(r'info=(-?\d+),(-?\d+),\[([0-9a-f ]+)\],"(.*?)"(?: guard=.*)?$', state)
    return int(m.group(1)), int(m.group(2)), m.group(3).split(), m.group(4)


def runs(state):
    return int(re.search(r"measurements started on this context: (\d+)\)", state).group(1))


def guard(state):
    return tuple(int(x) for x in re.search(r"guard=(\d+),(\d+),(\d+),(\d+),(\d+)$", state).groups())


def f32(num, den=1.0):
    """the bits of the float quotient, as the record prints them"""
    return "%08x" % (np.float32(num) / np.float32(den)).view(np.uint32)


def arrangements(what):
    """the run-length coded arrangements of a submit step -> [(arrangement, count)]"""
    return [tuple(int(v) for v in x.split("x")) for x in what["arr"].split(",") if x]


@pytest.fixture(scope="module")
def loop_policy(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_plan") / "loop_policy")
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
           os.path.join(ROOT, "tools", "host_plan", "loop_policy_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_policy_equals_the_record(loop_policy):
    r = subprocess.run([loop_policy], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, want = r.stdout.splitlines(), golden_lines()
    assert len(got) == len(want) <= MAX_LINES, (len(got), len(want))
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(want)} steps differ; the first:\n  got  {bad[0][0]}\n  want {bad[0][1]}"


def test_one_scenario(loop_policy):
    r = subprocess.run([loop_policy, "guard"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == [x for x in golden_lines() if x.startswith("guard.")]
    assert subprocess.run([loop_policy, "no-such-scenario"], capture_output=True).returncode == 1


def test_the_header_has_no_hip_in_it():
    """loop_policy.h includes standard headers only, and a plain C++ compiler takes it (the fixture's build is hipcc's host pass)"""
    path = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc", "loop_policy.h")
    with open(path) as f:
        includes = re.findall(r'^#include\s+(\S+)', f.read(), re.M)
    assert includes and all(re.fullmatch(r"<[a-z]+>", i) for i in includes), includes
    r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-fsyntax-only", path], capture_output=True, text=True)   # (as plain C++: no HIP header)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_record_reaches_every_route():
    lines = golden_lines()
    steps = [parse(x) for x in lines]
    assert len(lines) <= MAX_LINES and len({(s[0], s[1]) for s in steps}) == len(lines)
    by = {}
    for s in steps:
        by.setdefault(s[0], []).append(s)

    # ---- a full measurement
    full = by["full"]
    used = [a for s in full for a, _ in arrangements(s[3])]
    assert set(used) == set(range(8))
    ms_seen = {b for s in full for b in info(s[4])[2]}
    assert f32(96.0, 12) not in ms_seen                                   # the warm-up value is discarded
    p1, last = info(full[10][4])[2], info(full[-1][4])
    assert info(full[10][4])[0] == 8 and "00000000" not in p1              # after the first pass
    assert last[0] == 0 and last[1] == 3 and last[3].startswith("measured: ")
    assert int(last[2][3], 16) < int(p1[3], 16) and last[2][4] == p1[4] == f32(10.875, 12)   # pass 2: better is taken, worse is not
    assert last[2][3] == last[2][7] == min(last[2])                        # a tie: the lower index (positive floats order as their bits)
    assert [info(s[4])[0] for s in full[2:19]] == list(range(16, -1, -1))  # trials_left counts the 17 trials down
    assert full[2][3]["quiesce"] == "1" and full[2][3]["timed"] == "3:2,15:14"
    assert info(by["rule-below"][-1][4])[1] == 5 and info(by["rule-below"][-1][4])[2][5] == f32(11.8125, 12)
    assert info(by["rule-above"][-1][4])[1] == 0 and info(by["rule-above"][-1][4])[2][5] == f32(11.828125, 12)
    some = info(by["timer-some"][-1][4])[2]
    assert some[2] == f32(11.5, 12) and some[3] == f32(11.0, 12) and some[6] == f32(1e30)   # pass 1 only, pass 2 only, both
    every = info(by["timer-all"][-1][4])
    assert set(every[2]) == {f32(1e30)} and every[1] == 0 and every[3].startswith("measured: " + SEQ)
    # ---- a wait that fails once at a trial boundary
    wf = by["wait-fails"]
    assert wf[1][3]["failed"] == "1:-4" and wf[1][3]["quiesce"] == "1" and wf[1][4] == wf[0][4]   # the tuner is unchanged
    assert wf[2][3]["failed"] == "" and wf[2][3]["quiesce"] == "1" and info(wf[2][4])[0] == 16
    assert wf[4][3]["failed"] == "1:-4" and info(wf[4][4])[2][0] == f32(9.0, 12)
    # ---- configuration changes
    ls = by["leave-settled"]
    assert info(ls[0][4])[1] == 4 and info(ls[1][4])[0] == 16 and info(ls[2][4])[:2] == (0, 4) and ls[2][3]["quiesce"] == ""
    assert runs(ls[2][4]) == 2 and ls[3][3]["timed"] == "3:2" and runs(ls[3][4]) == 2          # K1's trial: again from its first buffer
    lm = by["leave-mid-trial"]
    assert arrangements(lm[0][3])[-1] == (2, 7) and arrangements(lm[2][3]) == [(2, 14)] and lm[2][3]["timed"] == "3:2"
    assert lm[3][3]["quiesce"] == "2" and arrangements(lm[3][3]) == [(2, 1), (3, 1)]
    al = by["alternation"]
    assert [info(s[4])[0] for s in al[:8]] == [17] * 8 and [info(s[4])[:2] for s in al[8:10]] == [(0, 0), (0, 0)]   # four interruptions each
    assert all(s[3]["quiesce"] == "" for s in al)
    ev = by["eviction"]
    assert [runs(s[4]) for s in ev] == list(range(1, 11)) + [11, 12, 12, 13]   # the first and the third again, the tenth not, the fourth again
    assert info(ev[12][4])[3].startswith("measured: ")
    nb = by["neighbour"]
    assert info(nb[1][4])[3].startswith(TAKEN) and info(nb[1][4])[1] == 3 and runs(nb[1][4]) == 1 and nb[1][3]["quiesce"] == ""
    assert info(nb[2][4])[3].startswith("measured: ")
    two = by["two-neighbours"]
    assert info(two[0][4])[1] == 3 and info(two[2][4])[1] == 5 and info(two[2][4])[3].startswith("measured: ") and runs(two[2][4]) == 2
    assert info(two[4][4])[1] == 5 and info(two[4][4])[3].startswith(TAKEN)                    # the most recent of the two
    un = by["unsettled-neighbour"]
    assert info(un[1][4])[0] == 17 and runs(un[1][4]) == 2 and info(un[2][4])[0] == 16 and runs(un[2][4]) == 2
    nbd = by["near-bounds"]
    assert [s[2].split(" ")[1] for s in nbd] == ["S9000", "S11000", "S10000", "S9999", "S10001", "P900000", "P1100000", "P1000000", "P999000",
                                                 "P1001000"]
    assert [info(s[4])[3].startswith(TAKEN) for s in nbd] == [False, False, False, True, True, False, False, False, True, True]
    assert [runs(s[4]) for s in nbd] == [1, 2, 3, 3, 3, 4, 5, 6, 6, 6]
    nn = by["not-near"]
    assert [s[2].split(" ")[1] for s in nn[1:6]] == ["raster", "precision", "alignment", "iq-kind", "frames"]
    assert [runs(s[4]) for s in nn] == [1, 2, 3, 4, 5, 6, 6, 6] and info(nn[6][4])[3].startswith(TAKEN)
    # ---- options
    pin = by["pin"]
    pinned = [(int(s[2].split(" ")[2]), pin[i + 1]) for i, s in enumerate(pin) if s[2].startswith("option pipe_pin") and s[3]["rc"] == "0"
              and int(s[2].split(" ")[2]) >= 0]
    assert [p for p, _ in pinned] == list(range(8)) + [3]
    for p, nxt in pinned:
        assert arrangements(nxt[3]) == [(p, 2)] and nxt[3]["quiesce"] == nxt[3]["timed"] == "" and info(nxt[4])[3].startswith("pinned (\"pipe_pin\"): ")
    assert [s[3]["rc"] for s in pin if s[2] == "option pipe_pin 8"] == ["-1"]
    assert pin[-1][3]["quiesce"] == "1" and info(pin[-1][4])[0] == 15 and runs(pin[-1][4]) == 1   # back to -1: the measurement goes on
    mode = {s[2]: arrangements(mode_next[3]) for s, mode_next in zip(by["mode"], by["mode"][1:]) if s[2].startswith("option")}
    assert mode == {"option pipe_mode 0": [(1, 2)], "option pipe_priority 0": [(2, 2)], "option pipe_priority 7": [(1, 2)],
                    "option pipe_mode 1": [(4, 2)], "option pipe_lanes 3": [(7, 2)], "option pipe_lanes 4": [(4, 2)],
                    "option pipe_mode 2": [(0, 2)], "option pipe_mode 9": [(0, 2)], "option pipe_mode -3": [(0, 2)]}
    assert info(by["mode"][1][4])[3].startswith("forced: image lane + high-priority tail lane")
    to = by["tune-off"]
    assert arrangements(to[2][3]) == [(1, 2)] and arrangements(to[3][3]) == [(4, 2)] and info(to[3][4])[2] == ["00000000"] * 8
    assert info(to[5][4])[0] == 17 and runs(to[0][4]) == 1 and runs(to[5][4]) == 2              # nothing remembered, the counter kept
    mn = by["measure-now"]
    assert [runs(s[4]) for s in mn] == [0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 4, 4, 5]
    assert info(mn[3][4])[0] == 16 and info(mn[5][4])[0] == 17 and info(mn[7][4])[0] == 0 and info(mn[9][4])[0] == 17
    # ---- the guard's route
    g = [(s[2], s[3], guard(s[4])) for s in by["guard"]]
    closes = [(int(w["frames"]), before[0] + int(w["frames"])) for (e, w, now), (_, _, before) in zip(g[1:], g) if e.startswith("entry") and now[:2] == (0, 0)]
    assert any(total == 60 for _, total in closes) and any(total > 60 for _, total in closes)
    assert g[1][2] == (0, 0, 0, 0, 0)                                      # 9 of 60 stays
    assert g[5][2][2:4] == (1, 1) and (g[3][2][1] + 4, g[4][2][0] + 15) == (7, 65)
    assert g[7][2][2:4] == (1, 1) and g[10][2][2:4] == (0, 2)              # 3 of 60 stays, 2 of 60 goes back
    off = [i for i, x in enumerate(g) if x[0] == "option sync_guard_auto 0"][0]
    assert g[off - 1][2][:3] == (30, 30, 1) and g[off][2][:3] == (30, 30, 0) and g[off + 2][2] == g[off][2]
    ppb = [i for i, x in enumerate(g) if x[0].startswith("option sync_guard_ppb")]
    assert [g[i - 1][2][:3] for i in ppb] == [(40, 40, 1), (59, 59, 0)] and all(g[i][2][:3] == (0, 0, 0) for i in ppb)
    assert g[-2][2][3:] == (6, 7) and "".join(w["route"] for e, w, _ in g if e.startswith("buffers")) == "FFEEEEFFEEFE"
    assert g[-2][1] == {"tag": "65535", "frames": "16777215", "flagged": "0"}
