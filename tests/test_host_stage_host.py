"""The staging path of the host-pointer entry points (csrc/host_stage.h) without a GPU.

tools/host_plan/host_stage_main.cpp is built as plain C++ (no HIP header, a few seconds) and drives the header's bookkeeping over
a back end that records: declaration order is enqueue order, the NULL and zero-byte rules, a failed slot growth enqueues nothing,
sub-ranges of a slot, the ninth entry, and the temporaries that have to outlive a wait that gave up (the same program under
ASan + UBSan: tools/asan_host_loop_policy.sh).  The sources are then searched: host <-> device copies are enqueued in
host_stage.h and nowhere else (group.hip and ring.hip keep their own pinning rules and DMA tickets).
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tempestsdr.jl_amd", "csrc")
HEADER = os.path.join(CSRC, "host_stage.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OWN_COPIES = {"host_stage.h", "group.hip", "ring.hip"}


def strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def calls(code, name):
    """the argument text of every call of `name` in `code`"""
    out = []
    for m in re.finditer(r"\b%s\s*\(" % name, code):
        depth, k = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(code[k], 0)
            k += 1
        out.append(code[m.end():k - 1])
    return out


@pytest.fixture(scope="module")
def host_stage(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_plan") / "host_stage")
    cmd = [HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tools", "host_plan", "host_stage_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_the_bookkeeping_holds(host_stage):
    r = subprocess.run([host_stage], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 expectation(s) failed" and not any("FAILED" in x for x in lines)
    assert len(lines) == 11, lines   # ten scenarios and the verdict


def test_the_bookkeeping_part_has_no_hip_in_it():
    """what comes before the context's back end includes standard headers and the C API's header only; a plain C++ compiler takes
    the whole file (the back end is compiled where common.h asks for it)"""
    text = open(HEADER).read()
    plain, marker, backend = text.partition("#ifdef TSDR_HOST_STAGE_WITH_CTX")
    assert marker and "hipMemcpyAsync" in backend
    includes = re.findall(r'^#include\s+(\S+)', text, re.M)
    assert includes and all(re.fullmatch(r"<[a-z]+>", i) or i == '"../../include/tempest_hip.h"' for i in includes), includes
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__device__|tsdr_ctx", strip_comments(plain))
    r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-fsyntax-only", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    common = strip_comments(open(os.path.join(CSRC, "common.h")).read())
    assert re.search(r'#define TSDR_HOST_STAGE_WITH_CTX\s*\n\s*#include "host_stage.h"', common) and "host_map" not in common


def test_host_device_copies_are_enqueued_by_the_stage_alone():
    seen = 0
    for f in sorted(os.listdir(CSRC)):
        code = strip_comments(open(os.path.join(CSRC, f)).read())
        for args in calls(code, "hipMemcpyAsync"):
            seen += 1
            if f not in OWN_COPIES:
                assert "hipMemcpyHostToDevice" not in args and "hipMemcpyDeviceToHost" not in args, (f, args)
                assert "hipMemcpyDeviceToDevice" in args, (f, args)   # (no copy kind hidden in a variable or hipMemcpyDefault)
    assert seen > 20
    stage = strip_comments(open(HEADER).read())
    kinds = [re.search(r"hipMemcpy(HostToDevice|DeviceToHost)", a).group(1) for a in calls(stage, "hipMemcpyAsync")]
    assert kinds == ["HostToDevice", "DeviceToHost"], kinds
    # the blocking table uploads of fft.hip / fft_mixed.hip are another matter and are not matched
    assert any("hipMemcpyHostToDevice" in a for a in calls(strip_comments(open(os.path.join(CSRC, "fft.hip")).read()), "hipMemcpy"))


def test_every_host_form_goes_through_the_stage():
    """the wrappers that used to write their own slot choice, copies and wait"""
    users = {"frames.hip": 1, "sync.hip": 2, "sync64.hip": 1, "raster_accum.hip": 1, "raster_register.hip": 1, "display.hip": 1,
             "fold_engine.h": 1, "raster_cstack.hip": 1, "ctx.hip": 3, "spectrum.hip": 3, "spectra64.hip": 2}
    for f, n in users.items():
        code = strip_comments(open(os.path.join(CSRC, f)).read())
        assert len(re.findall(r"\bHostStage \w+\(ctx\)", code)) == n, f
    for f in os.listdir(CSRC):   # ... and no wrapper sizes a staging slot by hand any more (the multi-device group stages per member)
        if f not in OWN_COPIES:
            assert not re.search(r"scratch\(WS_(IN|OUT|AUX)\b", strip_comments(open(os.path.join(CSRC, f)).read())), f
