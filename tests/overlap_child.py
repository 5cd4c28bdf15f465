"""Child of tests/test_frames_overlap_gpu.py:test_default_option_in_a_process_of_its_own: a fresh process that holds exactly ONE
Context, touches no module-level wrapper (they would open a context of their own) and leaves "frames_overlap" at its default of 1
-- the configuration every single-context caller runs, which a test session with its shared contexts never reaches.
  * six "small" buffers through tsdr_frames_d: all six on the lanes;
  * a second context is opened, one more call: sequential, why = 1 (the device is shared);
  * the second context is closed, one more call: on the lanes again;
  * the same eight calls with "frames_overlap" 0 in this process: frames, sync indices, IIR state, guard counters bit for bit.
Prints one JSON line; exit status 0 = everything held."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NPX, NFR, NBUF = 600 * 800, 3, 6
GEO = dict(Fs=300000.0, x_t=300, y_t=200, fv=50.0)   # "small" of tests/test_frames_overlap_gpu.py


def main():
    import importlib

    import torch
    from tempest_loader import load_package
    tsdr = load_package()
    api = importlib.import_module("tempestsdr_jl_amd.api")
    synth = importlib.import_module("tempestsdr_jl_amd.synth")
    S = synth.samples_per_frame(GEO["Fs"], GEO["fv"])
    n = S * NFR + 5
    iqs = [torch.from_numpy(synth.synth_leak(GEO["Fs"], GEO["x_t"], GEO["y_t"], GEO["fv"], n, n0=b * n).view(np.float32)).to("cuda:0")
           for b in range(NBUF)]
    ctx = tsdr.Context(0)
    out = {}

    def eight(option):
        """six calls, one beside a second context, one after it has gone -> everything the calls left, and the stats on the way"""
        outs = [(torch.zeros(NFR * NPX, dtype=torch.float32, device="cuda:0"), torch.zeros(2 * NFR, dtype=torch.int32, device="cuda:0"))
                for _ in range(NBUF + 2)]
        state = torch.zeros(NPX, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        sync = tsdr.SyncXY(ctx, 600, 800)
        if option is not None:
            ctx.set_option("frames_overlap", option)
        ctx.set_option("sync_guard_ppb", 20000)   # (restarts the adaptive route's window: both passes start from the same history)
        ctx.sync_guard_stats(reset=True)
        ctx.frames_overlap_stats(reset=True)
        stats = {}

        def call(k):
            fo, si = outs[k]
            assert api.frames_d(ctx, sync, iqs[k % NBUF], n, S, GEO["y_t"], GEO["x_t"], np.float32(0.1), True, state, fo, None, si) == NFR

        for k in range(NBUF):
            call(k)
        stats["alone"] = list(ctx.frames_overlap_stats())
        other = tsdr.Context(0)
        try:
            call(NBUF)
            stats["second_context"] = list(ctx.frames_overlap_stats())
        finally:
            other.close()
        call(NBUF + 1)
        stats["alone_again"] = list(ctx.frames_overlap_stats())
        ctx.synchronize()
        res = [state.clone()] + [t.clone() for o in outs for t in o]
        guard = list(ctx.sync_guard_stats())
        sync.close()
        return res, guard, stats

    got, guard, stats = eight(None)            # the default: nothing sets the option
    want, guard0, stats0 = eight(0)
    out.update(stats)
    out["option_0"] = stats0["alone_again"]
    out["guard"] = guard
    out["equal"] = guard == guard0 and len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    out["wait_stats"] = list(ctx.wait_stats())
    ctx.close()
    ok = (out["equal"] and out["alone"] == [NBUF, 0, 0] and out["second_context"] == [NBUF, 1, 1] and out["alone_again"] == [NBUF + 1, 1, 1]
          and out["option_0"] == [0, NBUF + 2, 1] and out["wait_stats"] == [0, 0])
    print(json.dumps(out), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
