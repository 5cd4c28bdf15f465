"""Development aid (GPU box): the frame loop at the C2 geometry under both polarities of "vsync_blank_dark", for one
rocprofv3 --kernel-trace --stats run of its own (k_beta<4, false> / k_beta<4, true> appear as two kernels), and the step
time of each by host clock.

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_beta_polarity.py [steps]

Polarity 0 runs on the "box" leak, polarity 1 on "box_dark": each on the card it is meant for.  One buffer = 30 frames."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from tempest_loader import load_package

T = load_package()
api = importlib.import_module("tempestsdr_jl_amd.api")
synth = importlib.import_module("tempestsdr_jl_amd.synth")


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    w = synth.WORKLOADS["C2"]
    Fs, x_t, y_t, fv = w["Fs"], w["x_t"], w["y_t"], w["fv"]
    S, nfr, npx = synth.samples_per_frame(Fs, fv), 30, 600 * 800
    ctx = T.Context()
    for dark, card in ((0, "box"), (1, "box_dark")):
        iq = synth.synth_leak(Fs, x_t, y_t, fv, S * nfr, card=card)
        d_iq, d_state, d_ix = ctx.upload(iq.view(np.float32)), ctx.upload(np.zeros(npx, np.float32)), ctx.dev_alloc(nfr * 8)
        sync = T.SyncXY(ctx, 600, 800)
        ctx.set_option("vsync_blank_dark", dark)
        try:
            for k in range(5 + steps):
                if k == 5:
                    ctx.synchronize()
                    t0 = time.perf_counter()
                api.frames_d(ctx, sync, d_iq, iq.size, S, y_t, x_t, np.float32(0.1), True, d_state, None, None, d_ix)
            ctx.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            idx = ctx.download(d_ix, (nfr, 2), np.int32)
            print(f"vsync_blank_dark={dark} card={card}: {ms:.4f} ms per 30-frame buffer (raster-free), guard {ctx.sync_guard_stats(reset=True)}, "
                  f"first indices {idx[:3].tolist()}")
        finally:
            ctx.set_option("vsync_blank_dark", 0)
            sync.close()
            for p in (d_iq, d_state, d_ix):
                ctx.dev_free(p)


if __name__ == "__main__":
    main()
