# Measures the display export (include/tempest_hip_display.h, tsdr_display_u8_d) on resident buffers, everything in one process,
# variants alternating so that drift hits them alike:
#   geometries   30 x 600x800 (a C2 buffer's frames_out), one 1125x2576 state, one 2250x4400 state
#   modes        FIXED, MINMAX, PERCENTILE (0.01, 0.99), each on the full picture and on an 80 % centred ROI
#   same address PERCENTILE on a constant picture with one outlier -- every lane of the histogram pass on one LDS counter -- with
#                the option "display_hist_agg" at 0 and at 1, beside the same call on an ordinary picture
#   split        the per-kernel times of one PERCENTILE call (profiling event pairs, a block of its own)
# Per variant: ms per call, the bytes of the header's cost model (FIXED 4R + R, MINMAX 8R + R, PERCENTILE 12R + R per picture), and
# those bytes over the time as a fraction of 8 TB/s.  Times are HIP events (tsdr_timer_*) around blocks of back-to-back calls, at
# least 0.3 s of calls per variant in all, after a warm-up of every shape; medians over the blocks.
#
#     python tools/time_display.py [out.json = profiles/display_u8.json]
#
# Prints one JSON document and writes it to out.json.  GPU box only.
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tempest_loader import load_package  # noqa: E402

T = load_package()
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "display_u8.json")
GEOMS = {"30x600x800": (30, 600, 800), "1x1125x2576": (1, 1125, 2576), "1x2250x4400": (1, 2250, 4400)}
MODES = {"fixed": 5, "minmax": 9, "percentile": 13}     # bytes per ROI pixel in the cost model: reads + the byte written
P = (0.01, 0.99)
PEAK = 8.0e12
MIN_SECONDS, ROUNDS = 0.3, 5

ctx = T.Context()
res = {"device": ctx.device_info()["name"], "rounds": ROUNDS, "min_seconds_per_variant": MIN_SECONDS, "peak_bytes_per_s": PEAK,
       "percentiles": list(P), "geometries": {}}


def timed_blocks(variants, reps):
    out = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            ctx.timer_start()
            for _ in range(reps[name]):
                fn()
            out[name].append(ctx.timer_stop() / reps[name])
    return out


def reps_for(fn, lo=3):
    for _ in range(lo):
        fn()
    ctx.timer_start()
    for _ in range(lo):
        fn()
    ms = max(ctx.timer_stop() / lo, 1e-3)
    return max(lo, int(np.ceil(MIN_SECONDS * 1e3 / ms / ROUNDS)))


def summary(blocks, nbytes):
    med = statistics.median(blocks)
    return {"ms_blocks": [round(b, 5) for b in blocks], "ms_median": round(med, 5), "ms_min": round(min(blocks), 5), "ms_max": round(max(blocks), 5),
            "model_bytes": nbytes, "fraction_of_8TBps": round(nbytes / (med * 1e-3) / PEAK, 4)}


def centred(h, w):
    rh, rw = int(0.8 * h), int(0.8 * w)
    return ((h - rh) // 2, (w - rw) // 2, rh, rw)


for gname, (n, h, w) in GEOMS.items():
    rng = np.random.default_rng(h + w)
    pics = np.abs(rng.normal(2.0, 1.0, (n, h * w))).astype(np.float32)
    const = np.full((n, h * w), 3.0, np.float32)
    const[:, 17] = 1000.0
    d_pics, d_const = ctx.upload(pics), ctx.upload(const)
    d_out, d_rng = ctx.dev_alloc(n * h * w), ctx.dev_alloc(8 * n)
    rois = {"full": (0, 0, h, w), "roi80": centred(h, w)}
    doc = {"n": n, "h": h, "w": w, "rois": {k: list(v) for k, v in rois.items()}, "calls": {}}

    def call(d_in, roi, mode):
        return lambda: ctx.display_u8_d(d_in, n, h, w, d_out, roi, mode, 0.0, 6.0, P, ranges_out=d_rng)

    variants, nbytes = {}, {}
    for rname, roi in rois.items():
        for mode, per_px in MODES.items():
            variants[f"{mode} {rname}"] = call(d_pics, roi, mode)
            nbytes[f"{mode} {rname}"] = per_px * n * roi[2] * roi[3]
    reps = {k: reps_for(f) for k, f in variants.items()}
    for name, blocks in timed_blocks(variants, reps).items():
        doc["calls"][name] = dict(summary(blocks, nbytes[name]), reps_per_block=reps[name])

    # every lane on one LDS counter: a constant picture with one outlier, beside the ordinary picture, both forms of the pass
    def with_agg(agg, fn):
        def run():
            ctx.set_option("display_hist_agg", agg)
            try:
                fn()
            finally:
                ctx.set_option("display_hist_agg", 0)
        return run

    full = rois["full"]
    same = {f"{what} agg={agg}": with_agg(agg, call(d_in, full, "percentile")) for what, d_in in (("ordinary", d_pics), ("constant+outlier", d_const))
            for agg in (0, 1)}
    reps = {k: reps_for(f) for k, f in same.items()}
    doc["same_address"] = {name: dict(summary(blocks, 13 * n * h * w), reps_per_block=reps[name]) for name, blocks in timed_blocks(same, reps).items()}
    # per-kernel split of a PERCENTILE call, in blocks of their own (the event pairs slow the stream down)
    doc["kernels_us_per_percentile_call"] = {}
    for what, fn in (("ordinary agg=0", same["ordinary agg=0"]), ("constant+outlier agg=0", same["constant+outlier agg=0"]),
                     ("constant+outlier agg=1", same["constant+outlier agg=1"])):
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(10):
            fn()
        ctx.synchronize()
        doc["kernels_us_per_percentile_call"][what] = {k: round(v["total_ms"] / 10 * 1e3, 2) for k, v in sorted(ctx.profile_results().items())}
        ctx.profile(False)
    ctx.synchronize()
    for p in (d_pics, d_const, d_out, d_rng):
        ctx.dev_free(p)
    res["geometries"][gname] = doc

text = json.dumps(res, indent=1)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text + "\n")
