# Measures the full-resolution frame average (include/tempest_hip_hires.h) at the C2 and C5 workloads of SURVEY.md (30 frames per
# buffer: 2576x1125 at 20 MS/s, 4400x2250 at 50 MS/s), everything in one process, variants alternating so that drift hits them alike:
#   (a) raster_accum alone: us per launch over the 30 rasters of a buffer, with shifts (image units) and without; the bytes the
#       algorithm needs, n*4P + 8P, over that time; its share of the 8 TB/s HBM peak
#   (b) tsdr_frames_hires_iq_d per buffer against tsdr_frames_iq_d with raster_out on the same buffer: the cost the feature adds
#       over rasters the library could already produce
#   (c) the default (the whole buffer in one chunk) against "hires_chunk_frames" = the most frames whose rasters stay at or under
#       192 MiB, the rule that was meant to keep a chunk's rasters in the Infinity Cache between the two stages
# Times are HIP events (tsdr_timer_*) around blocks of back-to-back calls, at least 0.3 s of launches per variant in all, after
# a warm-up of every shape.
#
#     python tools/time_hires.py [out.json = profiles/hires_c2.json] [workloads = C2,C5]
#
# Prints one JSON document and writes it to out.json.  GPU box only.
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tempest_loader import load_package  # noqa: E402

T = load_package()
api = importlib.import_module("tempestsdr_jl_amd.api")
synth = importlib.import_module("tempestsdr_jl_amd.synth")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hires_c2.json")
WANT = (sys.argv[2] if len(sys.argv) > 2 else "C2,C5").split(",")
WORKLOADS = {"C2": dict(Fs=20e6, x_t=2576, y_t=1125, fv=60.0, frames=30), "C5": dict(Fs=50e6, x_t=4400, y_t=2250, fv=60.0, frames=30)}
HBM_PEAK = 8.0e12
MIN_SECONDS, ROUNDS = 0.3, 5
NPX = 600 * 800

ctx = T.Context()
res = {"device": ctx.device_info()["name"], "precision": ctx.precision, "rounds": ROUNDS, "min_seconds_per_variant": MIN_SECONDS,
       "workloads": {}}


def timed_blocks(variants, reps):
    """variants: name -> callable (one call = one launch / one buffer).  -> name -> [us per call of each block], blocks alternating"""
    out = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            ctx.timer_start()
            for _ in range(reps):
                fn()
            out[name].append(ctx.timer_stop() / reps * 1e3)
    return out


def summary(blocks):
    return {"us_blocks": [round(b, 2) for b in blocks], "us_median": round(statistics.median(blocks), 2), "us_min": round(min(blocks), 2),
            "us_max": round(max(blocks), 2)}


def reps_for(fn, lo=3):
    """calls per block so that the ROUNDS blocks of a variant add up to MIN_SECONDS at least (from a short warmed trial)"""
    for _ in range(lo):
        fn()
    ctx.timer_start()
    for _ in range(lo):
        fn()
    ms = max(ctx.timer_stop() / lo, 1e-3)
    return max(lo, int(np.ceil(MIN_SECONDS * 1e3 / ms / ROUNDS)))


for wname in WANT:
    w = WORKLOADS[wname]
    y_t, x_t, n = w["y_t"], w["x_t"], w["frames"]
    P = y_t * x_t
    S = synth.samples_per_frame(w["Fs"], w["fv"])
    nEch = S * n
    doc = {"y_t": y_t, "x_t": x_t, "frames": n, "S": S, "raster_bytes_per_frame": 4 * P}
    iq = synth.synth_leak(w["Fs"], x_t, y_t, w["fv"], nEch)
    d_iq = ctx.upload(iq)
    d_state, d_hires = ctx.upload(np.zeros(NPX, np.float32)), ctx.upload(np.zeros(P, np.float32))
    d_rasters, d_idx = ctx.dev_alloc(4 * P * n), ctx.upload(np.zeros(2 * n, np.int32))
    sync = T.SyncXY(ctx, 600, 800)
    alpha = np.float32(0.1)

    def frames_raster():
        api.frames_iq_d(ctx, sync, d_iq, "cf32", 1.0, nEch, S, y_t, x_t, alpha, True, d_state, None, d_rasters, d_idx)

    def frames_hires():
        ctx.frames_hires_d(sync, d_iq, "cf32", 1.0, nEch, S, y_t, x_t, alpha, True, d_state, alpha, d_hires, None, d_idx)

    k192 = max(1, min(n, (192 << 20) // (4 * P)))

    def frames_hires_chunks_192MiB():
        ctx.set_option("hires_chunk_frames", k192)
        try:
            frames_hires()
        finally:
            ctx.set_option("hires_chunk_frames", 0)

    # (a) the kernel alone, on rasters and indices the loop itself wrote
    frames_raster()
    ctx.synchronize()
    idx = ctx.download(d_idx, (n, 2), np.int32)
    doc["sync_idx_first_rows"] = idx[:4].tolist()
    kernel = {"shifted": lambda: ctx.raster_accumulate_d(d_rasters, n, y_t, x_t, alpha, d_hires, d_idx, "image"),
              "unshifted": lambda: ctx.raster_accumulate_d(d_rasters, n, y_t, x_t, alpha, d_hires)}
    reps = max(reps_for(f) for f in kernel.values())
    nbytes = n * 4 * P + 8 * P
    doc["raster_accum"] = {"reps_per_block": reps, "bytes": nbytes}
    for name, blocks in timed_blocks(kernel, reps).items():
        s = summary(blocks)
        s["TB_per_s"] = round(nbytes / (s["us_median"] * 1e-6) / 1e12, 3)
        s["share_of_8TBps"] = round(nbytes / (s["us_median"] * 1e-6) / HBM_PEAK, 3)
        doc["raster_accum"][name] = s
    # (b), (c) the loop per buffer
    loop = {"frames_iq_d_with_raster_out": frames_raster, "frames_hires_one_chunk": frames_hires,
            "frames_hires_chunks_192MiB": frames_hires_chunks_192MiB}
    reps = max(reps_for(f) for f in loop.values())
    doc["loop"] = {"reps_per_block": reps, "chunk_frames_192MiB": k192}
    for name, blocks in timed_blocks(loop, reps).items():
        doc["loop"][name] = summary(blocks)
    base = doc["loop"]["frames_iq_d_with_raster_out"]["us_median"]
    doc["loop"]["added_us_per_buffer_one_chunk"] = round(doc["loop"]["frames_hires_one_chunk"]["us_median"] - base, 2)
    doc["loop"]["added_us_per_buffer_chunks_192MiB"] = round(doc["loop"]["frames_hires_chunks_192MiB"]["us_median"] - base, 2)
    # per-kernel split of one hires buffer, in a block of its own (the event pairs slow the stream down)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(5):
        frames_hires()
    ctx.synchronize()
    doc["loop"]["kernels_us_per_buffer_one_chunk"] = {k: round(v["total_ms"] / 5 * 1e3, 2) for k, v in sorted(ctx.profile_results().items())}
    ctx.profile(False)
    ctx.synchronize()
    for p in (d_iq, d_state, d_hires, d_rasters, d_idx):
        ctx.dev_free(p)
    res["workloads"][wname] = doc

text = json.dumps(res, indent=1)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text + "\n")
