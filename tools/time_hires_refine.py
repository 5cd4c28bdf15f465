# Measures the registration to the raster pixel (include/tempest_hip_register.h, option "hires_refine") at the C2 and C5 workloads
# of SURVEY.md (30 frames per buffer: 2576x1125 at 20 MS/s, 4400x2250 at 50 MS/s), everything in one process on resident buffers,
# variants alternating so that drift hits them alike:
#   (a) the profiles pass alone (tsdr_raster_profiles_d over the 30 rasters of a buffer): us per call, the n*4P bytes it reads over
#       that time; and the whole registration (tsdr_raster_register_d: profiles of the rasters and of ref, scores, choice)
#   (b) tsdr_frames_hires_iq_d per buffer with the option at 0 and at 1: what the refinement adds to a buffer
#   (c) the per-kernel split of one refined buffer
#   (d) the effect on the picture: the residual of tests/test_register_host.py (mean squared distance between each aligned raster
#       and the final state) with the option at 0 and at 1, from a zero state, at the test geometry (150x2400, fv = 60.1) and at C2
#       with fv = 60.14, where S = round(Fs/fv) is off by 0.44 samples per frame
# Times are HIP events (tsdr_timer_*) around blocks of back-to-back calls, at least 0.3 s of calls per variant in all, after a
# warm-up of every shape; medians over the blocks.
#
#     python tools/time_hires_refine.py [out.json = profiles/hires_refine.json] [workloads = C2,C5]
#
# Prints one JSON document and writes it to out.json.  GPU box only.
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
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hires_refine.json")
WANT = (sys.argv[2] if len(sys.argv) > 2 else "C2,C5").split(",")
WORKLOADS = {"C2": dict(Fs=20e6, x_t=2576, y_t=1125, fv=60.0, frames=30), "C5": dict(Fs=50e6, x_t=4400, y_t=2250, fv=60.0, frames=30)}
PICTURES = {"150x2400": dict(Fs=3.0e6, x_t=2400, y_t=150, fv=60.1, frames=6), "C2 fv=60.14": dict(Fs=20e6, x_t=2576, y_t=1125, fv=60.14, frames=30)}
MIN_SECONDS, ROUNDS = 0.3, 5
NPX = 600 * 800

ctx = T.Context()
res = {"device": ctx.device_info()["name"], "precision": ctx.precision, "rounds": ROUNDS, "min_seconds_per_variant": MIN_SECONDS,
       "workloads": {}, "picture": {}}


def timed_blocks(variants, reps):
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
    for _ in range(lo):
        fn()
    ctx.timer_start()
    for _ in range(lo):
        fn()
    ms = max(ctx.timer_stop() / lo, 1e-3)
    return max(lo, int(np.ceil(MIN_SECONDS * 1e3 / ms / ROUNDS)))


def refine_radius(k, y_t, x_t):
    return min(-(-k * y_t // 600), (y_t - 1) // 2), min(-(-k * x_t // 800), (x_t - 1) // 2)


for wname in WANT:
    w = WORKLOADS[wname]
    y_t, x_t, n = w["y_t"], w["x_t"], w["frames"]
    P = y_t * x_t
    S = synth.samples_per_frame(w["Fs"], w["fv"])
    nEch = S * n
    d_y, d_x = refine_radius(1, y_t, x_t)
    doc = {"y_t": y_t, "x_t": x_t, "frames": n, "S": S, "raster_bytes_per_frame": 4 * P, "d_y": d_y, "d_x": d_x}
    d_iq = ctx.upload(synth.synth_leak(w["Fs"], x_t, y_t, w["fv"], nEch))
    d_state, d_hires = ctx.upload(np.zeros(NPX, np.float32)), ctx.upload(np.zeros(P, np.float32))
    d_rasters, d_idx, d_out = ctx.dev_alloc(4 * P * n), ctx.upload(np.zeros(2 * n, np.int32)), ctx.dev_alloc(8 * n)
    d_col, d_row = ctx.dev_alloc(8 * n * x_t), ctx.dev_alloc(8 * n * y_t)
    sync = T.SyncXY(ctx, 600, 800)
    alpha = np.float32(0.1)

    def frames_hires():
        ctx.frames_hires_d(sync, d_iq, "cf32", 1.0, nEch, S, y_t, x_t, alpha, True, d_state, alpha, d_hires, None, d_idx)

    def loop_with(k):
        def run():
            ctx.set_option("hires_refine", k)
            try:
                frames_hires()
            finally:
                ctx.set_option("hires_refine", 0)
        return run

    # (a) the two launches alone, on rasters, indices and a state the loop itself wrote
    api.frames_iq_d(ctx, sync, d_iq, "cf32", 1.0, nEch, S, y_t, x_t, alpha, True, d_state, None, d_rasters, d_idx)
    frames_hires()
    ctx.synchronize()
    alone = {"raster_profiles_d": lambda: ctx.call("tsdr_raster_profiles_d", api._ptr(d_rasters), n, y_t, x_t, api._ptr(d_col), api._ptr(d_row)),
             "raster_register_d": lambda: ctx.raster_register_d(d_rasters, n, y_t, x_t, d_y, d_x, d_out, d_hires, d_idx, "image")}
    reps = max(reps_for(f) for f in alone.values())
    doc["alone"] = {"reps_per_block": reps, "bytes_read_profiles": n * 4 * P}
    for name, blocks in timed_blocks(alone, reps).items():
        doc["alone"][name] = summary(blocks)
    doc["alone"]["raster_profiles_d"]["TB_per_s"] = round(n * 4 * P / (doc["alone"]["raster_profiles_d"]["us_median"] * 1e-6) / 1e12, 3)
    # (b) the loop per buffer, option off / on
    loop = {"hires_refine_0": loop_with(0), "hires_refine_1": loop_with(1)}
    reps = max(reps_for(f) for f in loop.values())
    doc["loop"] = {"reps_per_block": reps}
    for name, blocks in timed_blocks(loop, reps).items():
        doc["loop"][name] = summary(blocks)
    doc["loop"]["added_us_per_buffer"] = round(doc["loop"]["hires_refine_1"]["us_median"] - doc["loop"]["hires_refine_0"]["us_median"], 2)
    # (c) per-kernel split of one refined buffer, in a block of its own (the event pairs slow the stream down)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(5):
        loop_with(1)()
    ctx.synchronize()
    doc["loop"]["kernels_us_per_refined_buffer"] = {k: round(v["total_ms"] / 5 * 1e3, 2) for k, v in sorted(ctx.profile_results().items())}
    ctx.profile(False)
    ctx.synchronize()
    for p in (d_iq, d_state, d_hires, d_rasters, d_idx, d_out, d_col, d_row):
        ctx.dev_free(p)
    res["workloads"][wname] = doc


def residual(rasters, shifts, state):
    """mean squared distance between each aligned raster and the state (tests/test_register_host.py:residual)"""
    st = np.asarray(state, np.float64)
    return float(np.mean([np.mean((np.roll(np.asarray(r, np.float64), (-int(s[0]), -int(s[1])), axis=(0, 1)) - st) ** 2)
                          for r, s in zip(rasters, shifts)]))


# (d) the picture
for pname, w in PICTURES.items():
    y_t, x_t, n = w["y_t"], w["x_t"], w["frames"]
    P = y_t * x_t
    S = synth.samples_per_frame(w["Fs"], w["fv"])
    nEch = S * n
    d_iq = ctx.upload(synth.synth_leak(w["Fs"], x_t, y_t, w["fv"], nEch))
    d_rasters = ctx.dev_alloc(4 * P * n)
    d_state = ctx.upload(np.zeros(NPX, np.float32))
    api.frames_iq_d(ctx, T.SyncXY(ctx, 600, 800), d_iq, "cf32", 1.0, nEch, S, y_t, x_t, np.float32(0.1), True, d_state, None, d_rasters, None)
    rasters = ctx.download(d_rasters, (n, P), np.float32)
    mats = [rasters[f].reshape((y_t, x_t), order="F") for f in range(n)]
    doc = {"y_t": y_t, "x_t": x_t, "frames": n, "S": S, "samples_per_frame_exact": round(w["Fs"] / w["fv"], 3), "by_alpha_hires": {}}
    for a_h in (0.1, 0.9):
        row = {}
        for k in (0, 1):
            d_st, d_hi = ctx.upload(np.zeros(NPX, np.float32)), ctx.upload(np.zeros(P, np.float32))
            ctx.set_option("hires_refine", k)
            try:
                ctx.frames_hires_d(T.SyncXY(ctx, 600, 800), d_iq, "cf32", 1.0, nEch, S, y_t, x_t, np.float32(0.1), True, d_st, np.float32(a_h), d_hi)
            finally:
                ctx.set_option("hires_refine", 0)
            shifts = ctx.hires_shifts()
            state = ctx.download(d_hi, (P,), np.float32).reshape((y_t, x_t), order="F")
            row[f"hires_refine_{k}"] = {"residual": residual(mats, shifts, state), "shifts_first_rows": shifts[:6].tolist()}
            if k:
                row["frames_moved"] = int(np.sum(np.any(shifts != coarse, axis=1)))
                row["largest_move_px"] = [int(v) for v in np.max(np.minimum(np.abs(shifts - coarse), [y_t, x_t] - np.abs(shifts - coarse)), axis=0)]
            else:
                coarse = shifts
            ctx.dev_free(d_st)
            ctx.dev_free(d_hi)
        row["residual_ratio"] = round(row["hires_refine_1"]["residual"] / row["hires_refine_0"]["residual"], 4)
        doc["by_alpha_hires"][str(a_h)] = row
    ctx.dev_free(d_iq)
    ctx.dev_free(d_rasters)
    ctx.dev_free(d_state)
    res["picture"][pname] = doc

text = json.dumps(res, indent=1)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text + "\n")
