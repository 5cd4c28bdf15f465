# Measures coherent frame folding (include/tempest_hip_fold.h) on resident C2 and C5 buffers (30 frames per buffer of a monitor at
# 60.14 Hz: 2576x1125 at 20 MS/s, 4400x2250 at 50 MS/s; T = Fs/60.14 samples, fractional), everything in one process, variants
# alternating so that drift hits them alike:
#   (a) tsdr_fold_iq_d per buffer, alpha = 0 (state written) and alpha = 0.1 (state read and written): us per call, the bytes the
#       algorithm needs, 8n + 8P, over that time, as a share of the 8 TB/s HBM peak and of the 6.29 TB/s copy figure of DESIGN.md section 4
#   (b) a 17-trial tsdr_fold_scan_iq_d at dT = 1/8 sample around T: us per call and per trial
#   (c) tsdr_frames_hires_iq_d on the same buffer with S = round(T), "hires_refine" 0 and 1: what the full-size picture cost so far
# Times are HIP events (tsdr_timer_*) around blocks of back-to-back calls, at least 0.3 s of launches per variant in all, after a
# warm-up of every shape.
#
#     python tools/time_fold.py [out.json = profiles/fold.json] [workloads = C2,C5]
#
# Prints one JSON document and writes it to out.json.  GPU box only.
import importlib
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tempest_loader import load_package  # noqa: E402

T = load_package()
synth = importlib.import_module("tempestsdr_jl_amd.synth")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fold.json")
WANT = (sys.argv[2] if len(sys.argv) > 2 else "C2,C5").split(",")
WORKLOADS = {"C2": dict(Fs=20e6, x_t=2576, y_t=1125, fv=60.14, frames=30), "C5": dict(Fs=50e6, x_t=4400, y_t=2250, fv=60.14, frames=30)}
HBM_PEAK, COPY = 8.0e12, 6.29e12
MIN_SECONDS, ROUNDS = 0.3, 5
NPX = 600 * 800
N_TRIALS, DT = 17, 0.125

ctx = T.Context()
res = {"device": ctx.device_info()["name"], "precision": ctx.precision, "rounds": ROUNDS, "min_seconds_per_variant": MIN_SECONDS,
       "workloads": {}}


def timed_blocks(variants, reps):
    """variants: name -> callable (one call = one buffer).  -> name -> [us per call of each block], blocks alternating"""
    out = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            ctx.timer_start()
            for _ in range(reps[name]):
                fn()
            out[name].append(ctx.timer_stop() / reps[name] * 1e3)
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
    y_t, x_t, F = w["y_t"], w["x_t"], w["frames"]
    P = y_t * x_t
    period = w["Fs"] / w["fv"]
    half = (N_TRIALS - 1) // 2
    n = int(math.ceil(F * (period + half * DT))) + 2          # the scan's largest trial still holds F frames
    S = int(round(period))
    doc = {"y_t": y_t, "x_t": x_t, "frames": F, "T": period, "n": n, "S_of_the_frame_loop": S, "bytes_8n_8P": 8 * n + 8 * P}
    iq = synth.synth_leak(w["Fs"], x_t, y_t, w["fv"], n)
    d_iq = ctx.upload(iq)
    d_fold, d_score = ctx.upload(np.zeros(P, np.float32)), ctx.dev_alloc(8 * N_TRIALS)
    d_state, d_hires = ctx.upload(np.zeros(NPX, np.float32)), ctx.upload(np.zeros(P, np.float32))
    d_idx = ctx.upload(np.zeros(2 * (n // S), np.int32))
    sync = T.SyncXY(ctx, 600, 800)
    alpha = np.float32(0.1)

    def hires(refine):
        ctx.set_option("hires_refine", refine)
        try:
            ctx.frames_hires_d(sync, d_iq, "cf32", 1.0, n, S, y_t, x_t, alpha, True, d_state, alpha, d_hires, None, d_idx)
        finally:
            ctx.set_option("hires_refine", 0)

    variants = {
        "fold_alpha_0": lambda: ctx.fold_d(d_iq, "cf32", 1.0, n, 0.0, period, F, y_t, x_t, 0.0, d_fold),
        "fold_alpha_0.1": lambda: ctx.fold_d(d_iq, "cf32", 1.0, n, 0.0, period, F, y_t, x_t, 0.1, d_fold),
        "fold_scan_17": lambda: ctx.fold_scan_d(d_iq, "cf32", 1.0, n, 0.0, period - half * DT, DT, N_TRIALS, F, y_t, x_t, d_score),
        "frames_hires_refine_0": lambda: hires(0),
        "frames_hires_refine_1": lambda: hires(1),
    }
    reps = {k: reps_for(f) for k, f in variants.items()}
    doc["reps_per_block"] = reps
    for name, blocks in timed_blocks(variants, reps).items():
        s = summary(blocks)
        if name.startswith("fold_alpha"):
            rate = doc["bytes_8n_8P"] / (s["us_median"] * 1e-6)
            s.update(TB_per_s=round(rate / 1e12, 3), share_of_8TBps=round(rate / HBM_PEAK, 3), share_of_copy_6_29TBps=round(rate / COPY, 3))
        if name == "fold_scan_17":
            s["us_per_trial"] = round(s["us_median"] / N_TRIALS, 2)
        doc[name] = s
    ctx.synchronize()
    scores = ctx.download(d_score, (N_TRIALS,), np.float64)
    doc["scan_first_maximum"] = int(np.argmax(scores))
    doc["scan_scores_relative"] = [round(float(v / scores.max()), 5) for v in scores]
    # per-kernel split of one fold and one scan, in a block of its own (the event pairs slow the stream down)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(5):
        variants["fold_alpha_0.1"]()
        variants["fold_scan_17"]()
    ctx.synchronize()
    doc["kernels_us_per_call"] = {k: round(v["total_ms"] / 5 * 1e3, 2) for k, v in sorted(ctx.profile_results().items())}
    ctx.profile(False)
    ctx.synchronize()
    for p in (d_iq, d_fold, d_score, d_state, d_hires, d_idx):
        ctx.dev_free(p)
    res["workloads"][wname] = doc

text = json.dumps(res, indent=1)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text + "\n")
