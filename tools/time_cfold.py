# Measures phase-coherent frame folding (include/tempest_hip_cfold.h) beside the envelope fold (include/tempest_hip_fold.h) on resident
# C2 and C5 buffers (30 frames per buffer of a monitor at 60.14 Hz: 2576x1125 at 20 MS/s, 4400x2250 at 50 MS/s; T = Fs/60.14 samples,
# fractional), ComplexF32, everything in one process, variants alternating so that drift hits them alike:
#   (a) tsdr_cfold_iq_d and tsdr_fold_iq_d per buffer, alpha = 0.1 (state read and written): us per call and their ratio
#   (b) tsdr_cfold_scan_iq_d with 4 F trials over [0, 1) beside a 17-trial tsdr_fold_scan_iq_d at dT = 1/8 sample around T: us per
#       call and per trial, and the ratio of the two per-trial times -- the one condition: the coherent scan, which samples the IQ once
#       per batch of trials, must cost less per trial than the envelope scan, which samples it once per trial
# Times are HIP events (tsdr_timer_*) around blocks of back-to-back calls, at least 0.3 s of launches per variant in all, after a
# warm-up of every shape.
#
#     python tools/time_cfold.py [out.json = profiles/cfold.json] [workloads = C2,C5]
#
# Workload DIRECT (640x480 at 50 MS/s, not in the default) is the one whose spans do not fit the staged kernels.
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
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cfold.json")
WANT = (sys.argv[2] if len(sys.argv) > 2 else "C2,C5").split(",")
WORKLOADS = {"C2": dict(Fs=20e6, x_t=2576, y_t=1125, fv=60.14, frames=30), "C5": dict(Fs=50e6, x_t=4400, y_t=2250, fv=60.14, frames=30),
             # not in the default: T / P = 2.7 samples per pixel, W = 350 -- all four calls take their direct kernel (kernels_us_per_call)
             "DIRECT": dict(Fs=50e6, x_t=640, y_t=480, fv=60.14, frames=30)}
MIN_SECONDS, ROUNDS = 0.3, 5
N_TRIALS, DT = 17, 0.125          # the envelope scan of tools/time_fold.py
OVERSAMPLE = 4                    # the coherent scan: refine_carrier's level 0

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
    n = int(math.ceil(F * (period + half * DT))) + 2          # the envelope scan's largest trial still holds F frames
    nk = OVERSAMPLE * F
    kappa_true = (1e3 * period / w["Fs"]) % 1.0                # synth_leak's df = 1 kHz
    doc = {"y_t": y_t, "x_t": x_t, "frames": F, "T": period, "n": n, "bytes_8n_8P": 8 * n + 8 * P, "kappa_true": kappa_true,
           "cfold_scan_trials": nk, "fold_scan_trials": N_TRIALS, "flops_per_coherent_trial_8FP": 8 * F * P}
    iq = synth.synth_leak(w["Fs"], x_t, y_t, w["fv"], n)
    d_iq = ctx.upload(iq)
    d_fold, d_cfold = ctx.upload(np.zeros(P, np.float32)), ctx.upload(np.zeros(P, np.float32))
    d_score, d_cscore = ctx.dev_alloc(8 * N_TRIALS), ctx.dev_alloc(8 * nk)
    variants = {
        "fold_alpha_0.1": lambda: ctx.fold_d(d_iq, "cf32", 1.0, n, 0.0, period, F, y_t, x_t, 0.1, d_fold),
        "cfold_alpha_0.1": lambda: ctx.cfold_d(d_iq, "cf32", 1.0, n, 0.0, period, kappa_true, F, y_t, x_t, 0.1, d_cfold),
        "fold_scan_17": lambda: ctx.fold_scan_d(d_iq, "cf32", 1.0, n, 0.0, period - half * DT, DT, N_TRIALS, F, y_t, x_t, d_score),
        "cfold_scan_4F": lambda: ctx.cfold_scan_d(d_iq, "cf32", 1.0, n, 0.0, period, 0.0, 1.0 / nk, nk, F, y_t, x_t, d_cscore),
    }
    reps = {k: reps_for(f) for k, f in variants.items()}
    doc["reps_per_block"] = reps
    for name, blocks in timed_blocks(variants, reps).items():
        s = summary(blocks)
        if name == "fold_scan_17":
            s["us_per_trial"] = round(s["us_median"] / N_TRIALS, 2)
        if name == "cfold_scan_4F":
            s["us_per_trial"] = round(s["us_median"] / nk, 2)
            s["GFLOP_per_s_8FP_per_trial"] = round(8.0 * F * P * nk / (s["us_median"] * 1e-6) / 1e9, 1)
        doc[name] = s
    doc["cfold_over_fold_time"] = round(doc["cfold_alpha_0.1"]["us_median"] / doc["fold_alpha_0.1"]["us_median"], 3)
    doc["coherent_over_envelope_scan_time_per_trial"] = round(doc["cfold_scan_4F"]["us_per_trial"] / doc["fold_scan_17"]["us_per_trial"], 3)
    doc["coherent_scan_is_cheaper_per_trial"] = doc["cfold_scan_4F"]["us_per_trial"] < doc["fold_scan_17"]["us_per_trial"]
    ctx.synchronize()
    scores = ctx.download(d_cscore, (nk,), np.float64)
    doc["cfold_scan_first_maximum"] = int(np.argmax(scores))
    doc["cfold_scan_kappa_at_maximum"] = int(np.argmax(scores)) / nk
    # per-kernel split of one call of each, in a block of its own (the event pairs slow the stream down)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(5):
        for fn in variants.values():
            fn()
    ctx.synchronize()
    doc["kernels_us_per_call"] = {k: round(v["total_ms"] / 5 * 1e3, 2) for k, v in sorted(ctx.profile_results().items())}
    ctx.profile(False)
    ctx.synchronize()
    for p in (d_iq, d_fold, d_cfold, d_score, d_cscore):
        ctx.dev_free(p)
    res["workloads"][wname] = doc

text = json.dumps(res, indent=1)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text + "\n")
