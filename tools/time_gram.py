# Measures the frame Gram matrix (include/tempest_hip_gram.h) beside what it replaces, on resident C2 and C5 buffers (30 frames per
# buffer of a monitor at 60.14 Hz: 2576x1125 at 20 MS/s, 4400x2250 at 50 MS/s; T = Fs/60.14 samples, fractional), ComplexF32,
# everything in one process, variants alternating so that drift hits them alike:
#   cfold            tsdr_cfold_iq_d, alpha = 0.1: one pass over the IQ, one picture -- the unit the Gram call is measured in
#   gram_null        tsdr_ctrack_gram_iq_d with no track
#   gram_track       tsdr_ctrack_gram_iq_d along a track with a quadratic a_f and a slope b_f
#   cfold_scan_4F    tsdr_cfold_scan_iq_d with 4 F trials: level 0 of refine_carrier, which gram_carrier replaces
# and, end to end with their host work and synchronisations (wall clock, median of 5): refine_track (from the true kappa, two
# iterations) beside blind_track (two passes), and refine_carrier beside one Gram + gram_carrier.  Times of the first group are HIP
# events (tsdr_timer_*) around blocks of back-to-back calls, at least 0.3 s of launches per variant in all, after a warm-up of every
# shape; then the per-kernel split of one call of each.
#
#     python tools/time_gram.py [out.json = profiles/gram.json] [workloads = C2,C5]
#
# Prints one JSON document and writes it to out.json.  GPU box only.
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tempest_loader import load_package  # noqa: E402

T = load_package()
synth = importlib.import_module("tempestsdr_jl_amd.synth")
gram = importlib.import_module("tempestsdr_jl_amd.gram")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gram.json")
WANT = (sys.argv[2] if len(sys.argv) > 2 else "C2,C5").split(",")
WORKLOADS = {"C2": dict(Fs=20e6, x_t=2576, y_t=1125, fv=60.14, frames=30), "C5": dict(Fs=50e6, x_t=4400, y_t=2250, fv=60.14, frames=30),
             # not in the default: T / P = 2.7 samples per pixel -- the direct kernels
             "DIRECT": dict(Fs=50e6, x_t=640, y_t=480, fv=60.14, frames=30)}
MIN_SECONDS, ROUNDS, ALPHA, PHI, WALL_ROUNDS = 0.3, 5, 0.1, 0.37, 5

ctx = T.Context()
res = {"device": ctx.device_info()["name"], "precision": ctx.precision, "rounds": ROUNDS, "min_seconds_per_variant": MIN_SECONDS,
       "wall_rounds": WALL_ROUNDS, "workloads": {}}


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


def wall(fn):
    """one warm-up, then WALL_ROUNDS calls from an idle stream: us per call, host work and waits included"""
    fn()
    out = []
    for _ in range(WALL_ROUNDS):
        ctx.synchronize()
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        out.append((time.perf_counter() - t) * 1e6)
    return summary(out)


for wname in WANT:
    w = WORKLOADS[wname]
    y_t, x_t, F = w["y_t"], w["x_t"], w["frames"]
    P = y_t * x_t
    period = w["Fs"] / w["fv"]
    n = int(math.ceil(F * period)) + 2
    kappa_true = (1e3 * period / w["Fs"]) % 1.0                # synth_leak's df = 1 kHz
    f = np.arange(F, dtype=np.float64)
    track = np.ascontiguousarray(np.stack([PHI + f * kappa_true + 1e-3 * f * f, 2e-3 * f + 0.25], axis=1))
    doc = {"y_t": y_t, "x_t": x_t, "frames": F, "T": period, "n": n, "kappa_true": kappa_true, "scan_trials": 4 * F}
    iq = synth.synth_leak(w["Fs"], x_t, y_t, w["fv"], n)
    d_iq = ctx.upload(iq)
    d_cfold, d_zs, d_mag = ctx.upload(np.zeros(P, np.float32)), ctx.upload(np.zeros(P, np.complex64)), ctx.upload(np.zeros(P, np.float32))
    d_track, d_gram, d_score = ctx.upload(track), ctx.dev_alloc(16 * F * F), ctx.dev_alloc(8 * 4 * F)

    variants = {
        "cfold": lambda: ctx.cfold_d(d_iq, "cf32", 1.0, n, 0.0, period, kappa_true, F, y_t, x_t, ALPHA, d_cfold),
        "gram_null": lambda: ctx.ctrack_gram_d(d_iq, "cf32", 1.0, n, 0.0, period, None, F, y_t, x_t, d_gram),
        "gram_track": lambda: ctx.ctrack_gram_d(d_iq, "cf32", 1.0, n, 0.0, period, d_track, F, y_t, x_t, d_gram),
        "cfold_scan_4F": lambda: ctx.cfold_scan_d(d_iq, "cf32", 1.0, n, 0.0, period, 0.0, 1.0 / (4 * F), 4 * F, F, y_t, x_t, d_score),
    }
    reps = {k: reps_for(fn) for k, fn in variants.items()}
    doc["reps_per_block"] = reps
    for name, blocks in timed_blocks(variants, reps).items():
        doc[name] = summary(blocks)
    for name in ("gram_null", "gram_track", "cfold_scan_4F"):
        doc[f"{name}_over_cfold_time"] = round(doc[name]["us_median"] / doc["cfold"]["us_median"], 3)
    doc["cfold_scan_4F_over_gram_null_time"] = round(doc["cfold_scan_4F"]["us_median"] / doc["gram_null"]["us_median"], 3)
    # what the two find: the carrier from one Gram against the scan's ladder
    variants["gram_null"]()
    ctx.synchronize()
    G = gram.gram_matrix(ctx.download(d_gram, (2 * F * F,), np.float64), F)
    doc["gram_carrier"] = list(ctx.gram_carrier(G))
    doc["refine_carrier"] = list(ctx.refine_carrier(d_iq, "cf32", 1.0, n, 0.0, period, F, y_t, x_t)[:2])
    # end to end, host work and waits included
    doc["wall_refine_carrier"] = wall(lambda: ctx.refine_carrier(d_iq, "cf32", 1.0, n, 0.0, period, F, y_t, x_t))

    def gram_carrier_end_to_end():
        variants["gram_null"]()
        ctx.synchronize()
        return ctx.gram_carrier(gram.gram_matrix(ctx.download(d_gram, (2 * F * F,), np.float64), F))

    doc["wall_gram_carrier"] = wall(gram_carrier_end_to_end)
    doc["wall_refine_track"] = wall(lambda: ctx.refine_track(d_iq, "cf32", 1.0, n, 0.0, period, F, y_t, x_t, kappa_true, 2, 2, d_zs, d_mag))
    doc["wall_blind_track"] = wall(lambda: ctx.blind_track(d_iq, "cf32", 1.0, n, 0.0, period, F, y_t, x_t, 2, d_zs, d_mag))
    # per-kernel split of one call of each variant, each variant in a block of its own (the event pairs slow the stream down)
    doc["kernels_us_per_call"] = {}
    for name, fn in variants.items():
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(5):
            fn()
        ctx.synchronize()
        doc["kernels_us_per_call"][name] = {k: round(v["total_ms"] / 5 * 1e3, 2) for k, v in sorted(ctx.profile_results().items())}
        ctx.profile(False)
    ctx.synchronize()
    for p in [d_iq, d_cfold, d_zs, d_mag, d_track, d_gram, d_score]:
        ctx.dev_free(p)
    res["workloads"][wname] = doc

text = json.dumps(res, indent=1)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text + "\n")
