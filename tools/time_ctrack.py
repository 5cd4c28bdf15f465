# Measures carrier tracking (include/tempest_hip_ctrack.h) beside its neighbours on resident C2 and C5 buffers (30 frames per buffer of
# a monitor at 60.14 Hz: 2576x1125 at 20 MS/s, 4400x2250 at 50 MS/s; T = Fs/60.14 samples, fractional), ComplexF32, alpha = 0.1
# (every state read and written), everything in one process, variants alternating so that drift hits them alike:
#   cfold            tsdr_cfold_iq_d: the probe's neighbour (one pass over the IQ, one picture)
#   cstack_given     tsdr_cstack_iq_d, GIVEN, zstate + mag, info = NULL
#   cstack_lock      tsdr_cstack_iq_d, LOCK, zstate + mag + info
#   ctrack_given     tsdr_ctrack_stack_iq_d, GIVEN, the same outputs, along a track with a quadratic a_f and a slope b_f
#   ctrack_lock      tsdr_ctrack_stack_iq_d, LOCK
#   ctrack_probe     tsdr_ctrack_probe_iq_d along the same track against a resident picture
# and the ratios ctrack_given / cstack_given, ctrack_lock / cstack_lock, ctrack_probe / cfold.  Times are HIP events (tsdr_timer_*)
# around blocks of back-to-back calls, at least 0.3 s of launches per variant in all, after a warm-up of every shape; then the
# per-kernel split of one call of each.
#
#     python tools/time_ctrack.py [out.json = profiles/ctrack.json] [workloads = C2,C5]
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
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ctrack.json")
WANT = (sys.argv[2] if len(sys.argv) > 2 else "C2,C5").split(",")
WORKLOADS = {"C2": dict(Fs=20e6, x_t=2576, y_t=1125, fv=60.14, frames=30), "C5": dict(Fs=50e6, x_t=4400, y_t=2250, fv=60.14, frames=30),
             # not in the default: T / P = 2.7 samples per pixel -- the direct kernels
             "DIRECT": dict(Fs=50e6, x_t=640, y_t=480, fv=60.14, frames=30)}
MIN_SECONDS, ROUNDS, ALPHA, PHI = 0.3, 5, 0.1, 0.37

ctx = T.Context()
res = {"device": ctx.device_info()["name"], "precision": ctx.precision, "rounds": ROUNDS, "min_seconds_per_variant": MIN_SECONDS,
       "alpha": ALPHA, "workloads": {}}


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
    n = int(math.ceil(F * period)) + 2
    kappa_true = (1e3 * period / w["Fs"]) % 1.0                # synth_leak's df = 1 kHz
    f = np.arange(F, dtype=np.float64)
    track = np.ascontiguousarray(np.stack([PHI + f * kappa_true + 1e-3 * f * f, 2e-3 * f + 0.25], axis=1))
    doc = {"y_t": y_t, "x_t": x_t, "frames": F, "T": period, "n": n, "kappa_true": kappa_true,
           "bytes": {"cfold_8n_8P": 8 * n + 8 * P, "stack_given_8n_20P": 8 * n + 20 * P, "stack_lock_8n_48P": 8 * n + 48 * P,
                     "probe_8n_8P": 8 * n + 8 * P}}
    iq = synth.synth_leak(w["Fs"], x_t, y_t, w["fv"], n)
    d_iq = ctx.upload(iq)
    d_cfold = ctx.upload(np.zeros(P, np.float32))
    d_zs = [ctx.upload(np.zeros(P, np.complex64)) for _ in range(4)]
    d_mag = [ctx.upload(np.zeros(P, np.float32)) for _ in range(4)]
    d_info, d_track, d_out = ctx.dev_alloc(64), ctx.upload(track), ctx.dev_alloc(8 * (4 * F + 1))
    d_ref = ctx.upload(np.zeros(P, np.complex64))
    # the probe's picture: one stack of the buffer itself
    ctx.ctrack_stack_d(d_iq, "cf32", 1.0, n, 0.0, period, d_track, F, y_t, x_t, 0.0, "given", d_ref)

    def cstack(k, mode, info):
        return lambda: ctx.cstack_d(d_iq, "cf32", 1.0, n, 0.0, period, kappa_true, PHI, F, y_t, x_t, ALPHA, mode, d_zs[k], d_mag[k], info)

    def ctrack(k, mode, info):
        return lambda: ctx.ctrack_stack_d(d_iq, "cf32", 1.0, n, 0.0, period, d_track, F, y_t, x_t, ALPHA, mode, d_zs[k], d_mag[k], info)

    variants = {
        "cfold": lambda: ctx.cfold_d(d_iq, "cf32", 1.0, n, 0.0, period, kappa_true, F, y_t, x_t, ALPHA, d_cfold),
        "cstack_given": cstack(0, "given", None),
        "ctrack_given": ctrack(1, "given", None),
        "cstack_lock": cstack(2, "lock", d_info),
        "ctrack_lock": ctrack(3, "lock", d_info),
        "ctrack_probe": lambda: ctx.ctrack_probe_d(d_iq, "cf32", 1.0, n, 0.0, period, d_track, F, y_t, x_t, d_ref, d_out),
    }
    reps = {k: reps_for(fn) for k, fn in variants.items()}
    doc["reps_per_block"] = reps
    for name, blocks in timed_blocks(variants, reps).items():
        doc[name] = summary(blocks)
    for name, beside in (("ctrack_given", "cstack_given"), ("ctrack_lock", "cstack_lock"), ("ctrack_probe", "cfold")):
        doc[f"{name}_over_{beside}_time"] = round(doc[name]["us_median"] / doc[beside]["us_median"], 3)
    ctx.synchronize()
    out = ctx.download(d_out, (4 * F + 1,), np.float64)
    doc["probe_gamma_min_max"] = [float(out[3:4 * F:4].min()), float(out[3:4 * F:4].max())]
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
    for p in [d_iq, d_cfold, d_info, d_track, d_out, d_ref] + d_zs + d_mag:
        ctx.dev_free(p)
    res["workloads"][wname] = doc

text = json.dumps(res, indent=1)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text + "\n")
