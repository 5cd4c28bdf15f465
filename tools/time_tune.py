# Measures the tuner (include/tempest_hip_tune.h) beside the library's own streaming kernel with the nearest read : write mix, on
# resident C2 and C5 buffers (10^7 and 2.5 * 10^7 samples), ComplexF32 and sc16, everything in one process, variants alternating so that
# drift hits them alike:
#   expand_<fmt>          tsdr_iq_expand_d on the buffer: reads it once, writes n ComplexF32 (ComplexF32 input: a device-to-device copy)
#   tune_<fmt>_D<d>_L<l>  tsdr_tune_iq_d with a full history (a chained call): reads the buffer once, writes n / D ComplexF32 and the history;
#                         (D, L) = (4, 63), (2, 127), (16, 255)
# Times are HIP events (tsdr_timer_*) around blocks of back-to-back calls, at least 0.3 s of launches per variant in all, after a warm-up
# of every shape; medians of the blocks; then the per-kernel split of one call ("tune" and "tune_hist").  No threshold is asserted.
#
#     python tools/time_tune.py [out.json = profiles/tune.json] [workloads = C2,C5]
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
tune = importlib.import_module("tempestsdr_jl_amd.tune")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tune.json")
WANT = (sys.argv[2] if len(sys.argv) > 2 else "C2,C5").split(",")
WORKLOADS = {"C2": dict(Fs=20e6, n=10_000_000), "C5": dict(Fs=50e6, n=25_000_000)}
SHAPES = [(4, 63), (2, 127), (16, 255)]
FORMATS = {"cf32": 8, "sc16": 4}
MIN_SECONDS, ROUNDS, SCALE = 0.3, 5, 1.0 / 2048.0

ctx = T.Context()
res = {"device": ctx.device_info()["name"], "rounds": ROUNDS, "min_seconds_per_variant": MIN_SECONDS, "workloads": {}}


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
    n = w["n"]
    doc = {"n": n, "Fs": w["Fs"], "shapes_D_L": SHAPES}
    q = np.random.default_rng(1).integers(-2048, 2048, 2 * n).astype(np.int16)
    d_iq = {"sc16": ctx.upload(q), "cf32": ctx.dev_alloc(8 * n)}
    ctx.call("tsdr_iq_expand_d", d_iq["sc16"], 1, C.c_float(SCALE), n, d_iq["cf32"])
    ctx.synchronize()
    del q
    d_exp = ctx.dev_alloc(8 * n)
    m0 = 1 << 33
    nu = tune.freq_fix(-0.23 * w["Fs"], w["Fs"])
    variants, frees = {}, [d_exp] + list(d_iq.values())
    for fmt in FORMATS:
        variants[f"expand_{fmt}"] = (lambda f=fmt: ctx.call("tsdr_iq_expand_d", d_iq[f], 0 if f == "cf32" else 1, C.c_float(SCALE), n, d_exp))
        for D, L in SHAPES:
            j0 = -(-(m0 - (L - 1)) // D)
            cap, _ = tune.tune_plan(m0, n, L, D, j0, L - 1)
            d_taps, d_hist, d_out = ctx.upload(tune.design_lowpass(L, D)), ctx.upload(np.zeros(L - 1, np.complex64)), ctx.dev_alloc(8 * cap)
            frees += [d_taps, d_hist, d_out]
            variants[f"tune_{fmt}_D{D}_L{L}"] = (lambda f=fmt, D=D, L=L, j0=j0, t=d_taps, h=d_hist, o=d_out, c=cap:
                                                 ctx.tune_d(d_iq[f], f, SCALE, n, m0, nu, 0, t, L, D, j0, h, L - 1, o, c))
            doc[f"n_out_D{D}_L{L}"] = cap
    reps = {k: reps_for(fn) for k, fn in variants.items()}
    doc["reps_per_block"] = reps
    for name, blocks in timed_blocks(variants, reps).items():
        doc[name] = summary(blocks)
    for fmt, b in FORMATS.items():
        for D, L in SHAPES:
            k = f"tune_{fmt}_D{D}_L{L}"
            us = doc[k]["us_median"]
            doc[k + "_over_expand_time"] = round(us / doc[f"expand_{fmt}"]["us_median"], 3)
            doc[k + "_GBps_read_plus_written"] = round((b * n + 8 * doc[f"n_out_D{D}_L{L}"]) / us * 1e-3, 1)
            doc[k + "_GFMA_per_s"] = round(2.0 * L * doc[f"n_out_D{D}_L{L}"] / us * 1e-3, 1)
            doc[k + "_Gsamples_per_s"] = round(n / us * 1e-3, 2)
        doc[f"expand_{fmt}_GBps_read_plus_written"] = round((b + 8) * n / doc[f"expand_{fmt}"]["us_median"] * 1e-3, 1)
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
    for p in frees:
        ctx.dev_free(p)
    res["workloads"][wname] = doc

text = json.dumps(res, indent=1)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write(text + "\n")
