"""What the 8-bit IQ input buys on workload C2 (1080p60 at 20 MS/s, 0.5 s buffers), next to the formats that were there before,
every comparison inside one process:
  ingest   ingest.bench_ingest -- every buffer crosses PCIe through the staging ring -- frames/s and GB/s for ring formats
           cf32, sc16raw, sc8raw, uc8raw.  The comparison that matters is sc8raw against sc16raw: ~2x if PCIe is the bound.
  kernels  the image launches on device-resident buffers, HIP-event time per launch (the context's profiler) for cf32 / sc16 /
           sc8 / uc8 input: raster_down_iq (C2, FAST with rasters), the raster-free launch of C2 (down_fused_iq_sums) and
           down_walk_iq (the raster walk without rasters, at a geometry of more than two samples per pixel); min / median /
           max over --rounds rounds of --reps buffers (the spread is what the formats' differences are read against).
  search   tsdr_autocorr_search_iq_d at n = 4e6 (the reference's window at 20 MS/s) for cf32 / sc16 / sc8 input, stream time
           per call.
Without --step this file is the driver: it starts one child process per step, each under its own time limit, and stops at the
first step that fails or runs out of time.  One JSON line per step; --json FILE keeps them.
   python tools/time_iq8.py [--seconds 1.0] [--reps 20] [--rounds 5] [--json out.json]"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS = {"ingest": 240, "kernels": 240, "search": 180}   # seconds allowed per step

ap = argparse.ArgumentParser()
ap.add_argument("--step", choices=list(STEPS))
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

if args.step is None:
    lines = []
    for step, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--seconds", str(args.seconds), "--reps", str(args.reps),
               "--rounds", str(args.rounds)]
        try:
            r = subprocess.run(cmd, timeout=limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            sys.exit(f"time_iq8: step {step} did not finish within {limit} s; nothing further is started")
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            sys.stdout.write(r.stdout[-2000:])
            sys.exit(f"time_iq8: step {step} failed (exit status {r.returncode}); nothing further is started")
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        print(out[-1], flush=True)
        lines.append(json.loads(out[-1]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(lines, f, indent=1)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import iq8_ref as R  # noqa: E402
from tempest_loader import load_package  # noqa: E402

tsdr = load_package()
synth = importlib.import_module("tempestsdr_jl_amd.synth")
api = importlib.import_module("tempestsdr_jl_amd.api")
ingest = importlib.import_module("tempestsdr_jl_amd.ingest")
ctx = tsdr.Context(0)
w = synth.WORKLOADS["C2"]
Fs, x_t, y_t, fv = w["Fs"], w["x_t"], w["y_t"], w["fv"]
S = synth.samples_per_frame(Fs, fv)
res = {"step": args.step, "device": ctx.device_info()["name"], "workload": "C2"}

if args.step == "ingest":
    nEch = int(round(w["acquisition"] * Fs))
    iq = synth.synth_leak(Fs, x_t, y_t, fv, nEch)
    for fmt in ("cf32", "sc16raw", "sc8raw", "uc8raw"):
        res[fmt] = ingest.bench_ingest(ctx, tsdr, iq, S, y_t, x_t, seconds=args.seconds, fmt=fmt)
    res["sc8raw_over_sc16raw"] = round(res["sc8raw"]["frames_per_s"] / res["sc16raw"]["frames_per_s"], 3)
    res["sc16raw_over_cf32"] = round(res["sc16raw"]["frames_per_s"] / res["cf32"]["frames_per_s"], 3)

elif args.step == "kernels":
    IMAGE_KERNELS = ("raster_down_iq", "down_walk_iq", "down_fused_iq_sums", "down_fused_iq")
    # (C2 without rasters takes the tap kernel, down_fused_iq_sums; the raster walk without rasters, down_walk_iq, serves
    # geometries of more than two samples per raster pixel: 800x600@60 at 100 MS/s is one)
    legs = (("C2_rasters", Fs, x_t, y_t, 0.5, True), ("C2_raster_free", Fs, x_t, y_t, 0.5, False),
            ("100MSps_1056x628_raster_free", 100e6, 1056, 628, 0.1, False))
    for leg, fs_, xt_, yt_, acq, raster in legs:
        S_ = synth.samples_per_frame(fs_, fv)
        nEch = int(round(acq * fs_))
        nb = nEch // S_
        z = synth.synth_leak(fs_, xt_, yt_, fv, nEch)
        dev = {"cf32": (torch.from_numpy(z.view(np.float32).copy()).cuda(), 1.0)}
        for fmt in ("sc16", "sc8", "uc8"):
            q, scale = R.quantise(z, fmt)
            dev[fmt] = (torch.from_numpy(q.view(np.uint8).copy()).cuda(), float(scale))
        state = torch.zeros(480000, device="cuda")
        fo = torch.empty(nb * 480000, device="cuda")
        ro = torch.empty(nb * xt_ * yt_, device="cuda") if raster else None
        si = torch.zeros(2 * nb, dtype=torch.int32, device="cuda")
        sync = tsdr.SyncXY(ctx, 600, 800)
        torch.cuda.synchronize()
        samples = {}
        for rnd in range(args.rounds + 1):          # (round 0 warms up; the formats alternate inside every round)
            for fmt, (buf, scale) in dev.items():
                ctx.profile_reset()
                ctx.profile(True)
                for _ in range(args.reps):
                    api.frames_iq_d(ctx, sync, buf, fmt, scale, nEch, S_, yt_, xt_, np.float32(0.1), True, state, fo, ro, si)
                ctx.synchronize()
                ctx.profile(False)
                for k, pr in ctx.profile_results().items():
                    if rnd and k in IMAGE_KERNELS and pr["launches"]:
                        samples.setdefault(k, {}).setdefault(fmt, []).append(1e3 * pr["total_ms"] / pr["launches"])
        res[leg] = {k: {fmt: {"us_min": round(min(v), 1), "us_median": round(float(np.median(v)), 1), "us_max": round(max(v), 1)}
                        for fmt, v in per.items()} for k, per in samples.items()}
        sync.close()
        del dev, fo, ro

else:
    n = 4_000_000
    z = synth.synth_leak(Fs, x_t, y_t, fv, n)
    import ctypes as C
    cnt = int(round(0.1 * Fs))
    pmin, pmax = C.c_size_t(0), C.c_size_t(0)
    assert ctx.lib.tsdr_zoom_bounds(cnt, float(Fs), 50.0, 90.0, C.byref(pmin), C.byref(pmax)) == 0
    d_out = ctx.dev_alloc(cnt * 4)
    picks = {}
    for fmt in ("cf32", "sc16", "sc8"):
        if fmt == "cf32":
            host, scale = z.view(np.float32), 1.0
        else:
            host, scale = R.quantise(z, fmt)
        d_in = ctx.upload(host)
        n_out, idx, val = C.c_size_t(0), C.c_size_t(0), C.c_float(0)

        def call():
            ctx.call("tsdr_autocorr_search_iq_d", C.c_void_p(d_in), R.CODES[fmt], C.c_float(scale), n, float(Fs), 0.0, 0.1, 1,
                     C.c_void_p(d_out), C.byref(n_out), int(pmin.value - 1), int(pmax.value - pmin.value + 1), C.byref(idx), C.byref(val))

        for _ in range(3):
            call()
        ctx.synchronize()
        v = []
        for _ in range(args.rounds):
            ctx.timer_start()
            for _ in range(args.reps):
                call()
            v.append(1e3 * ctx.timer_stop() / args.reps)
        picks[fmt] = int(pmin.value - 1 + idx.value)
        res[fmt] = {"us_min": round(min(v), 1), "us_median": round(float(np.median(v)), 1), "us_max": round(max(v), 1),
                    "input_MB": round(host.nbytes / 1e6, 1), "lag": picks[fmt]}
        ctx.dev_free(d_in)
    ctx.dev_free(d_out)

print(json.dumps(res), flush=True)
