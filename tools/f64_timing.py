"""Device time of the Float64 per-function entry points (`_f64_d`, include/tempest_hip.h) next to their f32 twins at the same
size: HIP events on the context's stream around `reps` back-to-back calls after `warm` unmeasured ones, the mean per call.
   python tools/f64_timing.py [--reps 20] [--warm 3] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tempest_loader import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

tsdr = load_package()
ctx = tsdr.Context(0)
L, h = ctx.lib, ctx.h
rng = np.random.default_rng(1)
V = C.c_void_p


def timed(fn):
    for _ in range(args.warm):
        fn()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(args.reps):
        fn()
    return 1e3 * ctx.timer_stop() / args.reps   # microseconds per call


def dev(a):
    return V(ctx.upload(a))


def chk(rc):
    assert rc == 0, (rc, L.tsdr_last_error(h))


rows = []


def row(name, size, us64, us32, note=""):
    rows.append({"entry": name, "size": size, "f64_us": round(us64, 2), "f32_us": round(us32, 2), "note": note})
    print(f"{name:<22} {size:<28} f64 {us64:10.2f} us   f32 {us32:10.2f} us   x{us64 / us32:5.2f}  {note}", flush=True)


# am_demod: 1e7 samples (f64: 160 MB in + 80 MB out)
n = 10_000_000
z64 = dev((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex128))
z32 = dev(np.zeros(n, np.complex64))
o64, o32 = V(ctx.dev_alloc(8 * n)), V(ctx.dev_alloc(4 * n))
t64 = timed(lambda: chk(L.tsdr_am_demod_f64_d(h, z64, n, o64)))
t32 = timed(lambda: chk(L.tsdr_am_demod_d(h, z32, n, o32)))
row("am_demod_d", "1e7 samples", t64, t32, f"f64 {240e6 / (t64 * 1e-6) / 1e12:.2f} TB/s")
row("abs2_d", "1e7 samples", timed(lambda: chk(L.tsdr_abs2_f64_d(h, z64, n, o64))), timed(lambda: chk(L.tsdr_abs2_d(h, z32, n, o32))))
row("fm_demod_d", "1e7 samples", timed(lambda: chk(L.tsdr_fm_demod_f64_d(h, z64, n, o64))),
    timed(lambda: chk(L.tsdr_fm_demod_d(h, z32, n, o32))))
row("invert_am_d", "1e7 samples", timed(lambda: chk(L.tsdr_invert_am_f64_d(h, z64, n, o64))),
    timed(lambda: chk(L.tsdr_invert_am_d(h, z32, n, o32))))

# sig_to_image at C2 (333 333 -> 1125 x 2576) and C5 (833 333 -> 2250 x 4400), one frame per call
for S, y_t, x_t, tag in [(333_333, 1125, 2576, "C2"), (833_333, 2250, 4400, "C5")]:
    s64, s32 = dev(rng.random(S)), dev(rng.random(S, dtype=np.float32))
    i64, i32 = V(ctx.dev_alloc(8 * y_t * x_t)), V(ctx.dev_alloc(4 * y_t * x_t))
    t64 = timed(lambda: chk(L.tsdr_sig_to_image_f64_d(h, s64, S, y_t, x_t, i64)))
    t32 = timed(lambda: chk(L.tsdr_sig_to_image_d(h, s32, S, y_t, x_t, i32)))
    mb = (8 * S + 8 * y_t * x_t) / 1e6
    row("sig_to_image_d", f"{tag} {S} -> {y_t}x{x_t}", t64, t32, f"f64 {mb:.1f} MB, {mb * 1e6 / (t64 * 1e-6) / 1e12:.2f} TB/s")
    d64, d32 = V(ctx.dev_alloc(8 * 600 * 800)), V(ctx.dev_alloc(4 * 600 * 800))
    row("downgrade_d", f"{tag} {y_t}x{x_t} -> 600x800", timed(lambda: chk(L.tsdr_downgrade_f64_d(h, i64, y_t, x_t, d64))),
        timed(lambda: chk(L.tsdr_downgrade_d(h, i32, y_t, x_t, d32))))

# vsync at 600 x 800 and 1125 x 2576
for y_t, x_t in [(600, 800), (1125, 2576)]:
    p64, p32 = C.c_void_p(0), C.c_void_p(0)
    chk(L.tsdr_sync_create_f64(h, y_t, x_t, C.byref(p64)))
    chk(L.tsdr_sync_create(h, y_t, x_t, C.byref(p32)))
    m64, m32 = dev(rng.random((y_t, x_t))), dev(rng.random((y_t, x_t), dtype=np.float32))
    idx = V(ctx.dev_alloc(16))
    row("vsync_d", f"{y_t}x{x_t}", timed(lambda: chk(L.tsdr_vsync_f64_d(p64, m64, idx))), timed(lambda: chk(L.tsdr_vsync_d(p32, m32, idx))))
    L.tsdr_sync_free(p64)
    L.tsdr_sync_free(p32)

# autocorrelation: n = 4e6 (2^8 5^6) and 3e6, and a Bluestein length
nout = C.c_size_t(0)
for Fs, md, ln, tag in [(20e6, 0.1, 5_000_000, "n=4e6"), (20e6, 0.1, 3_000_000, "n=3e6"), (1e6, 0.06, 100_003, "n=100003 (Bluestein)")]:
    x64, x32 = dev(rng.random(ln)), dev(rng.random(ln, dtype=np.float32))
    cnt = int(round(md * Fs))
    a64, a32 = V(ctx.dev_alloc(8 * cnt)), V(ctx.dev_alloc(4 * cnt))
    row("autocorr_d", tag, timed(lambda: chk(L.tsdr_autocorr_f64_d(h, x64, ln, Fs, 0.0, md, 1, a64, C.byref(nout)))),
        timed(lambda: chk(L.tsdr_autocorr_d(h, x32, ln, Fs, 0.0, md, 1, a32, C.byref(nout)))))

# getSpectrum at N = 80 000 (complex input, the replay's amplitude is real: both)
N = 80_000
for cplx in (0, 1):
    k = 2 if cplx else 1
    q64, q32 = dev(rng.random(k * N)), dev(rng.random(k * N, dtype=np.float32))
    y64, y32 = V(ctx.dev_alloc(8 * N)), V(ctx.dev_alloc(4 * N))
    row("spectrum_d", f"N=80000 {'complex' if cplx else 'real'}", timed(lambda: chk(L.tsdr_spectrum_f64_d(h, q64, cplx, N, 0, y64))),
        timed(lambda: chk(L.tsdr_spectrum_d(h, q32, cplx, N, 0, y32))))

# getWelch / getWaterfall on a C2 capture (1e7 ComplexF64 samples: 160 MB read), the resampler at test_resampler.jl's size and
# at 1e6 x 4.  Bytes are the algorithmic ones: the input once, the output once.
n = 10_000_000
for N in (1024, 1000):
    y64, y32 = V(ctx.dev_alloc(8 * N)), V(ctx.dev_alloc(4 * N))
    t64 = timed(lambda: chk(L.tsdr_welch_f64_d(h, z64, 1, n, N, 0, y64)))
    t32 = timed(lambda: chk(L.tsdr_welch_d(h, z32, 1, n, N, 0, y32)))
    row("welch_d", f"1e7 complex, sizeFFT {N}", t64, t32, f"f64 {16 * n / (t64 * 1e-6) / 1e12:.2f} TB/s")
nw = 3_000_000
for N in (1024, 1000):
    m64 = V(ctx.dev_alloc(8 * nw))
    t64 = timed(lambda: chk(L.tsdr_waterfall_f64_d(h, z64, 1, nw, N, m64)))
    t32 = timed(lambda: chk(L.tsdr_waterfall_d(h, z32, 1, nw, N, m64)))
    row("waterfall_d", f"3e6 complex, sizeFFT {N}", t64, t32, f"f64 {(16 + 8) * nw / (t64 * 1e-6) / 1e12:.2f} TB/s")
for bs, up in [(1024, 4), (1_000_000, 4), (1000, 4), (999, 3)]:
    r64, r32 = C.c_void_p(0), C.c_void_p(0)
    chk(L.tsdr_resampler_init_f64(h, bs, up, C.byref(r64)))
    chk(L.tsdr_resampler_init(h, bs, up, C.byref(r32)))
    i64, i32 = dev(rng.standard_normal(bs)), dev(rng.standard_normal(bs).astype(np.float32))
    o64, o32 = V(ctx.dev_alloc(8 * bs * up)), V(ctx.dev_alloc(4 * bs * up))
    t64 = timed(lambda: chk(L.tsdr_resampler_run_f64_d(r64, i64, bs, o64)))
    t32 = timed(lambda: chk(L.tsdr_resampler_run_d(r32, i32, bs, o32)))
    row("resampler_run_d", f"({bs}, {up})", t64, t32)
    L.tsdr_resampler_free(r64)
    L.tsdr_resampler_free(r32)

info = ctx.device_info()
print(json.dumps({"device": info["name"], "reps": args.reps, "rows": rows}))
if args.json:
    with open(args.json, "w") as f:
        json.dump({"device": info["name"], "reps": args.reps, "rows": rows}, f, indent=1)
