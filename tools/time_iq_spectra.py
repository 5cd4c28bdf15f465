"""getWelch / getWaterfall on the C2 buffer (10^7 samples, sizeFFT 1024: 9765 segments on the wavefront-per-segment kernel) for
ComplexF32 input (tsdr_welch_d / tsdr_waterfall_d) and for integer IQ read as stored (tsdr_welch_iq_d / tsdr_waterfall_iq_d on
sc16, sc8, uc8): stream time per call between HIP events, --reps calls per measurement after a warm-up, min / median / max over
--rounds measurements with the formats alternating inside every round.  One JSON line.

The library is bound here directly (not through the package), so that a build from before the `_iq_d` entry points can be timed
with the same tool: TSDR_HIP_LIB=<other libtempest_hip.so> python tools/time_iq_spectra.py -- its integer legs are then absent.
Alternate the two libraries on one box (as tools/ab.sh does for bench.py); a single run of each on different boxes differs by the
+-5 % box spread.
   python tools/time_iq_spectra.py [--n 10000000] [--size 1024] [--reps 20] [--rounds 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import iq8_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

path = os.environ.get("TSDR_HIP_LIB") or os.path.join(ROOT, "tempestsdr.jl_amd", "libtempest_hip.so")
lib = C.CDLL(path)
vp, sz = C.c_void_p, C.c_size_t
lib.tsdr_create.restype, lib.tsdr_create.argtypes = vp, [C.c_int]
lib.tsdr_destroy.restype, lib.tsdr_destroy.argtypes = None, [vp]
lib.tsdr_dev_alloc.restype, lib.tsdr_dev_alloc.argtypes = vp, [vp, sz]
lib.tsdr_dev_free.argtypes = [vp, vp]
lib.tsdr_upload.argtypes = [vp, vp, vp, sz]
lib.tsdr_synchronize.argtypes = [vp]
lib.tsdr_timer_start.argtypes = [vp]
lib.tsdr_timer_stop.argtypes = [vp, C.POINTER(C.c_double)]
lib.tsdr_last_error.restype, lib.tsdr_last_error.argtypes = C.c_char_p, [vp]
lib.tsdr_welch_d.argtypes = [vp, vp, C.c_int, sz, sz, C.c_int, vp]
lib.tsdr_waterfall_d.argtypes = [vp, vp, C.c_int, sz, sz, vp]
have_iq = hasattr(lib, "tsdr_welch_iq_d")
if have_iq:
    lib.tsdr_welch_iq_d.argtypes = [vp, vp, C.c_int, C.c_float, sz, sz, C.c_int, vp]
    lib.tsdr_waterfall_iq_d.argtypes = [vp, vp, C.c_int, C.c_float, sz, sz, vp]

ctx = lib.tsdr_create(0)
if not ctx:
    sys.exit("time_iq_spectra: no HIP device")


def ok(rc, what):
    if rc:
        sys.exit(f"time_iq_spectra: {what} failed ({rc}): {lib.tsdr_last_error(ctx).decode()}")


def upload(a):
    a = np.ascontiguousarray(a)
    p = lib.tsdr_dev_alloc(ctx, a.nbytes)
    if not p:
        sys.exit("time_iq_spectra: out of device memory")
    ok(lib.tsdr_upload(ctx, p, a.ctypes.data, a.nbytes), "upload")
    return p


n, size = args.n, args.size
rng = np.random.default_rng(1)
z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
bufs = {"cf32": (upload(z.view(np.float32)), 1.0)}
if have_iq:
    for fmt in ("sc16", "sc8", "uc8"):
        q, scale = R.quantise(z, fmt)
        bufs[fmt] = (upload(q), float(scale))
d_y = lib.tsdr_dev_alloc(ctx, size * 4)
d_m = lib.tsdr_dev_alloc(ctx, (n // size) * size * 8)


def call(kind, fmt):
    p, scale = bufs[fmt]
    if kind == "welch":
        if fmt == "cf32":
            return lib.tsdr_welch_d(ctx, p, 1, n, size, 0, d_y)
        return lib.tsdr_welch_iq_d(ctx, p, R.CODES[fmt], scale, n, size, 0, d_y)
    if fmt == "cf32":
        return lib.tsdr_waterfall_d(ctx, p, 1, n, size, d_m)
    return lib.tsdr_waterfall_iq_d(ctx, p, R.CODES[fmt], scale, n, size, d_m)


samples = {}
for rnd in range(args.rounds + 1):          # (round 0 warms up)
    for kind in ("welch", "waterfall"):
        for fmt in bufs:
            ok(lib.tsdr_timer_start(ctx), "timer")
            for _ in range(args.reps):
                ok(call(kind, fmt), f"{kind} {fmt}")
            ms = C.c_double(0)
            ok(lib.tsdr_timer_stop(ctx, C.byref(ms)), "timer")
            if rnd:
                samples.setdefault(kind, {}).setdefault(fmt, []).append(1e3 * ms.value / args.reps)
res = {"lib": os.path.relpath(path, ROOT), "n": n, "sizeFFT": size, "segments": n // size, "reps": args.reps, "rounds": args.rounds}
for kind, per in samples.items():
    res[kind] = {fmt: {"us_min": round(min(v), 2), "us_median": round(float(np.median(v)), 2), "us_max": round(max(v), 2)}
                 for fmt, v in per.items()}
for p, _ in bufs.values():
    lib.tsdr_dev_free(ctx, p)
lib.tsdr_dev_free(ctx, d_y)
lib.tsdr_dev_free(ctx, d_m)
lib.tsdr_destroy(ctx)
print(json.dumps(res), flush=True)
