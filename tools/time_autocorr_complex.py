# Measures the complex autocorrelation search (tsdr_autocorr_cplx_search_iq_d) at one window length for ComplexF32 and sc8 input,
# next to the existing power search (tsdr_autocorr_search_iq_d) on the same samples in the same process: per-search wall time from
# tsdr_timer_* around alternating blocks of searches, and the per-kernel split from tsdr_profile_* in a separate block.
#
#     python tools/time_autocorr_complex.py [n = 4000000] [out.json]
#
# Prints one JSON document (and writes it to out.json when given).  GPU box only.
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tempest_loader import load_package  # noqa: E402

T = load_package()
ctx = T.Context()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
Fs, delay = 20e6 * n / 4_000_000, 0.1           # indexMax = n / 2: the search's own window, n = 2 indexMax
cnt = n // 2
lo, wc = int(round(Fs / 90)) - 1, int(round(Fs / 50)) - int(round(Fs / 90)) + 1   # zoom_autocorr(rate_min = 50, rate_max = 90)

rng = np.random.default_rng(1)
m = np.arange(n)
z = (((1 + 0.5j) + 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))) * np.exp(2j * np.pi * 37 * m / n) * 3e-3).astype(np.complex64)
sc = float(np.abs(z.view(np.float32)).max()) / 127.0
q = np.clip(np.round(z.view(np.float32) / sc), -127, 127).astype(np.int8)
d_z, d_q = ctx.upload(z), ctx.upload(q)
d_out = ctx.dev_alloc(4 * cnt)
n_out, idx, val = C.c_size_t(0), C.c_size_t(0), C.c_float(0)


def search(sym, ptr, code, scale):
    ctx.call(sym, C.c_void_p(ptr), code, C.c_float(scale), n, Fs, 0.0, delay, 1, C.c_void_p(d_out), C.byref(n_out), lo, wc, C.byref(idx),
             C.byref(val))
    return int(idx.value)


CASES = {"complex_cf32": ("tsdr_autocorr_cplx_search_iq_d", d_z, 0, 1.0), "complex_sc8": ("tsdr_autocorr_cplx_search_iq_d", d_q, 2, sc),
         "power_cf32": ("tsdr_autocorr_search_iq_d", d_z, 0, 1.0), "power_sc8": ("tsdr_autocorr_search_iq_d", d_q, 2, sc)}
REPS, ROUNDS = 20, 7
res = {"n": n, "Fs": Fs, "lags": cnt, "window": [lo, wc], "device": ctx.device_info()["name"], "reps_per_block": REPS, "rounds": ROUNDS,
       "cases": {}}
for name, args in CASES.items():      # warm every shape: code objects, workspaces, twiddle tables
    for _ in range(3):
        pos = search(*args)
    res["cases"][name] = {"pos": pos, "us_per_search_blocks": []}
for _ in range(ROUNDS):               # alternate the cases so that drift hits them alike
    for name, args in CASES.items():
        ctx.timer_start()
        for _ in range(REPS):
            search(*args)
        res["cases"][name]["us_per_search_blocks"].append(round(ctx.timer_stop() / REPS * 1e3, 2))
for name, c in res["cases"].items():
    b = c["us_per_search_blocks"]
    c["us_per_search_median"], c["us_per_search_min"], c["us_per_search_max"] = statistics.median(b), min(b), max(b)
for name, args in CASES.items():      # per-kernel split, in a block of its own (the event pairs slow the stream down)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(10):
        search(*args)
    ctx.synchronize()
    res["cases"][name]["kernels_us_per_search"] = {k: round(v["total_ms"] / 10 * 1e3, 2) for k, v in sorted(ctx.profile_results().items())}
    ctx.profile(False)
# bytes the algorithm needs per search: the samples once, the lags once (a lower bound: every pass of a transform moves 16 n more)
bps = {"complex_cf32": 8, "complex_sc8": 2, "power_cf32": 8, "power_sc8": 2}
for name, c in res["cases"].items():
    c["min_bytes"] = n * bps[name] + 4 * cnt
ctx.dev_free(d_z), ctx.dev_free(d_q), ctx.dev_free(d_out)
doc = json.dumps(res, indent=1)
print(doc)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    open(sys.argv[2], "w").write(doc + "\n")
