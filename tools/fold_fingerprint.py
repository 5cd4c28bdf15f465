"""SHA-256 of every output of frame folding (include/tempest_hip_fold.h, include/tempest_hip_cfold.h) at the geometries U, M, D, S,
R, X of tests/test_fold_gpu.py and tests/test_cfold_gpu.py: the fold's state at alpha 0 and at alpha 0.25 from a fixed state, and the
scan's scores (9 trials of the envelope scan, 19 of the coherent one: two batches and a ragged third), for cf32, sc16, sc8 and uc8
input, through the device-pointer and the host forms.  A refactor of the kernels leaves every digest as it was.

Inputs come from integer arithmetic alone (a 64-bit LCG in numpy.uint64; the integer formats are filled directly, cf32 is the sc16
stream divided by 32768), so the digests depend on no library's RNG or libm.  Two builds compare on one machine:
    TSDR_HIP_LIB=<the other build's libtempest_hip.so> python tools/fold_fingerprint.py before.json
    python tools/fold_fingerprint.py after.json  &&  cmp before.json after.json"""
import ctypes as C
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tempest_loader import load_package  # noqa: E402

GEOM = {
    "U": dict(y=70, x=150, T=1207.73, F=7, t0=3.25),
    "M": dict(y=66, x=160, T=9150.37, F=5, t0=0.0),
    "D": dict(y=77, x=131, T=11600.61, F=4, t0=11599.9),
    "S": dict(y=20, x=140, T=5180.3, F=3, t0=1.5),
    "R": dict(y=20, x=140, T=5195.3, F=3, t0=1.5),
    "X": dict(y=8, x=16, T=5000.5, F=3, t0=0.5),
}
CFOLD_T = {"S": 2550.3, "R": 2565.3}     # the coherent fold's boundary cases (TSDR_CFOLD_STAGE_MAX = 120)
SCALE = {"cf32": 1.0, "sc16": 1.0 / 32768, "sc8": 1.0 / 128, "uc8": 1.0 / 128}
DT, N_FOLD_TRIALS, N_CFOLD_TRIALS = 0.25, 9, 19
KAPPA = 0.671875                         # exact in binary; near the test captures' 2/3
ALPHA = 0.25


def lcg(count, seed):
    """x[k] = A^(k+1) seed + C (A^k + ... + 1) mod 2^64 (Knuth's MMIX constants), all of them at once; uint64 wraps"""
    a, c = np.uint64(6364136223846793005), np.uint64(1442695040888963407)
    with np.errstate(over="ignore"):
        pw = np.cumprod(np.full(count, a, np.uint64))                        # A^1 .. A^count
        geo = np.concatenate([np.ones(1, np.uint64), pw[:-1]]).cumsum(dtype=np.uint64)   # 1, 1 + A, ...
        return pw * np.uint64(seed) + c * geo


def inputs(n, seed):
    """fmt -> the array the API takes: 2n components of the LCG's top bits; cf32 is the sc16 stream / 32768 (exact)"""
    bits = lcg(2 * n, seed)
    sc16 = (bits >> np.uint64(48)).astype(np.uint16).view(np.int16)
    sc8 = (bits >> np.uint64(56)).astype(np.uint8).view(np.int8)
    uc8 = (bits >> np.uint64(40)).astype(np.uint8)
    cf32 = (sc16.astype(np.float32) / np.float32(32768)).view(np.complex64)
    return {"cf32": cf32, "sc16": sc16, "sc8": sc8, "uc8": uc8}


def main():
    ctx = load_package().Context(0)
    digests = {}

    def put(key, arr):
        digests[key] = hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()

    for kind in ("fold", "cfold"):
        for gi, (name, g) in enumerate(GEOM.items()):
            y, x, F, t0 = g["y"], g["x"], g["F"], g["t0"]
            T = CFOLD_T.get(name, g["T"]) if kind == "cfold" else g["T"]
            P = y * x
            n = int(math.ceil(t0 + F * (T + 2.0))) + 5
            n += n % 2                                               # whole words of the 8-bit formats
            state0 = ((lcg(P, 1000 + gi) >> np.uint64(40)).astype(np.float32) / np.float32(2.0 ** 30))   # [0, 2^-6)
            if kind == "fold":
                nt, T0 = N_FOLD_TRIALS, T - (N_FOLD_TRIALS - 1) * DT     # the largest trial is T: the fold's kernel choice
                fold_d = lambda iq, f, s, a, st: ctx.fold_d(iq, f, s, n, t0, T, F, y, x, a, st)                       # noqa: E731
                fold_h = lambda iq, f, s, a, st: ctx.fold(iq, t0, T, F, y, x, a, st, f, s)                            # noqa: E731
                scan_d = lambda iq, f, s, sc: ctx.fold_scan_d(iq, f, s, n, t0, T0, DT, nt, F, y, x, sc)               # noqa: E731
                scan_h = lambda iq, f, s: ctx.fold_scan(iq, t0, T0, DT, nt, F, y, x, f, s)                            # noqa: E731
            else:
                nt, dk = N_CFOLD_TRIALS, 1.0 / (8 * F)
                k0 = KAPPA - (nt // 2) * dk
                fold_d = lambda iq, f, s, a, st: ctx.cfold_d(iq, f, s, n, t0, T, KAPPA, F, y, x, a, st)               # noqa: E731
                fold_h = lambda iq, f, s, a, st: ctx.cfold(iq, t0, T, KAPPA, F, y, x, a, st, f, s)                    # noqa: E731
                scan_d = lambda iq, f, s, sc: ctx.cfold_scan_d(iq, f, s, n, t0, T, k0, dk, nt, F, y, x, sc)           # noqa: E731
                scan_h = lambda iq, f, s: ctx.cfold_scan(iq, t0, T, k0, dk, nt, F, y, x, f, s)                        # noqa: E731
            for fmt, arr in inputs(n, 1 + gi).items():
                scale = SCALE[fmt]
                key = f"{kind}/{name}/{fmt}"
                d_iq, d_st, d_sc = ctx.upload(arr), ctx.dev_alloc(4 * P), ctx.dev_alloc(8 * nt)
                for alpha in (0.0, ALPHA):
                    ctx.call("tsdr_upload", C.c_void_p(d_st), C.c_void_p(state0.ctypes.data), state0.nbytes)
                    fold_d(d_iq, fmt, scale, alpha, d_st)
                    ctx.synchronize()
                    put(f"{key}/state_d/alpha{alpha}", ctx.download(d_st, (P,), np.float32))
                    put(f"{key}/state_host/alpha{alpha}", fold_h(arr, fmt, scale, alpha, state0.reshape((y, x), order="F")).reshape(-1, order="F"))
                scan_d(d_iq, fmt, scale, d_sc)
                ctx.synchronize()
                put(f"{key}/score_d", ctx.download(d_sc, (nt,), np.float64))
                scores, best = scan_h(arr, fmt, scale)
                put(f"{key}/score_host", np.append(np.asarray(scores, np.float64), float(best)))
                for p in (d_iq, d_st, d_sc):
                    ctx.dev_free(p)
    text = json.dumps({"device": ctx.device_info()["name"], "sha256": digests}, indent=0, sort_keys=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    print(f"{len(digests)} outputs, digest of digests {hashlib.sha256(text.encode()).hexdigest()[:16]}")


if __name__ == "__main__":
    main()
