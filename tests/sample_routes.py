"""The calls whose launch sequence tests/test_sample_routes_gpu.py pins and whose output bits tools/sample_fingerprint.py
hashes: the spectra, tsdr_fft_c2c_d, the demodulators and the autocorrelations on every sample source (real f32, ComplexF32,
sc16, sc8, uc8), one tiny call per transform route.  A case is (id, prepare); prepare(ctx) uploads seeded inputs and returns
(call, fetch, free): call() makes the ONE library call and returns its status, fetch() downloads the outputs."""
import ctypes as C
import functools

import numpy as np

import iq8_ref as R
from test_iq_spectra_gpu import ROUTES

SOURCES = ["real", "cf32", "sc16", "sc8", "uc8"]
IQ = SOURCES[1:]
INTS = SOURCES[2:]


@functools.lru_cache(maxsize=None)
def _noise(n):
    rng = np.random.default_rng(4242 + n % 101)
    t = np.arange(n, dtype=np.float64)
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n) + 3.0 * np.exp(2j * np.pi * 0.1234 * t)
    return z.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def samples(src, n):
    """-> (array as stored, scale, bytes per sample)"""
    z = _noise(max(n, 1))
    if src == "real":
        a, scale, nb = np.ascontiguousarray(z.real), 1.0, 4
    elif src == "cf32":
        a, scale, nb = z.view(np.float32), 1.0, 8
    else:
        a, scale = R.quantise(z, src)
        nb = R.BYTES[src]
    a.setflags(write=False)
    return a, float(scale), nb


def _upload(ctx, src, n, lead=0):
    """the n samples behind `lead` junk samples, padded to whole words -> (base, pointer to the first sample, scale)"""
    a, scale, nb = samples(src, n)
    per = a.size // max(n, 1)
    buf = np.concatenate([np.full(lead * per, 55, a.dtype), a])
    if buf.nbytes % 4:
        buf = np.concatenate([buf, np.full(2, 55, a.dtype)])
    base = ctx.upload(buf)
    return base, base + lead * nb, scale


def _prepared(ctx, bufs, outs, call):
    """bufs: device allocations; outs: [(pointer, count, dtype)] downloaded after a synchronize"""
    def fetch():
        ctx.synchronize()
        return [ctx.download(p, (cnt,), dt) for p, cnt, dt in outs if cnt]

    def free():
        ctx.synchronize()
        for p in bufs:
            ctx.dev_free(p)
    return call, fetch, free


def _spectra(kind, src, n, size, lin):
    def prepare(ctx):
        base, p, scale = _upload(ctx, src, n)
        cnt, dt = (n, np.uint32) if kind == "spectrum" else (size, np.uint32) if kind == "welch" else (size * (n // size), np.uint64)
        out = ctx.dev_alloc(max(cnt, 1) * np.dtype(dt).itemsize)
        tail = (n, lin) if kind == "spectrum" else (n, size, lin) if kind == "welch" else (n, size)
        if src in INTS:
            f, head = getattr(ctx.lib, f"tsdr_{kind}_iq_d"), (C.c_void_p(p), R.CODES[src], C.c_float(scale))
        else:
            f, head = getattr(ctx.lib, f"tsdr_{kind}_d"), (C.c_void_p(p), int(src == "cf32"))
        return _prepared(ctx, [base, out], [(out, cnt, dt)], lambda: f(ctx.h, *head, *tail, C.c_void_p(out)))
    return prepare


def _fft(n, batch, direction):
    def prepare(ctx):
        base, p, _ = _upload(ctx, "cf32", n * batch)
        out = ctx.dev_alloc(8 * n * batch)
        return _prepared(ctx, [base, out], [(out, n * batch, np.uint64)],
                         lambda: ctx.lib.tsdr_fft_c2c_d(ctx.h, C.c_void_p(p), C.c_void_p(out), n, batch, direction))
    return prepare


def _resampler(buffer_size, up):
    """resampler!(out, in) with `in` 4 bytes off 8-byte alignment: the half-size route needs both pointers on 8 bytes, so this is
    the full-size one -- two transforms of sizeFFT = buffer_size * up points, the zero-stuffing and the filter in their loaders"""
    def prepare(ctx):
        base, p, _ = _upload(ctx, "real", buffer_size, 1)
        n = buffer_size * up
        out = ctx.dev_alloc(4 * n)
        h = C.c_void_p(0)
        rc = ctx.lib.tsdr_resampler_init(ctx.h, buffer_size, up, C.byref(h))
        assert rc == 0, (rc, ctx.lib.tsdr_last_error(ctx.h).decode())
        call, fetch, free_ = _prepared(ctx, [base, out], [(out, n, np.uint32)],
                                       lambda: ctx.lib.tsdr_resampler_run_d(h, C.c_void_p(p), buffer_size, C.c_void_p(out)))

        def free():
            free_()
            ctx.lib.tsdr_resampler_free(h)
        return call, fetch, free
    return prepare


def _demod(kind, src, n, lead):
    def prepare(ctx):
        base, p, scale = _upload(ctx, src, n, lead)
        out = ctx.dev_alloc(4 * n)
        f = getattr(ctx.lib, f"tsdr_{kind}_iq_d")
        return _prepared(ctx, [base, out], [(out, n, np.uint32)],
                         lambda: f(ctx.h, C.c_void_p(p), R.CODES[src], C.c_float(scale), n, C.c_void_p(out)))
    return prepare


def _lags(n):
    """(Fs, minDelay, maxDelay) with which a len-n call correlates all n samples: n = min(2 * indexMax, len)"""
    return 1.0, 0.0, float((n + 1) // 2)


def _search(name, src, n, window):
    """name: 'autocorr_cplx_search_iq' (any IQ source), 'autocorr_search_iq' (abs2 of an IQ source), 'autocorr_search' (real f32
    or abs2 of ComplexF32).  window: findmax over the middle half of the lags, else none (the plain device call)"""
    def prepare(ctx):
        base, p, scale = _upload(ctx, src, n)
        fs, lo, hi = _lags(n)
        cnt = (n + 1) // 2
        out = ctx.dev_alloc(4 * cnt)
        n_out, idx, val = C.c_size_t(0), C.c_size_t(0), C.c_float(0.0)
        win = (cnt // 4, cnt // 2) if window else (0, 0)
        head = (C.c_void_p(p), int(src != "real")) if name == "autocorr_search" else (C.c_void_p(p), R.CODES[src], C.c_float(scale))
        f = getattr(ctx.lib, f"tsdr_{name}_d")

        def call():
            return f(ctx.h, *head, n, fs, lo, hi, 1, C.c_void_p(out), C.byref(n_out), *win, C.byref(idx), C.byref(val))
        call_, fetch_, free = _prepared(ctx, [base, out], [(out, cnt, np.uint32)], call)

        def fetch():
            got = fetch_()
            assert n_out.value == cnt, (n_out.value, cnt)
            return got + ([np.array([idx.value], np.uint64), np.array([val.value], np.float32).view(np.uint32)] if window else [])
        return call_, fetch, free
    return prepare


def cases():
    out = []
    for src in SOURCES:
        for kind, n, size in ROUTES:
            out.append((f"{kind}-{src}-{n}-{size}", _spectra(kind, src, n, size, 0)))
        out.append((f"welch-{src}-{7 * 1000 + 5}-1000-lin", _spectra("welch", src, 7 * 1000 + 5, 1000, 1)))
    for n, batch in ((1024, 5), (1000, 5), (64, 5), (8192, 2), (1031, 2)):
        for direction in (-1, 1):
            out.append((f"fft_c2c-{n}x{batch}-dir{direction:+d}", _fft(n, batch, direction)))
    for kind in ("am_demod", "abs2", "invert_am", "fm_demod"):
        for src in IQ:
            out.append((f"{kind}-{src}-4099-aligned", _demod(kind, src, 4099, 0)))
            out.append((f"{kind}-{src}-4099-sample1", _demod(kind, src, 4099, 1)))
    for n in (200, 1000, 4001, 4096):
        for src in IQ:
            out.append((f"autocorr_cplx-{src}-{n}", _search("autocorr_cplx_search_iq", src, n, False)))
            out.append((f"autocorr_cplx_search-{src}-{n}", _search("autocorr_cplx_search_iq", src, n, True)))
    for n in (4096, 3000):
        for src in ("real", "cf32"):
            out.append((f"autocorr_search-{src}-{n}", _search("autocorr_search", src, n, True)))
    for src in INTS:
        out.append((f"autocorr_search_iq-{src}-4096", _search("autocorr_search_iq", src, 4096, True)))
    for buffer_size, up in ((256, 2), (100, 3)):   # sizeFFT 512 = 32 x 16 and 300 = 25 x 12: two passes on either engine
        out.append((f"resampler-{buffer_size}x{up}-in4", _resampler(buffer_size, up)))
    return out


def run(ctx, prepare, around=None):
    """one case -> its outputs; `around` (a context manager factory) brackets the one library call.  The same call is made once
    before, unbracketed: what a context builds at the first use of a length (a Bluestein plan, a twiddle table) and keeps is
    launched there, so the bracketed call is the steady one whatever ran on the context earlier."""
    call, fetch, free = prepare(ctx)
    try:
        rc = call()
        assert rc == 0, (rc, ctx.lib.tsdr_last_error(ctx.h).decode())
        if around is None:
            rc = call()
        else:
            with around():
                rc = call()
        assert rc == 0, (rc, ctx.lib.tsdr_last_error(ctx.h).decode())
        return fetch()
    finally:
        free()
