"""Host-side mirror of TempestSDR.jl's processing API over the HIP C ABI.

Same function names, argument meaning and error behaviour as the reference's
Demodulation.jl / Resampler.jl / Autocorrelations.jl / GetSpectrum.jl /
FrameSynchronisation.jl, so tests read like the reference's own call sites
(GUI.jl:73-74,136,164,168,171; production/investigate_data.jl).  Matrices are Fortran-order
numpy arrays (Julia is column-major); complex vectors are complex64 (ComplexF32).

Every function runs on the GPU through libtempest_hip.so; nothing here computes on the CPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import RENDER_H, RENDER_W, TempestHIPError, check


def _ptr(a):
    """host numpy array, torch tensor (device or host) or raw integer address -> c_void_p"""
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    if isinstance(a, int):
        return C.c_void_p(a)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    raise TypeError(f"cannot take the address of {type(a)}")


def _c64(sig):
    a = np.ascontiguousarray(sig)
    if not np.iscomplexobj(a):
        # amDemod(sig::Array{Complex{T}}): a real array is a MethodError in the reference
        raise AssertionError("expected a complex vector (MethodError in the reference)")
    return a.astype(np.complex64, copy=False)


def _f32(sig):
    return np.ascontiguousarray(sig, dtype=np.float32)


def _is64(dtype):
    """the `dtype=` keyword of the per-function API: None (today's Float32 path, input converted to f32) or np.float64
    (the `_f64` entry points; Float64 / ComplexF64 input only)"""
    if dtype is None:
        return False
    if np.dtype(dtype) == np.float64:
        return True
    raise AssertionError(f"dtype must be None or numpy.float64 (got {dtype}; MethodError in the reference)")


def _need(a, dtype, what):
    """Float64 entry points take exactly their element type: no silent conversion either way (the MethodError analogue)"""
    if not isinstance(a, np.ndarray) or a.dtype != dtype:
        raise AssertionError(f"{what}: expected a {np.dtype(dtype).name} array, got "
                             f"{getattr(a, 'dtype', type(a))} (MethodError in the reference)")
    return a


def _c128(sig, what):
    return np.ascontiguousarray(_need(sig, np.complex128, what))


def _f64(sig, what):
    return np.ascontiguousarray(_need(sig, np.float64, what))


class Context:
    """One tsdr_ctx (HIP stream + workspaces).  One per caller thread, as in the reference's
    two-task layout."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        self.h = self.lib.tsdr_create(int(device))
        if not self.h:
            raise TempestHIPError(f"tsdr_create({device}) failed: no usable HIP device (no CPU fallback exists)")
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsdr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing -------------------------------------------------------------------
    def call(self, name, *args):
        rc = getattr(self.lib, name)(self.h, *args)
        check(self.h, rc, name)

    def synchronize(self):
        self.call("tsdr_synchronize")

    def set_precision(self, mode):
        """'exact' (bit-identical to the oracle) or 'fast' (within 1 ulp, default) -- tsdr_set_precision"""
        self.call("tsdr_set_precision", {"exact": _lib.EXACT, "fast": _lib.FAST}[mode])

    @property
    def precision(self):
        return "exact" if self.lib.tsdr_get_precision(self.h) == _lib.EXACT else "fast"

    def set_option(self, name, value):
        """switches ("ac_mixed", "fft_no_mix2", "sync_guard_ppb", "sync_guard_auto", "vsync_blank_dark", ...) -- tsdr_set_option"""
        self.call("tsdr_set_option", name.encode(), int(value))

    def sync_guard_stats(self, reset=False):
        """running totals of the FAST frame loop's sync guard: (frames checked, frames flagged = computed exactly)"""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        self.call("tsdr_sync_guard_stats", C.byref(a), C.byref(b), int(bool(reset)))
        return int(a.value), int(b.value)

    def sync_guard_auto(self):
        """adaptive route of the sync guard: (whole buffers run exactly right now?, calls that did, route changes)"""
        e, a, b = C.c_int(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self.call("tsdr_sync_guard_auto", C.byref(e), C.byref(a), C.byref(b))
        return bool(e.value), int(a.value), int(b.value)

    def wait_stats(self):
        """(stream waits given up after "wait_ms", guard ring entries that went uncounted) on this context -- tsdr_wait_stats"""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        self.call("tsdr_wait_stats", C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def frames_overlap_stats(self, reset=False):
        """which route the frames_d / frames_sc16_d / frames_iq_d calls of this context took: (calls on the internal streams,
        calls on the context's stream, why the latest of those was sequential: bits 1 option or another context on the device,
        2 profiling, 4 'exact', 8 adopted stream).  Host-side counters -- tsdr_frames_overlap_stats"""
        a, b, w = C.c_ulonglong(0), C.c_ulonglong(0), C.c_uint(0)
        self.call("tsdr_frames_overlap_stats", C.byref(a), C.byref(b), C.byref(w), int(bool(reset)))
        return int(a.value), int(b.value), int(w.value)

    def debug_hold_tail(self, ms):
        """diagnostic: the tail of the next call that takes the internal streams starts `ms` milliseconds late (0 .. 1000, 0
        disarms) -- tsdr_debug_hold_tail"""
        self.call("tsdr_debug_hold_tail", int(ms))

    def pipeline_info(self):
        """what tsdr_frames_submit_d measured on this context: dict(trials_left, chosen, ms_per_buffer[8], text)"""
        left, chosen, ms, text = C.c_int(0), C.c_int(-1), (C.c_float * 8)(), C.create_string_buffer(1024)
        self.call("tsdr_frames_pipeline_info", C.byref(left), C.byref(chosen), ms, 8, text, 1024)
        txt = text.value.decode()
        import re
        m = re.search(r"measurements started on this context: (\d+)", txt)
        return {"trials_left": left.value, "chosen": chosen.value, "ms_per_buffer": [round(float(v), 5) for v in ms],
                "text": txt, "measurements_started": int(m.group(1)) if m else None}

    def sync_guard_margins(self, max_frames=1 << 16):
        """(frames, 2) relative top-2 margins (x, y) the guard saw in the last FAST frame-loop call"""
        n = C.c_int(0)
        self.call("tsdr_sync_guard_margins", 0, None, C.byref(n))
        nf = min(n.value, int(max_frames))
        m = np.zeros((nf, 2), np.float32)
        if nf:
            self.call("tsdr_sync_guard_margins", nf, _ptr(m), C.byref(n))
        return m

    def set_stream(self, stream_ptr):
        self.call("tsdr_set_stream", C.c_void_p(stream_ptr or 0))

    def device_info(self):
        name = C.create_string_buffer(256)
        cu = C.c_int(0)
        mem = C.c_size_t(0)
        self.call("tsdr_device_info", name, 256, C.byref(cu), C.byref(mem))
        return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value}

    # -- resident device buffers (for the *_d entry points) ----------------------------
    def dev_alloc(self, nbytes):
        p = self.lib.tsdr_dev_alloc(self.h, int(nbytes))
        if not p:
            raise MemoryError(self.lib.tsdr_last_error(self.h).decode())
        return p

    def dev_free(self, p):
        self.call("tsdr_dev_free", C.c_void_p(p))

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.dev_alloc(a.nbytes)
        self.call("tsdr_upload", C.c_void_p(p), _ptr(a), a.nbytes)
        return p

    def download(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        self.call("tsdr_download", _ptr(out), C.c_void_p(p), out.nbytes)
        return out

    def timer_start(self):
        self.call("tsdr_timer_start")

    def timer_stop(self):
        ms = C.c_double(0)
        self.call("tsdr_timer_stop", C.byref(ms))
        return ms.value

    def profile(self, on):
        self.call("tsdr_profile_enable", int(bool(on)))

    def profile_reset(self):
        self.call("tsdr_profile_reset")

    def profile_results(self):
        n = self.lib.tsdr_profile_count(self.h)
        if n < 0:
            check(self.h, n, "tsdr_profile_count")
        out = {}
        for i in range(n):
            name = C.create_string_buffer(128)
            ms = C.c_double(0)
            cnt = C.c_longlong(0)
            self.call("tsdr_profile_get", i, name, 128, C.byref(ms), C.byref(cnt))
            out[name.value.decode()] = {"total_ms": ms.value, "launches": cnt.value}
        return out

    # -- Demodulation.jl ----------------------------------------------------------------
    # iq_fmt "sc16" / "sc8" / "uc8" (keyword only, as autocorr_search): sig is integer IQ as the hardware stores it -- an int16 /
    # int8 / uint8 array of 2*n interleaved components (strict about the dtype); every sample is converted with iq_scale in the
    # kernel's loader, and the result has the bits of the same call on expand_iq(sig, iq_fmt, iq_scale).
    def _demod_iq(self, what, sym, sig, iq_fmt, iq_scale, dtype):
        if dtype is not None:
            raise AssertionError(f"{what}: iq_fmt is a Float32 path (dtype must be None)")
        a, code, n = _int_iq(sig, iq_fmt, what)
        out = np.empty(n, np.float32)
        if n == 0 and what != "invert_amDemod":
            return out
        d_in = self.upload(a) if n else 0
        d_out = None
        try:
            d_out = self.dev_alloc(max(n, 1) * 4)
            self.call(sym, C.c_void_p(d_in), code, C.c_float(iq_scale), n, C.c_void_p(d_out))
            return self.download(d_out, (n,), np.float32)
        finally:
            if d_in:
                self.dev_free(d_in)
            if d_out is not None:
                self.dev_free(d_out)

    def amDemod(self, sig, *, dtype=None, iq_fmt=None, iq_scale=1.0):
        if iq_fmt is not None:
            return self._demod_iq("amDemod", "tsdr_am_demod_iq_d", sig, iq_fmt, iq_scale, dtype)
        if _is64(dtype):
            z = _c128(sig, "amDemod")
            out = np.empty(z.shape, np.float64)
            self.call("tsdr_am_demod_f64", _ptr(z), z.size, _ptr(out))
            return out
        z = _c64(sig)
        out = np.empty(z.shape, np.float32)
        self.call("tsdr_am_demod", _ptr(z), z.size, _ptr(out))
        return out

    def invert_amDemod(self, sig, *, dtype=None, iq_fmt=None, iq_scale=1.0):
        if iq_fmt is not None:
            return self._demod_iq("invert_amDemod", "tsdr_invert_am_iq_d", sig, iq_fmt, iq_scale, dtype)
        if _is64(dtype):
            z = _c128(sig, "invert_amDemod")
            out = np.empty(z.shape, np.float64)
            self.call("tsdr_invert_am_f64", _ptr(z), z.size, _ptr(out))
            return out
        z = _c64(sig)
        out = np.empty(z.shape, np.float32)
        self.call("tsdr_invert_am", _ptr(z), z.size, _ptr(out))
        return out

    def fmDemod(self, sig, *, dtype=None, iq_fmt=None, iq_scale=1.0):
        if iq_fmt is not None:
            return self._demod_iq("fmDemod", "tsdr_fm_demod_iq_d", sig, iq_fmt, iq_scale, dtype)
        if _is64(dtype):
            z = _c128(sig, "fmDemod")
            out = np.empty(z.shape, np.float64)
            self.call("tsdr_fm_demod_f64", _ptr(z), z.size, _ptr(out))
            return out
        z = _c64(sig)
        out = np.empty(z.shape, np.float32)
        self.call("tsdr_fm_demod", _ptr(z), z.size, _ptr(out))
        return out

    def abs2(self, sig, *, dtype=None, iq_fmt=None, iq_scale=1.0):
        if iq_fmt is not None:
            return self._demod_iq("abs2", "tsdr_abs2_iq_d", sig, iq_fmt, iq_scale, dtype)
        if _is64(dtype):
            z = _c128(sig, "abs2")
            out = np.empty(z.shape, np.float64)
            self.call("tsdr_abs2_f64", _ptr(z), z.size, _ptr(out))
            return out
        z = _c64(sig)
        out = np.empty(z.shape, np.float32)
        self.call("tsdr_abs2", _ptr(z), z.size, _ptr(out))
        return out

    # -- Resampler.jl -------------------------------------------------------------------
    def imresize1d(self, sig, n_out, *, dtype=None):
        if _is64(dtype):
            x = _f64(sig, "imresize")
            out = np.empty(int(n_out), np.float64)
            self.call("tsdr_resize1d_f64", _ptr(x), x.size, int(n_out), _ptr(out))
            return out
        x = _f32(sig)
        out = np.empty(int(n_out), np.float32)
        self.call("tsdr_resize1d", _ptr(x), x.size, int(n_out), _ptr(out))
        return out

    def sig_to_image(self, sig, y_t, x_t, *, dtype=None):
        if _is64(dtype):
            x = _f64(sig, "sig_to_image")
            img = np.empty((int(y_t), int(x_t)), np.float64, order="F")
            self.call("tsdr_sig_to_image_f64", _ptr(x), x.size, int(y_t), int(x_t), _ptr(img))
            return img
        x = _f32(sig)
        img = np.empty((int(y_t), int(x_t)), np.float32, order="F")
        self.call("tsdr_sig_to_image", _ptr(x), x.size, int(y_t), int(x_t), _ptr(img))
        return img

    def imresize2d(self, image, size, *, dtype=None):
        if _is64(dtype):
            a = np.asfortranarray(_need(image, np.float64, "imresize"))
            h, w = int(size[0]), int(size[1])
            out = np.empty((h, w), np.float64, order="F")
            self.call("tsdr_resize2d_f64", _ptr(a), a.shape[0], a.shape[1], h, w, _ptr(out))
            return out
        a = np.asfortranarray(image, dtype=np.float32)
        h, w = int(size[0]), int(size[1])
        out = np.empty((h, w), np.float32, order="F")
        self.call("tsdr_resize2d", _ptr(a), a.shape[0], a.shape[1], h, w, _ptr(out))
        return out

    def downgradeImage(self, image, *, dtype=None):
        return self.imresize2d(image, (RENDER_H, RENDER_W), dtype=dtype)

    def naiveResampler(self, sigOut, sigId, upCoeff, *, dtype=None):
        if _is64(dtype):
            x = _f64(sigId, "naiveResampler")
            if not (isinstance(sigOut, np.ndarray) and sigOut.dtype == np.float64 and sigOut.flags.c_contiguous):
                raise AssertionError("sigOut must be a contiguous float64 array")
            if sigOut.size < x.size * int(upCoeff):
                raise IndexError("sigOut too short (BoundsError in the reference)")
            self.call("tsdr_naive_resample_f64", _ptr(x), x.size, int(upCoeff), _ptr(sigOut))
            return
        x = _f32(sigId)
        if not (isinstance(sigOut, np.ndarray) and sigOut.dtype == np.float32 and sigOut.flags.c_contiguous):
            raise AssertionError("sigOut must be a contiguous float32 array")
        if sigOut.size < x.size * int(upCoeff):
            raise IndexError("sigOut too short (BoundsError in the reference)")
        self.call("tsdr_naive_resample", _ptr(x), x.size, int(upCoeff), _ptr(sigOut))

    def init_resampler(self, T, bufferSize, upCoeff):
        """init_resampler(T,bufferSize,upCoeff) -> resampler!(out,in)  (Resampler.jl:26-62); T is Float32 or Float64"""
        if np.dtype(T) not in (np.float32, np.float64):
            raise AssertionError("only Float32 and Float64 resamplers are implemented on the GPU path")
        return Resampler(self, int(bufferSize), int(upCoeff), dtype=np.dtype(T))

    # -- Autocorrelations.jl --------------------------------------------------------------
    def calculate_autocorrelation(self, x, Fs, minDelay, maxDelay, scale="log", *, dtype=None, iq_fmt=None, iq_scale=1.0):
        """Real x: the autocorrelation of x (Float32, or Float64 with dtype=np.float64).  Complex x -- complex64, complex128
        with dtype=np.float64, or with iq_fmt "sc16" / "sc8" / "uc8" (keyword only) an int16 / int8 / uint8 array of 2*n
        interleaved components -- takes the complex route: the coherent autocorrelation of the IQ samples themselves
        (autocorr_cplx.py; the reference function is untyped, Autocorrelations.jl:23-37)."""
        if iq_fmt is not None or np.iscomplexobj(x):
            return autocorr_cplx.calculate(self, x, Fs, minDelay, maxDelay, scale, dtype=dtype, iq_fmt=iq_fmt, iq_scale=iq_scale)
        f64 = _is64(dtype)
        xv = _f64(x, "calculate_autocorrelation") if f64 else _f32(x)
        index_min = 1 + int(np.round(minDelay * Fs))
        index_max = int(np.round(maxDelay * Fs))
        cnt = max(index_max - index_min + 1, 0)
        out = np.empty(max(cnt, 1), np.float64 if f64 else np.float32)
        n_out = C.c_size_t(0)
        self.call("tsdr_autocorr_f64" if f64 else "tsdr_autocorr", _ptr(xv), xv.size, float(Fs), float(minDelay), float(maxDelay),
                  1 if scale == "log" else 0, _ptr(out), C.byref(n_out))
        lags = np.arange(0, index_max - index_min + 1, dtype=np.float64) * (1.0 / Fs)
        return out[: n_out.value], lags

    def autocorr_search(self, sig, Fs, minDelay, maxDelay, rate_min=50, rate_max=90, scale="log", *, iq_fmt=None, iq_scale=1.0,
                        n_samples=None):
        """calculate_autocorrelation + zoom_autocorr + findmax as ONE library call (tsdr_autocorr_search_d; GUI.jl:73-81).
        sig: real power samples, or complex IQ whose abs2 is formed on the fly (GUI.jl:70).
        iq_fmt "sc16" / "sc8" / "uc8" (keyword only): sig is integer IQ as the hardware stores it -- an int16 / int8 / uint8
        array of 2*n interleaved components (strict about the dtype), or the integer address of such a buffer on the device
        (16-byte aligned, e.g. from StagingRing.take_d) with n_samples = n; every sample is converted with iq_scale by the first
        pass's loader (tsdr_autocorr_search_iq_d).
        -> (G, pos, val): the lag vector, the 0-based findmax position inside the zoom window, its value."""
        d_in, own, code = None, True, 0
        if iq_fmt is None:
            a = np.ascontiguousarray(sig)
            is_iq = int(np.iscomplexobj(a))
            a = a.astype(np.complex64 if is_iq else np.float32, copy=False)
            n = a.size
        else:
            code = iq_fmt_code(iq_fmt)
            if code == 0:
                raise AssertionError("iq_fmt is for integer IQ (sc16, sc8, uc8); ComplexF32 goes in as a complex array")
            if isinstance(sig, (int, np.integer)) and not isinstance(sig, bool):
                if n_samples is None or int(n_samples) <= 0:
                    raise AssertionError("a device address needs n_samples")
                d_in, own, n = int(sig), False, int(n_samples)
            else:
                want = {1: np.int16, 2: np.int8, 3: np.uint8}[code]
                if not isinstance(sig, np.ndarray) or sig.dtype != want or sig.size % 2:
                    raise AssertionError(f"iq_fmt {iq_fmt!r} takes an {np.dtype(want).name} array of 2*n interleaved components")
                a = np.ascontiguousarray(sig)
                n = a.size // 2
        index_min = 1 + int(np.round(minDelay * Fs))
        index_max = int(np.round(maxDelay * Fs))
        cnt = max(index_max - index_min + 1, 0)
        pmin, pmax = C.c_size_t(0), C.c_size_t(0)
        check(self.h, self.lib.tsdr_zoom_bounds(cnt, float(Fs), float(rate_min), float(rate_max), C.byref(pmin), C.byref(pmax)),
              "tsdr_zoom_bounds")
        if d_in is None:
            d_in = self.upload(a)
        d_out = None
        try:
            d_out = self.dev_alloc(max(cnt, 1) * 4)
            n_out, idx, val = C.c_size_t(0), C.c_size_t(0), C.c_float(0)
            if iq_fmt is None:
                self.call("tsdr_autocorr_search_d", C.c_void_p(d_in), is_iq, n, float(Fs), float(minDelay), float(maxDelay),
                          1 if scale == "log" else 0, C.c_void_p(d_out), C.byref(n_out), int(pmin.value - 1),
                          int(pmax.value - pmin.value + 1), C.byref(idx), C.byref(val))
            else:
                self.call("tsdr_autocorr_search_iq_d", C.c_void_p(d_in), code, C.c_float(iq_scale), n, float(Fs), float(minDelay),
                          float(maxDelay), 1 if scale == "log" else 0, C.c_void_p(d_out), C.byref(n_out), int(pmin.value - 1),
                          int(pmax.value - pmin.value + 1), C.byref(idx), C.byref(val))
            G = self.download(d_out, (n_out.value,), np.float32)
        finally:
            if own:
                self.dev_free(d_in)
            if d_out is not None:
                self.dev_free(d_out)
        return G, int(idx.value), float(val.value)

    def autocorr_search_complex(self, sig, Fs, minDelay, maxDelay, rate_min=50, rate_max=90, scale="log", *, iq_fmt=None, iq_scale=1.0,
                                n_samples=None):
        """autocorr_search on the complex samples themselves (no abs2 before the correlation): a complex array, integer IQ
        with iq_fmt, or a device address with iq_fmt and n_samples -> (G, pos, val).  autocorr_cplx.search."""
        return autocorr_cplx.search(self, sig, Fs, minDelay, maxDelay, rate_min, rate_max, scale, iq_fmt=iq_fmt, iq_scale=iq_scale,
                                    n_samples=n_samples)

    def zoom_autocorr(self, G, Fs, rate_min=20, rate_max=100):
        pmin, pmax = C.c_size_t(0), C.c_size_t(0)
        rc = self.lib.tsdr_zoom_bounds(len(G), float(Fs), float(rate_min), float(rate_max), C.byref(pmin), C.byref(pmax))
        check(self.h, rc, "tsdr_zoom_bounds")
        idx = np.arange(pmin.value, pmax.value + 1, dtype=np.float64)
        rates = 1.0 / (idx / Fs)
        return rates, np.asarray(G)[pmin.value - 1: pmax.value]

    # -- GetSpectrum.jl -----------------------------------------------------------------
    def _sig(self, sig):
        a = np.ascontiguousarray(sig)
        if np.iscomplexobj(a):
            return a.astype(np.complex64, copy=False), 1
        return a.astype(np.float32, copy=False), 0

    def getSpectrum(self, fs, sig, N=None, lin=False, *, dtype=None, iq_fmt=None, iq_scale=1.0):
        """iq_fmt "sc16" / "sc8" / "uc8" (here and in getWelch / getWaterfall; keyword only): sig is integer IQ as the hardware
        stores it -- an int16 / int8 / uint8 array of 2*n interleaved components -- uploaded as it is and converted with iq_scale
        in the transform's loader (tsdr_spectrum_iq / tsdr_welch_iq / tsdr_waterfall_iq)."""
        if iq_fmt is not None:
            if dtype is not None:
                raise AssertionError("getSpectrum: iq_fmt is a Float32 path (dtype must be None)")
            a, code, n = _int_iq(sig, iq_fmt, "getSpectrum")
            N = n if N is None else int(N)
            if N > n:
                raise IndexError("N exceeds the signal length (BoundsError in the reference)")
            y = np.empty(N, np.float32)
            self.call("tsdr_spectrum_iq", _ptr(a), code, C.c_float(iq_scale), N, int(lin), _ptr(y))
            return (np.arange(N) / N - 0.5) * fs, y
        f64 = _is64(dtype)
        if f64:
            if not (isinstance(sig, np.ndarray) and sig.dtype in (np.float64, np.complex128)):
                raise AssertionError(f"getSpectrum: expected a float64 / complex128 array, got {getattr(sig, 'dtype', type(sig))}")
            a, cplx = np.ascontiguousarray(sig), int(np.iscomplexobj(sig))
        else:
            a, cplx = self._sig(sig)
        N = a.size if N is None else int(N)
        if N > a.size:
            raise IndexError("N exceeds the signal length (BoundsError in the reference)")
        y = np.empty(N, np.float64 if f64 else np.float32)
        self.call("tsdr_spectrum_f64" if f64 else "tsdr_spectrum", _ptr(a), cplx, N, int(lin), _ptr(y))
        freq = (np.arange(N) / N - 0.5) * fs
        return freq, y

    def _sig64(self, sig, what):
        """Float64 / ComplexF64 input of the `dtype=np.float64` spectra, as it is (no conversion)"""
        if not (isinstance(sig, np.ndarray) and sig.dtype in (np.float64, np.complex128)):
            raise AssertionError(f"{what}: expected a float64 / complex128 array, got {getattr(sig, 'dtype', type(sig))}")
        return np.ascontiguousarray(sig), int(np.iscomplexobj(sig))

    def getWelch(self, fe, sig, sizeFFT=1024, lin=False, *, dtype=None, iq_fmt=None, iq_scale=1.0):
        if iq_fmt is not None:
            if dtype is not None:
                raise AssertionError("getWelch: iq_fmt is a Float32 path (dtype must be None)")
            a, code, n = _int_iq(sig, iq_fmt, "getWelch")
            y = np.empty(int(sizeFFT), np.float32)
            self.call("tsdr_welch_iq", _ptr(a), code, C.c_float(iq_scale), n, int(sizeFFT), int(lin), _ptr(y))
            return (np.arange(sizeFFT) / sizeFFT - 0.5) * fe, y
        f64 = _is64(dtype)
        a, cplx = self._sig64(sig, "getWelch") if f64 else self._sig(sig)
        y = np.empty(int(sizeFFT), np.float64 if f64 else np.float32)
        self.call("tsdr_welch_f64" if f64 else "tsdr_welch", _ptr(a), cplx, a.size, int(sizeFFT), int(lin), _ptr(y))
        freq = (np.arange(sizeFFT) / sizeFFT - 0.5) * fe
        return freq, y

    def getWaterfall(self, fe, sig, sizeFFT=1024, *, dtype=None, iq_fmt=None, iq_scale=1.0):
        if iq_fmt is not None:
            if dtype is not None:
                raise AssertionError("getWaterfall: iq_fmt is a Float32 path (dtype must be None)")
            a, code, n = _int_iq(sig, iq_fmt, "getWaterfall")
            nb = n // int(sizeFFT)
            m = np.empty((int(sizeFFT), nb), np.float64, order="F")
            self.call("tsdr_waterfall_iq", _ptr(a), code, C.c_float(iq_scale), n, int(sizeFFT), _ptr(m))
            return np.arange(nb) * (sizeFFT / fe), (np.arange(sizeFFT) / sizeFFT - 0.5) * fe, m
        f64 = _is64(dtype)
        a, cplx = self._sig64(sig, "getWaterfall") if f64 else self._sig(sig)
        nb = a.size // int(sizeFFT)
        m = np.empty((int(sizeFFT), nb), np.float64, order="F")
        self.call("tsdr_waterfall_f64" if f64 else "tsdr_waterfall", _ptr(a), cplx, a.size, int(sizeFFT), _ptr(m))
        f_ax = (np.arange(sizeFFT) / sizeFFT - 0.5) * fe
        t_ax = np.arange(nb) * (sizeFFT / fe)
        return t_ax, f_ax, m

    def fft(self, x, inverse=False):
        a = np.ascontiguousarray(x).astype(np.complex64)
        batch = 1 if a.ndim == 1 else a.shape[0]
        n = a.shape[-1]
        out = np.empty_like(a)
        self.call("tsdr_fft_c2c", _ptr(a), _ptr(out), n, batch, 1 if inverse else -1)
        return out

    def fft64(self, x, inverse=False):
        """complex f64 FFT (tsdr_fft_z2z): the transform initLPF's ComplexF64 filter is built with"""
        a = np.ascontiguousarray(x).astype(np.complex128)
        out = np.empty_like(a)
        self.call("tsdr_fft_z2z", _ptr(a), _ptr(out), a.size, 1 if inverse else -1)
        return out

    # -- FrameSynchronisation.jl ------------------------------------------------------------
    def SyncXY(self, image, *, dtype=None):
        a = np.asarray(image)
        return SyncXY(self, a.shape[0], a.shape[1], dtype=np.float64 if _is64(dtype) else np.float32)

    def vsync(self, image, sync):
        return sync.vsync(image)

    def fill_beta(self, cv, n, w_min, w_max, *, dtype=None):
        f64 = _is64(dtype)
        x = _f64(cv, "fill_beta!") if f64 else _f32(cv)
        beta = np.empty((w_max - w_min + 1, n), np.float64 if f64 else np.float32, order="F")
        self.call("tsdr_fill_beta_f64" if f64 else "tsdr_fill_beta", _ptr(x), int(n), int(w_min), int(w_max), _ptr(beta))
        return beta

    def circshift_neg(self, image, s_y, s_x):
        a = np.asfortranarray(image, dtype=np.float32)
        out = np.empty_like(a, order="F")
        self.call("tsdr_circshift_neg", _ptr(a), a.shape[0], a.shape[1], int(s_y), int(s_x), _ptr(out))
        return out

    # -- frame loop (GUI.jl:163-178) ---------------------------------------------------------
    def frames(self, sync, iq, S, y_t, x_t, alpha, imageOut, do_align=True, want_frames=True, want_raster=False):
        """One SDR buffer through the steady-state loop.  imageOut (600x800 F-order float32) is
        updated in place.  Returns dict(n_frames, frames, raster, sync_idx)."""
        z = _c64(iq)
        nb = z.size // int(S)
        if not (isinstance(imageOut, np.ndarray) and imageOut.dtype == np.float32 and imageOut.flags.f_contiguous
                and imageOut.shape == (RENDER_H, RENDER_W)):
            raise AssertionError("imageOut must be a Fortran-order float32 (600,800) array")
        frames = np.empty((nb, RENDER_H, RENDER_W), np.float32) if want_frames else None
        raster = np.empty((nb, int(y_t) * int(x_t)), np.float32) if want_raster else None
        idx = np.zeros((nb, 2), np.int32)
        n = C.c_int(0)
        self.call("tsdr_frames", C.c_void_p(sync.h if sync is not None else 0), _ptr(z), z.size, int(S), int(y_t),
                  int(x_t), C.c_float(alpha), int(bool(do_align)), _ptr(imageOut), _ptr(frames), _ptr(raster), _ptr(idx),
                  C.byref(n))
        out = {"n_frames": n.value, "sync_idx": idx}
        if frames is not None:  # each frame is stored column-major (600,800)
            out["frames"] = [frames[f].reshape(-1).reshape((RENDER_H, RENDER_W), order="F") for f in range(nb)]
        if raster is not None:
            out["raster"] = [raster[f].reshape((int(y_t), int(x_t)), order="F") for f in range(nb)]
        return out

    # -- the same average at the monitor's own resolution (include/tempest_hip_hires.h; hires.py) -----------
    def raster_accumulate(self, rasters, state, alpha, shifts=None, units="raster", grid=(RENDER_H, RENDER_W)):
        """state (y_t x x_t, Fortran-order float32, in place) <- alpha*state + (1-alpha)*circshift(raster, -shift), raster by
        raster: GUI.jl:172,175 at raster size.  shifts: one (s_y, s_x) per raster in raster lines / pixels (units="raster") or as
        indices of a `grid` sync image (units="image", what the frame loop's sync_idx holds); None: no shift."""
        return hires.raster_accumulate(self, rasters, state, alpha, shifts, units, grid)

    def raster_accumulate_d(self, rasters, n_frames, y_t, x_t, alpha, state, shifts=None, units="raster", grid=(RENDER_H, RENDER_W)):
        """device-pointer form of raster_accumulate: enqueues on the context's stream and returns"""
        return hires.raster_accum_d(self, rasters, n_frames, y_t, x_t, alpha, state, shifts, units, grid)

    def frames_hires(self, sync, iq, S, y_t, x_t, alpha, imageOut, alpha_hires, hires_state, iq_fmt=None, iq_scale=1.0, do_align=True,
                     want_frames=True):
        """Context.frames plus hires_state (y_t x x_t, in place): the buffer's rasters, registered by the loop's own sync indices
        and averaged with alpha_hires.  Returns dict(n_frames, frames, sync_idx)."""
        return hires.frames_hires(self, sync, iq, S, y_t, x_t, alpha, imageOut, alpha_hires, hires_state, iq_fmt, iq_scale, do_align,
                                  want_frames)

    def frames_hires_d(self, sync, iq, fmt, scale, nEch, S, y_t, x_t, alpha, do_align, state, alpha_hires, hires_state, frames_out=None,
                       sync_idx=None):
        """device-pointer form of frames_hires (iq: nEch samples of format `fmt`): enqueues and returns the number of frames"""
        return hires.frames_hires_d(self, sync, iq, fmt, scale, nEch, S, y_t, x_t, alpha, do_align, state, alpha_hires, hires_state,
                                    frames_out, sync_idx)

    # -- registration of those rasters to the raster pixel (include/tempest_hip_register.h; register.py) -----------
    def raster_profiles(self, rasters):
        """-> (col (n, x_t), row (n, y_t)) float64: the sums over rows and over columns of n rasters (y_t, x_t)"""
        return register.raster_profiles(self, rasters)

    def raster_register(self, rasters, d_y, d_x, ref=None, shifts=None, units="raster", grid=(RENDER_H, RENDER_W), want_scores=False):
        """-> (n, 2) int32 shifts in raster units: the coarse `shifts` (None: 0) refined by at most d_y lines / d_x pixels against
        `ref` (None, or a flat picture: the first raster)"""
        return register.raster_register(self, rasters, d_y, d_x, ref, shifts, units, grid, want_scores)

    def raster_register_d(self, rasters, n_frames, y_t, x_t, d_y, d_x, shifts_out, ref=None, shifts=None, units="raster",
                          grid=(RENDER_H, RENDER_W), scores=None):
        """device-pointer form of raster_register: enqueues on the context's stream and returns"""
        return register.raster_register_d(self, rasters, n_frames, y_t, x_t, d_y, d_x, shifts_out, ref, shifts, units, grid, scores)

    def hires_shifts(self, max_frames=1 << 16):
        """(n, 2) int32: the raster-unit shifts the most recent frames_hires call averaged its rasters with (synchronises)"""
        return register.hires_shifts(self, max_frames)

    # -- display export of any of those pictures (include/tempest_hip_display.h; display.py) ----------------------
    def display_u8(self, images, roi=None, mode="minmax", lo=0.0, hi=1.0, p=(0.01, 0.99), invert=False, shared=False):
        """-> (bytes (n, rh, rw) uint8, ranges (n, 2) float32): the ROI (i0, j0, rh, rw; None: everything) of n pictures (h, w)
        mapped to 0 .. 255 over a "fixed" range (lo, hi), the ROI's finite "minmax", or its "percentile" fractions p"""
        return display.display_u8(self, images, roi, mode, lo, hi, p, invert, shared)

    def display_u8_d(self, images, n_images, h, w, out, roi=None, mode="minmax", lo=0.0, hi=1.0, p=(0.01, 0.99), invert=False,
                     shared=False, ranges_out=None):
        """device-pointer form of display_u8: enqueues on the context's stream and returns"""
        return display.display_u8_d(self, images, n_images, h, w, out, roi, mode, lo, hi, p, invert, shared, ranges_out)

    # -- coherent folding at a fractional frame period (include/tempest_hip_fold.h; fold.py) -------------------------
    def fold(self, iq, t0, T, n_frames, y_t, x_t, alpha=0.0, state=None, fmt="cf32", scale=1.0):
        """-> (y_t, x_t) float32: alpha * state + (1 - alpha) * the mean of n_frames frames of period T (samples, fractional)
        starting at t0, each sampled at t0 + f*T + ...; alpha == 0: no state needed"""
        return _fold.fold(self, iq, t0, T, n_frames, y_t, x_t, alpha, state, fmt, scale)

    def fold_d(self, iq, fmt, scale, n, t0, T, n_frames, y_t, x_t, alpha, state):
        """device-pointer form of fold: enqueues on the context's stream and returns"""
        return _fold.fold_d(self, iq, fmt, scale, n, t0, T, n_frames, y_t, x_t, alpha, state)

    def fold_scan(self, iq, t0, T0, dT, n_trials, n_frames, y_t, x_t, fmt="cf32", scale=1.0):
        """-> (scores float64[n_trials], best): the variance times y_t * x_t of the picture folded at T0 + k * dT, and its first maximum"""
        return _fold.fold_scan(self, iq, t0, T0, dT, n_trials, n_frames, y_t, x_t, fmt, scale)

    def fold_scan_d(self, iq, fmt, scale, n, t0, T0, dT, n_trials, n_frames, y_t, x_t, score):
        """device-pointer form of fold_scan (score: n_trials float64 on the device): enqueues and returns"""
        return _fold.fold_scan_d(self, iq, fmt, scale, n, t0, T0, dT, n_trials, n_frames, y_t, x_t, score)

    def refine_period(self, iq_d, fmt, scale, n, T_guess, n_frames, y_t, x_t, dT=0.125, half=8, levels=2, shrink=4):
        """-> (T_hat, last_dT, scores): the frame period refined from a guess good to half a sample by folding at trial periods"""
        return _fold.refine_period(self, iq_d, fmt, scale, n, T_guess, n_frames, y_t, x_t, dT, half, levels, shrink)

    # -- phase-coherent folding with carrier de-rotation (include/tempest_hip_cfold.h; cfold.py) ----------------------
    def cfold(self, iq, t0, T, kappa, n_frames, y_t, x_t, alpha=0.0, state=None, fmt="cf32", scale=1.0):
        """-> (y_t, x_t) float32: alpha * state + (1 - alpha) * |the mean of n_frames complex frames of period T starting at t0,
        frame f turned by -f * kappa turns|; alpha == 0: no state needed"""
        return _cfold.cfold(self, iq, t0, T, kappa, n_frames, y_t, x_t, alpha, state, fmt, scale)

    def cfold_d(self, iq, fmt, scale, n, t0, T, kappa, n_frames, y_t, x_t, alpha, state):
        """device-pointer form of cfold: enqueues on the context's stream and returns"""
        return _cfold.cfold_d(self, iq, fmt, scale, n, t0, T, kappa, n_frames, y_t, x_t, alpha, state)

    def cfold_scan(self, iq, t0, T, kappa0, dkappa, n_trials, n_frames, y_t, x_t, fmt="cf32", scale=1.0):
        """-> (scores float64[n_trials], best): the energy of the complex picture folded at kappa0 + k * dkappa, and its first maximum"""
        return _cfold.cfold_scan(self, iq, t0, T, kappa0, dkappa, n_trials, n_frames, y_t, x_t, fmt, scale)

    def cfold_scan_d(self, iq, fmt, scale, n, t0, T, kappa0, dkappa, n_trials, n_frames, y_t, x_t, score):
        """device-pointer form of cfold_scan (score: n_trials float64 on the device): enqueues and returns"""
        return _cfold.cfold_scan_d(self, iq, fmt, scale, n, t0, T, kappa0, dkappa, n_trials, n_frames, y_t, x_t, score)

    def refine_carrier(self, iq_d, fmt, scale, n, t0, T, n_frames, y_t, x_t, oversample=4, half=8, levels=2, shrink=4):
        """-> (kappa_hat mod 1, last_dkappa, scores): the carrier's advance per frame in turns, by a coarse-to-fine carrier scan"""
        return _cfold.refine_carrier(self, iq_d, fmt, scale, n, t0, T, n_frames, y_t, x_t, oversample, half, levels, shrink)

    # -- coherent stacking across buffers: a complex fold state, phase lock (include/tempest_hip_cstack.h; cstack.py) ----------------
    def cstack(self, iq, t0, T, kappa, phi, n_frames, y_t, x_t, alpha=0.0, mode="given", zstate=None, fmt="cf32", scale=1.0):
        """-> (zstate complex64 (y_t, x_t), mag float32 (y_t, x_t), info float64[8]): alpha * zstate + (1 - alpha) * conj(q) * Z, Z the
        complex mean of n_frames frames turned by -(phi + f * kappa) turns; q = 1 ("given") or the measured turn ("lock")"""
        return _cstack.cstack(self, iq, t0, T, kappa, phi, n_frames, y_t, x_t, alpha, mode, zstate, fmt, scale)

    def cstack_d(self, iq, fmt, scale, n, t0, T, kappa, phi, n_frames, y_t, x_t, alpha, mode, zstate, mag=None, info=None):
        """device-pointer form of cstack (mag, info: optional device pointers): enqueues on the context's stream and returns"""
        return _cstack.cstack_d(self, iq, fmt, scale, n, t0, T, kappa, phi, n_frames, y_t, x_t, alpha, mode, zstate, mag, info)

    @staticmethod
    def cstack_plan(n, t0, T, kappa, phi, theta=0.0):
        """-> (F, next_t0, next_phi): fold_plan, and the carrier phase carried over the F frames and the straddling one"""
        return _cstack.cstack_plan(n, t0, T, kappa, phi, theta)

    # -- carrier tracking: a frame phase probe, stacking along a phase track (include/tempest_hip_ctrack.h; ctrack.py) ----------------
    def ctrack_stack(self, iq, t0, T, track, n_frames, y_t, x_t, alpha=0.0, mode="given", zstate=None, fmt="cf32", scale=1.0):
        """-> (zstate, mag, info) of cstack along `track` ((F, 2) float64: frame f on line l turned by -(a_f + b_f (l + 1/2) / y_t) turns)"""
        return _ctrack.ctrack_stack(self, iq, t0, T, track, n_frames, y_t, x_t, alpha, mode, zstate, fmt, scale)

    def ctrack_stack_d(self, iq, fmt, scale, n, t0, T, track, n_frames, y_t, x_t, alpha, mode, zstate, mag=None, info=None):
        """device-pointer form of ctrack_stack (track: 2 * n_frames float64 on the device): enqueues on the context's stream and returns"""
        return _ctrack.ctrack_stack_d(self, iq, fmt, scale, n, t0, T, track, n_frames, y_t, x_t, alpha, mode, zstate, mag, info)

    def ctrack_probe(self, iq, t0, T, track, n_frames, y_t, x_t, zref, fmt="cf32", scale=1.0):
        """-> (rho complex128[F], E_f float64[F], gamma float64[F], E_s): every frame's inner product with the picture zref after the
        track's turn (track None: the zero track)"""
        return _ctrack.ctrack_probe(self, iq, t0, T, track, n_frames, y_t, x_t, zref, fmt, scale)

    def ctrack_probe_d(self, iq, fmt, scale, n, t0, T, track, n_frames, y_t, x_t, zref, out):
        """device-pointer form of ctrack_probe (out: 4 * n_frames + 1 float64 on the device): enqueues and returns"""
        return _ctrack.ctrack_probe_d(self, iq, fmt, scale, n, t0, T, track, n_frames, y_t, x_t, zref, out)

    @staticmethod
    def constant_track(n_frames, kappa, phi=0.0, slope=0.0):
        """-> the (F, 2) track a_f = f * kappa + phi, b_f = slope: cstack's weights when slope == 0"""
        return _ctrack.constant_track(n_frames, kappa, phi, slope)

    @staticmethod
    def fit_track(rho, track, degree=2):
        """-> (track, p): `track` corrected by the weighted polynomial through the probe's phases arg(rho_f) / 2 pi"""
        return _ctrack.fit_track(rho, track, degree)

    def refine_track(self, iq_d, fmt, scale, n, t0, T, n_frames, y_t, x_t, kappa, iterations=2, degree=2, zstate=None, mag=None):
        """-> (track, polynomials, gammas): a buffer's phase track from a start kappa, by stack / probe / fit iterations"""
        return _ctrack.refine_track(self, iq_d, fmt, scale, n, t0, T, n_frames, y_t, x_t, kappa, iterations, degree, zstate, mag)

    # -- the frame Gram matrix: blind carrier phases and the kappa periodogram from one pass (include/tempest_hip_gram.h; gram.py) ----
    def ctrack_gram(self, iq, t0, T, track, n_frames, y_t, x_t, fmt="cf32", scale=1.0):
        """-> G complex128 (F, F): G[f][g] = sum_m v_f(m) conj(v_g(m)), the frames of `iq` turned along `track` ((F, 2) or None)"""
        return _gram.ctrack_gram(self, iq, t0, T, track, n_frames, y_t, x_t, fmt, scale)

    def ctrack_gram_d(self, iq, fmt, scale, n, t0, T, track, n_frames, y_t, x_t, gram):
        """device-pointer form of ctrack_gram (gram: 2 * n_frames^2 float64 on the device; track may be None): enqueues and returns"""
        return _gram.ctrack_gram_d(self, iq, fmt, scale, n, t0, T, track, n_frames, y_t, x_t, gram)

    @staticmethod
    def gram_energy(G, turns):
        """-> the energy of the coherent fold for per-frame turns a_f, from G alone"""
        return _gram.gram_energy(G, turns)

    @staticmethod
    def gram_carrier(G, oversample=16, steps=4):
        """-> (kappa mod 1, energy): the maximum of the kappa periodogram of G"""
        return _gram.gram_carrier(G, oversample, steps)

    @staticmethod
    def gram_phases(G, iters=50):
        """-> (v, rho): every frame's carrier phase (unit modulus, v_0 = 1) and its inner product with the stack of all other frames"""
        return _gram.gram_phases(G, iters)

    @staticmethod
    def gram_track(G, track=None, v=None):
        """-> the track G was measured along with a_f += arg(v_f) / 2 pi (v: gram_phases(G)[0], computed when not given)"""
        return _gram.gram_track(G, track, v)

    @staticmethod
    def track_slopes(track):
        """-> the track with b_f from the differences of its a_f, and a_f moved from the frame's middle to its start"""
        return _gram.track_slopes(track)

    def blind_track(self, iq_d, fmt, scale, n, t0, T, n_frames, y_t, x_t, passes=2, zstate=None, mag=None):
        """-> (track, |rho|): a buffer's phase track with no start kappa and no reference picture, then one stack along it"""
        return _gram.blind_track(self, iq_d, fmt, scale, n, t0, T, n_frames, y_t, x_t, passes, zstate, mag)

    def coherent_period_scan(self, iq_d, fmt, scale, n, t0, y_t, x_t, periods):
        """-> (energies, kappas, best): the joint (T, kappa) search, one Gram launch per trial period"""
        return _gram.coherent_period_scan(self, iq_d, fmt, scale, n, t0, y_t, x_t, periods)

    # -- the tuner: frequency shift, FIR low-pass and decimation of an IQ stream (include/tempest_hip_tune.h; tune.py) ----
    def tune(self, iq, nu_fix, taps, decim, m0=0, phi_fix=0, j0=None, hist=None, n_hist=0, fmt="cf32", scale=1.0):
        """host arrays -> (y complex64[n_out], hist complex64[L - 1], next): `iq` shifted by nu_fix, low-passed by `taps`, decimated"""
        return _tune.tune(self, iq, nu_fix, taps, decim, m0, phi_fix, j0, hist, n_hist, fmt, scale)

    def tune_d(self, iq, fmt, scale, n, m0, nu_fix, phi_fix, taps, n_taps, decim, j0, hist, n_hist, out, out_cap):
        """device-pointer form of tune (out: room for out_cap ComplexF32; hist: n_taps - 1 ComplexF32 or None): enqueues, returns n_out"""
        return _tune.tune_d(self, iq, fmt, scale, n, m0, nu_fix, phi_fix, taps, n_taps, decim, j0, hist, n_hist, out, out_cap)

    def tuner(self, nu_fix, taps, decim, phi_fix=0, m0=0):
        """-> tune.Tuner: the device taps, the history and the plan of a stream, push_d per buffer"""
        return _tune.Tuner(self, nu_fix, taps, decim, phi_fix, m0)


def frames_d(ctx, sync, iq, nEch, S, y_t, x_t, alpha, do_align, state, frames_out=None, raster_out=None, sync_idx=None):
    """Device-pointer form of Context.frames: every array argument is a device buffer (torch tensor
    or raw address); enqueues and returns without synchronising -- on the context's stream, or (option "frames_overlap", the
    default while the context is alone on its device) with the buffer's tail on an internal stream beside the next call's image
    launch; whatever goes through the context afterwards is ordered behind it either way (tempest_hip.h: tsdr_frames_d)."""
    n = C.c_int(0)
    ctx.call("tsdr_frames_d", C.c_void_p(sync.h if sync is not None else 0), _ptr(iq), int(nEch), int(S), int(y_t),
             int(x_t), C.c_float(alpha), int(bool(do_align)), _ptr(state), _ptr(frames_out), _ptr(raster_out),
             _ptr(sync_idx), C.byref(n))
    return n.value


def frames_submit_d(ctx, sync, iq, nEch, S, y_t, x_t, alpha, do_align, state, frames_out=None, raster_out=None,
                    sync_idx=None):
    """frames_d pipelined across successive buffers on the library's internal streams: only enqueues; the tail of a
    buffer (statistics, guard, shift + IIR) runs beside the image launch of the next.  Up to three submissions in flight, each
    with its own outputs.  Outputs are complete after frames_flush(ctx) in stream order / ctx.synchronize() on the host."""
    n = C.c_int(0)
    ctx.call("tsdr_frames_submit_d", C.c_void_p(sync.h if sync is not None else 0), _ptr(iq), int(nEch), int(S), int(y_t),
             int(x_t), C.c_float(alpha), int(bool(do_align)), _ptr(state), _ptr(frames_out), _ptr(raster_out),
             _ptr(sync_idx), C.byref(n))
    return n.value


# IQ sample formats of the generic entry points (TSDR_IQ_* of tempest_hip.h): code, numpy dtype of the stored components,
# the offset subtracted before the one product by scale (uc8: 127.5, fixed)
IQ_FORMATS = {"cf32": (0, np.float32, 0.0), "sc16": (1, np.int16, 0.0), "sc8": (2, np.int8, 0.0), "uc8": (3, np.uint8, 127.5)}


def iq_fmt_code(fmt):
    """"cf32" / "sc16" / "sc8" / "uc8" (or the TSDR_IQ_* integer) -> TSDR_IQ_* code; AssertionError for anything else"""
    if isinstance(fmt, str) and fmt in IQ_FORMATS:
        return IQ_FORMATS[fmt][0]
    if isinstance(fmt, (int, np.integer)) and not isinstance(fmt, bool) and 0 <= int(fmt) <= 3:
        return int(fmt)
    raise AssertionError(f"unknown IQ format {fmt!r} (cf32, sc16, sc8, uc8)")


def expand_iq(q, fmt, scale):
    """The conversion rule of the integer IQ formats on the host: interleaved components (2*n values of the format's dtype) ->
    complex64[n], every component (f32(code) - offset) * f32(scale) with the product as the one rounding.  What every loader
    of the library forms from the raw buffer, bit for bit."""
    name = fmt if isinstance(fmt, str) else {v[0]: k for k, v in IQ_FORMATS.items()}[iq_fmt_code(fmt)]
    _, dt, off = IQ_FORMATS[name]
    a = np.ascontiguousarray(q)
    if a.dtype != dt or a.size % 2:
        raise AssertionError(f"{name} IQ is an even number of {np.dtype(dt).name} values, got {a.dtype} x {a.size}")
    if name == "cf32":
        return a.view(np.complex64)
    v = (a.astype(np.float32) - np.float32(off)) * np.float32(scale)
    return v.view(np.complex64)


def _int_iq(sig, iq_fmt, what):
    """the `iq_fmt=` keyword of the per-function API: (contiguous component array, TSDR_IQ_* code, samples); strict about the dtype"""
    code = iq_fmt_code(iq_fmt)
    if code == 0:
        raise AssertionError(f"{what}: iq_fmt is for integer IQ (sc16, sc8, uc8); ComplexF32 goes in as a complex array")
    want = {1: np.int16, 2: np.int8, 3: np.uint8}[code]
    if not isinstance(sig, np.ndarray) or sig.dtype != want or sig.size % 2:
        raise AssertionError(f"{what}: iq_fmt {iq_fmt!r} takes an {np.dtype(want).name} array of 2*n interleaved components")
    a = np.ascontiguousarray(sig)
    return a, code, a.size // 2


# Device-pointer forms of the spectra and demodulators on a buffer of `fmt` samples (the entry points of include/tempest_hip_iq.h):
# iq.py, re-exported here next to frames_iq_d.
from .iq import DEMOD_IQ, demod_iq_d, expand_iq_d, spectrum_iq_d, waterfall_iq_d, welch_iq_d  # noqa: E402
# calculate_autocorrelation of complex input (the entry points of include/tempest_hip_cplx.h): autocorr_cplx.py
from . import autocorr_cplx  # noqa: E402
# the aligned IIR on the full-size rasters and the loop that feeds it (the entry points of include/tempest_hip_hires.h): hires.py
from . import hires  # noqa: E402
# their registration to the raster pixel (the entry points of include/tempest_hip_register.h): register.py
from . import register  # noqa: E402
# the display export of any picture (the entry points of include/tempest_hip_display.h): display.py
from . import display  # noqa: E402
# coherent folding at a fractional frame period and its period scan (the entry points of include/tempest_hip_fold.h): fold.py
from . import fold as _fold  # noqa: E402  (the package exports a function of that name)
# phase-coherent folding with carrier de-rotation and its carrier scan (the entry points of include/tempest_hip_cfold.h): cfold.py
from . import cfold as _cfold  # noqa: E402  (the package exports a function of that name)
# coherent stacking across buffers (the entry points of include/tempest_hip_cstack.h): cstack.py
from . import cstack as _cstack  # noqa: E402  (the package exports a function of that name)
# carrier tracking (the entry points of include/tempest_hip_ctrack.h): ctrack.py
from . import ctrack as _ctrack  # noqa: E402
# the frame Gram matrix (the entry points of include/tempest_hip_gram.h): gram.py
from . import gram as _gram  # noqa: E402
# the tuner (the entry points of include/tempest_hip_tune.h): tune.py
from . import tune as _tune  # noqa: E402


def frames_iq_d(ctx, sync, iq, fmt, scale, nEch, S, y_t, x_t, alpha, do_align, state, frames_out=None, raster_out=None, sync_idx=None,
                submit=False):
    """frames_d / frames_submit_d on a device buffer of nEch samples of format `fmt` ("cf32", "sc16", "sc8", "uc8"): integer
    samples are converted in the kernels' loaders (tsdr_frames_iq_d / tsdr_frames_submit_iq_d); the buffer is never expanded."""
    code = iq_fmt_code(fmt)
    n = C.c_int(0)
    ctx.call("tsdr_frames_submit_iq_d" if submit else "tsdr_frames_iq_d", C.c_void_p(sync.h if sync is not None else 0), _ptr(iq),
             code, C.c_float(scale), int(nEch), int(S), int(y_t), int(x_t), C.c_float(alpha), int(bool(do_align)), _ptr(state),
             _ptr(frames_out), _ptr(raster_out), _ptr(sync_idx), C.byref(n))
    return n.value


def frames_sc16_d(ctx, sync, iq, scale, nEch, S, y_t, x_t, alpha, do_align, state, frames_out=None, raster_out=None, sync_idx=None,
                  submit=False):
    """frames_d / frames_submit_d on a device buffer of nEch interleaved int16 (re, im) pairs: every sample is
    ComplexF32(re, im) * scale, formed in the kernels' loaders (tsdr_frames_sc16_d / tsdr_frames_submit_sc16_d)."""
    n = C.c_int(0)
    ctx.call("tsdr_frames_submit_sc16_d" if submit else "tsdr_frames_sc16_d", C.c_void_p(sync.h if sync is not None else 0), _ptr(iq),
             C.c_float(scale), int(nEch), int(S), int(y_t), int(x_t), C.c_float(alpha), int(bool(do_align)), _ptr(state),
             _ptr(frames_out), _ptr(raster_out), _ptr(sync_idx), C.byref(n))
    return n.value


def frames_flush(ctx):
    """Order the context's stream after every buffer submitted with frames_submit_d."""
    ctx.call("tsdr_frames_flush")


class Group:
    """One process, several GPUs (tsdr_group_*): one context per device and one RCCL communicator per device inside the
    library; host arrays in and out.  The Python twin of TempestHIP.jl's `HipGroup` -- what a single-process runtime such as
    the reference's (GUI.jl:380-382) holds to use every MI355X of a node.  A group of one device is valid."""

    ROUTES = {"auto": 0, "sharded": 1, "root": 2}

    def __init__(self, devices=(0,)):
        self.lib = _lib.load()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p(0)
        rc = self.lib.tsdr_group_create(devs, len(devices), C.byref(h))
        if rc or not h.value:
            raise TempestHIPError(f"tsdr_group_create({list(devices)}) failed: {self.lib.tsdr_strerror(rc).decode()} "
                                  "(no usable HIP device / RCCL communicator; there is no CPU fallback)")
        self.h = h.value
        self.devices = tuple(int(d) for d in devices)

    def _chk(self, rc, what):
        if rc == _lib.TSDR_OK:
            return
        detail = self.lib.tsdr_group_last_error(self.h).decode()
        msg = f"{what}: {self.lib.tsdr_strerror(rc).decode()}" + (f" [{detail}]" if detail else "")
        if rc == _lib.TSDR_EINVAL:
            raise AssertionError(msg)
        if rc == _lib.TSDR_EBOUNDS:
            raise IndexError(msg)
        if rc == _lib.TSDR_ENOMEM:
            raise MemoryError(msg)
        raise TempestHIPError(msg)

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsdr_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.lib.tsdr_group_size(self.h)

    def set_precision(self, mode):
        self._chk(self.lib.tsdr_group_set_precision(self.h, {"exact": _lib.EXACT, "fast": _lib.FAST}[mode]), "set_precision")

    def set_option(self, name, value):
        self._chk(self.lib.tsdr_group_set_option(self.h, name.encode(), int(value)), f"set_option({name})")

    def sync_reset(self):
        self._chk(self.lib.tsdr_group_sync_reset(self.h), "sync_reset")

    def timing(self):
        """(route, [ms per-member stage incl. upload, ms collective, ms root's final stage]) of the last call"""
        r, ms = C.c_int(0), (C.c_double * 3)()
        self._chk(self.lib.tsdr_group_timing(self.h, C.byref(r), ms), "timing")
        return {1: "sharded", 2: "root"}.get(r.value, "none"), [float(v) for v in ms]

    def autocorr_search(self, sig, Fs, minDelay, maxDelay, rate_min=50, rate_max=90, scale="log", route="auto"):
        """Context.autocorr_search over the group (tsdr_group_search; GUI.jl:73-81): -> (G, pos, val)."""
        a = np.ascontiguousarray(sig)
        is_iq = int(np.iscomplexobj(a))
        a = a.astype(np.complex64 if is_iq else np.float32, copy=False)
        index_min = 1 + int(np.round(minDelay * Fs))
        index_max = int(np.round(maxDelay * Fs))
        cnt = max(index_max - index_min + 1, 0)
        pmin, pmax = C.c_size_t(0), C.c_size_t(0)
        check(None, self.lib.tsdr_zoom_bounds(cnt, float(Fs), float(rate_min), float(rate_max), C.byref(pmin), C.byref(pmax)),
              "tsdr_zoom_bounds")
        G = np.empty(max(cnt, 1), np.float32)
        n_out, idx, val = C.c_size_t(0), C.c_size_t(0), C.c_float(0)
        self._chk(self.lib.tsdr_group_search(self.h, _ptr(a), is_iq, a.size, float(Fs), float(minDelay), float(maxDelay),
                                             1 if scale == "log" else 0, _ptr(G), C.byref(n_out), int(pmin.value - 1),
                                             int(pmax.value - pmin.value + 1), C.byref(idx), C.byref(val), self.ROUTES[route]),
                  "tsdr_group_search")
        return G[: n_out.value], int(idx.value), float(val.value)

    def frames(self, iq, S, y_t, x_t, alpha, imageOut, do_align=True, want_frames=True, want_raster=False):
        """Context.frames over the group (tsdr_group_frames): frames sharded over the members, combined on the root."""
        z = _c64(iq)
        nb = z.size // int(S)
        if not (isinstance(imageOut, np.ndarray) and imageOut.dtype == np.float32 and imageOut.flags.f_contiguous
                and imageOut.shape == (RENDER_H, RENDER_W)):
            raise AssertionError("imageOut must be a Fortran-order float32 (600,800) array")
        frames = np.empty((nb, RENDER_H, RENDER_W), np.float32) if want_frames else None
        raster = np.empty((nb, int(y_t) * int(x_t)), np.float32) if want_raster else None
        idx = np.zeros((nb, 2), np.int32)
        n = C.c_int(0)
        self._chk(self.lib.tsdr_group_frames(self.h, _ptr(z), z.size, int(S), int(y_t), int(x_t), C.c_float(alpha),
                                             int(bool(do_align)), _ptr(imageOut), _ptr(frames), _ptr(raster), _ptr(idx), C.byref(n)),
                  "tsdr_group_frames")
        out = {"n_frames": n.value, "sync_idx": idx}
        if frames is not None:
            out["frames"] = [frames[f].reshape(-1).reshape((RENDER_H, RENDER_W), order="F") for f in range(nb)]
        if raster is not None:
            out["raster"] = [raster[f].reshape((int(y_t), int(x_t)), order="F") for f in range(nb)]
        return out

    def getWelch(self, fe, sig, sizeFFT=1024, lin=False):
        """Context.getWelch over the group (tsdr_group_welch): segments sharded, one all-reduce of sizeFFT floats."""
        a = np.ascontiguousarray(sig)
        cplx = int(np.iscomplexobj(a))
        a = a.astype(np.complex64 if cplx else np.float32, copy=False)
        y = np.empty(int(sizeFFT), np.float32)
        self._chk(self.lib.tsdr_group_welch(self.h, _ptr(a), cplx, a.size, int(sizeFFT), int(bool(lin)), _ptr(y)), "tsdr_group_welch")
        fAx = (np.arange(int(sizeFFT), dtype=np.float64) / int(sizeFFT) - 0.5) * fe
        return fAx, y


class StagingRing:
    """Pinned-host staging ring: the consumer side of AtomicCircularBuffer / recv!(buffer, csdr)
    (AtomicAbstractSDRs.jl:64-190, 320-322) with the buffer landing on the device.
    fmt "cf32": ComplexF32 slots; "sc16": interleaved int16 I/Q, expanded on the device to ComplexF32 * scale; "sc16raw": int16
    slots that stay int16 on the device (take_d hands out int16 pairs for frames_sc16_d with the same scale).  8-bit I/Q, two
    bytes per sample: "sc8" (int8 pairs) / "uc8" (uint8 pairs around 127.5) expanded on the device, "sc8raw" / "uc8raw" handed
    out as stored, for frames_iq_d and autocorr_search(iq_fmt=...) with the same scale.  Raw slots are also what spectrum_iq_d,
    welch_iq_d, waterfall_iq_d, demod_iq_d and expand_iq_d read (fmt = ring.iq_fmt): the displays and demodulators of the buffer
    being rastered, without an expanded copy."""
    FORMATS = {"cf32": 0, "sc16": 1, "sc16raw": 2, "sc8": 3, "sc8raw": 4, "uc8": 5, "uc8raw": 6}
    SLOT_DTYPES = {"cf32": (np.float32, np.complex64), "sc16": (np.int16,), "sc16raw": (np.int16,), "sc8": (np.int8,),
                   "sc8raw": (np.int8,), "uc8": (np.uint8,), "uc8raw": (np.uint8,)}

    def __init__(self, ctx, nEch, depth=16, fmt="cf32", scale=1.0):
        if fmt not in self.FORMATS:
            raise AssertionError(f"unknown ring format {fmt!r} ({', '.join(self.FORMATS)})")
        self.ctx, self.nEch, self.depth, self.fmt = ctx, int(nEch), int(depth), fmt
        self.scale = float(scale)
        self.sample_bytes = 8 if fmt == "cf32" else 4 if fmt in ("sc16", "sc16raw") else 2
        self.h = None
        h = C.c_void_p(0)
        ctx.call("tsdr_ring_create", self.nEch, self.depth, self.FORMATS[fmt], C.c_float(scale), C.byref(h))
        self.h = h.value

    @property
    def iq_fmt(self):
        """format of the buffers take_d hands out: "cf32" for every expanding ring, else "sc16" / "sc8" / "uc8" """
        return self.fmt[:-3] if self.fmt.endswith("raw") else "cf32"

    def _chk(self, rc, what):
        check(self.ctx.h, rc, what)

    def put(self, buf):
        """circ_put!: copy one buffer (complex64[nEch], or int16 / int8 / uint8 [2*nEch] for the integer formats) into the
        ring; never waits for the consumer."""
        a = np.ascontiguousarray(buf)
        want = self.nEch * self.sample_bytes
        if a.nbytes != want:
            raise AssertionError(f"ring slot is {want} bytes, got {a.nbytes}")
        if self.sample_bytes == 2 and a.dtype not in self.SLOT_DTYPES[self.fmt]:   # (int8 and uint8 differ in meaning only)
            raise AssertionError(f"a {self.fmt} ring takes {np.dtype(self.SLOT_DTYPES[self.fmt][0]).name} components, got {a.dtype}")
        self._chk(self.ctx.lib.tsdr_ring_put(self.h, _ptr(a)), "tsdr_ring_put")

    def write_view(self):
        """Zero-copy producer: a numpy view of the pinned slot to fill; publish it with commit()."""
        p = self.ctx.lib.tsdr_ring_write_ptr(self.h)
        n = self.nEch * 2
        ctype = {8: C.c_float, 4: C.c_int16}.get(self.sample_bytes, C.c_uint8 if self.fmt.startswith("uc8") else C.c_int8)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(n,))

    def commit(self):
        self._chk(self.ctx.lib.tsdr_ring_commit(self.h), "tsdr_ring_commit")

    def take_d(self, timeout_ms=-1):
        """circ_take! / recv!: device address of the next buffer (nEch ComplexF32); IndexError on timeout/stop."""
        p = C.c_void_p(0)
        self._chk(self.ctx.lib.tsdr_ring_take_d(self.h, int(timeout_ms), C.byref(p)), "tsdr_ring_take_d")
        return p.value

    def stop(self):
        self._chk(self.ctx.lib.tsdr_ring_stop(self.h), "tsdr_ring_stop")

    def stats(self):
        a, b, c = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        rp, rc_ = C.c_double(0), C.c_double(0)
        self._chk(self.ctx.lib.tsdr_ring_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(rp), C.byref(rc_)),
                  "tsdr_ring_stats")
        h, m = C.c_ulonglong(0), C.c_ulonglong(0)
        self._chk(self.ctx.lib.tsdr_ring_prefetch_stats(self.h, C.byref(h), C.byref(m)), "tsdr_ring_prefetch_stats")
        return {"produced": a.value, "consumed": b.value, "overflow": c.value, "producer_msps": rp.value,
                "consumer_msps": rc_.value, "prefetch_hits": h.value, "prefetch_misses": m.value}

    def close(self):
        if self.h:
            self.ctx.lib.tsdr_ring_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SyncXY:
    """SyncXY{Float32} state (FrameSynchronisation.jl:25-48) living on the device; dtype=np.float64: SyncXY{Float64}
    (tsdr_sync_create_f64), whose vsync takes Float64 images and whose beta fields are Float64."""

    def __init__(self, ctx, y_t, x_t, dtype=np.float32):
        self.ctx = ctx
        self.y_t, self.x_t = int(y_t), int(x_t)
        if np.dtype(dtype) not in (np.float32, np.float64):
            raise AssertionError(f"SyncXY{{{dtype}}}: only Float32 and Float64 states exist (MethodError in the reference)")
        self.dtype = np.dtype(dtype)
        self.f64 = self.dtype == np.float64
        h = C.c_void_p(0)
        ctx.call("tsdr_sync_create_f64" if self.f64 else "tsdr_sync_create", self.y_t, self.x_t, C.byref(h))
        self.h = h.value
        b = (C.c_int * 4)()
        check(ctx.h, ctx.lib.tsdr_sync_bounds(self.h, b), "tsdr_sync_bounds")
        self.wmin_y, self.wmax_y, self.wmin_x, self.wmax_x = list(b)

    def reset(self):
        check(self.ctx.h, self.ctx.lib.tsdr_sync_reset(self.h), "tsdr_sync_reset")

    def vsync(self, image):
        if self.f64:
            a = np.asfortranarray(_need(image, np.float64, "vsync(::Matrix, ::SyncXY{Float64})"))
        else:
            a = np.asfortranarray(image, dtype=np.float32)
        if a.shape != (self.y_t, self.x_t):
            raise AssertionError("image size does not match the SyncXY state")
        sy, sx = C.c_int(0), C.c_int(0)
        fn = "tsdr_vsync_f64" if self.f64 else "tsdr_vsync"
        check(self.ctx.h, getattr(self.ctx.lib, fn)(self.h, _ptr(a), C.byref(sy), C.byref(sx)), fn)
        return sy.value, sx.value

    def beta(self, which):
        """which='x' -> beta_x (W_x, x_t); 'y' -> beta_y (W_y, y_t); Fortran order like the Julia field."""
        if which == "x":
            shape, w = (1 + self.wmax_x - self.wmin_x, self.x_t), 0
        else:
            shape, w = (1 + self.wmax_y - self.wmin_y, self.y_t), 1
        out = np.empty(shape, self.dtype, order="F")
        fn = "tsdr_sync_beta_f64" if self.f64 else "tsdr_sync_beta"
        check(self.ctx.h, getattr(self.ctx.lib, fn)(self.h, w, _ptr(out)), fn)
        return out

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.tsdr_sync_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Resampler:
    """The closure init_resampler returns (Resampler.jl:26-62): call it as r(out, inp).  dtype=np.float64: the Float64 closure
    (tsdr_resampler_init_f64), whose buffers are float64."""

    def __init__(self, ctx, bufferSize, upCoeff, dtype=np.float32):
        self.ctx, self.bufferSize, self.upCoeff = ctx, bufferSize, upCoeff
        self.dtype = np.dtype(dtype)
        self.f64 = self.dtype == np.float64
        h = C.c_void_p(0)
        ctx.call("tsdr_resampler_init_f64" if self.f64 else "tsdr_resampler_init", bufferSize, upCoeff, C.byref(h))
        self.h = h.value

    def __call__(self, out, inp):
        if not (isinstance(out, np.ndarray) and isinstance(inp, np.ndarray)):
            raise AssertionError("numpy arrays expected")
        if self.f64:
            if out.dtype != np.float64 or inp.dtype != np.float64:  # Resampler.jl:44
                raise AssertionError(f"Type of input ({inp.dtype}) should match type used during init (Float64)")
        elif out.dtype != np.float32 or inp.dtype != np.float32:
            raise AssertionError("Type of input should match type used during init (Float32)")  # Resampler.jl:44
        if inp.size != self.bufferSize:
            raise AssertionError(f"Size of input {inp.size} should match size used during init {self.bufferSize}")  # :47
        if out.size < self.bufferSize * self.upCoeff:
            raise IndexError("out too short")
        if not out.flags.c_contiguous:
            raise AssertionError("out must be contiguous")
        x = np.ascontiguousarray(inp)
        fn = "tsdr_resampler_run_f64" if self.f64 else "tsdr_resampler_run"
        check(self.ctx.h, getattr(self.ctx.lib, fn)(self.h, _ptr(x), x.size, _ptr(out)), fn)

    def lpf(self):
        H = np.empty(self.bufferSize * self.upCoeff, np.complex64)
        check(self.ctx.h, self.ctx.lib.tsdr_resampler_lpf(self.h, _ptr(H)), "tsdr_resampler_lpf")
        return H

    def lpf64(self):
        """H as the closure applies it: ComplexF64 (Resampler.jl:93-97)"""
        H = np.empty(self.bufferSize * self.upCoeff, np.complex128)
        check(self.ctx.h, self.ctx.lib.tsdr_resampler_lpf64(self.h, _ptr(H)), "tsdr_resampler_lpf64")
        return H

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.tsdr_resampler_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default = None


def default_context():
    global _default
    if _default is None:
        _default = Context(0)
    return _default


# module-level functions with the reference's names, bound to the default context
def amDemod(sig, *, dtype=None): return default_context().amDemod(sig, dtype=dtype)
def invert_amDemod(sig, *, dtype=None): return default_context().invert_amDemod(sig, dtype=dtype)
def fmDemod(sig, *, dtype=None): return default_context().fmDemod(sig, dtype=dtype)
def abs2(sig, *, dtype=None): return default_context().abs2(sig, dtype=dtype)
def imresize1d(sig, n_out, *, dtype=None): return default_context().imresize1d(sig, n_out, dtype=dtype)
def imresize2d(image, size, *, dtype=None): return default_context().imresize2d(image, size, dtype=dtype)
def sig_to_image(sig, y_t, x_t, *, dtype=None): return default_context().sig_to_image(sig, y_t, x_t, dtype=dtype)
def downgradeImage(image, *, dtype=None): return default_context().downgradeImage(image, dtype=dtype)
def naiveResampler(sigOut, sigId, upCoeff, *, dtype=None): return default_context().naiveResampler(sigOut, sigId, upCoeff, dtype=dtype)
def init_resampler(T, bufferSize, upCoeff): return default_context().init_resampler(T, bufferSize, upCoeff)
def calculate_autocorrelation(x, Fs, minDelay, maxDelay, scale="log", *, dtype=None, iq_fmt=None, iq_scale=1.0):
    return default_context().calculate_autocorrelation(x, Fs, minDelay, maxDelay, scale, dtype=dtype, iq_fmt=iq_fmt, iq_scale=iq_scale)
def zoom_autocorr(G, Fs, rate_min=20, rate_max=100): return default_context().zoom_autocorr(G, Fs, rate_min, rate_max)
def getSpectrum(fs, sig, N=None, *, dtype=None): return default_context().getSpectrum(fs, sig, N, dtype=dtype)
def getWelch(fe, sig, sizeFFT=1024, *, dtype=None): return default_context().getWelch(fe, sig, sizeFFT, dtype=dtype)
def getWaterfall(fe, sig, sizeFFT=1024, *, dtype=None): return default_context().getWaterfall(fe, sig, sizeFFT, dtype=dtype)
def vsync(image, sync): return sync.vsync(image)
