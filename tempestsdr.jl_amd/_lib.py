"""ctypes binding of libtempest_hip.so (the C ABI declared in include/tempest_hip.h).

This is the Python twin of julia/TempestHIP.jl: same entry points, same status-code ->
exception mapping.  There is no fallback of any kind: if the shared library is missing or
no HIP device can be opened, loading/creating raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# TSDR_HIP_LIB: load another build of the same library (A/B timing of kernel variants on one GPU box)
LIB_PATH = os.environ.get("TSDR_HIP_LIB") or os.path.join(HERE, "libtempest_hip.so")

TSDR_OK, TSDR_EINVAL, TSDR_EBOUNDS, TSDR_ENOMEM, TSDR_EHIP, TSDR_ENODEV = 0, -1, -2, -3, -4, -5
RENDER_H, RENDER_W = 600, 800
EXACT, FAST = 0, 1  # tsdr_precision


class TempestHIPError(RuntimeError):
    pass


_lib = None

c_f = C.POINTER(C.c_float)
c_d = C.POINTER(C.c_double)
c_i = C.POINTER(C.c_int)
c_sz = C.c_size_t
c_szp = C.POINTER(C.c_size_t)
vp = C.c_void_p

# name -> (restype, argtypes).  Pointers that may be host OR device are declared c_void_p.
_SIGS = {
    "tsdr_create": (vp, [C.c_int]),
    "tsdr_destroy": (None, [vp]),
    "tsdr_strerror": (C.c_char_p, [C.c_int]),
    "tsdr_last_error": (C.c_char_p, [vp]),
    "tsdr_version": (C.c_char_p, []),
    "tsdr_set_stream": (C.c_int, [vp, vp]),
    "tsdr_synchronize": (C.c_int, [vp]),
    "tsdr_set_precision": (C.c_int, [vp, C.c_int]),
    "tsdr_get_precision": (C.c_int, [vp]),
    "tsdr_set_option": (C.c_int, [vp, C.c_char_p, C.c_int]),
    "tsdr_sync_guard_stats": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.c_int]),
    "tsdr_sync_guard_auto": (C.c_int, [vp, c_i, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "tsdr_wait_stats": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "tsdr_debug_hold_stream": (C.c_int, [vp, C.c_int]),
    "tsdr_frames_overlap_stats": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint), C.c_int]),
    "tsdr_debug_hold_tail": (C.c_int, [vp, C.c_int]),
    "tsdr_sync_guard_margins": (C.c_int, [vp, C.c_int, vp, c_i]),
    "tsdr_device_info": (C.c_int, [vp, C.c_char_p, c_sz, c_i, c_szp]),
    "tsdr_dev_alloc": (vp, [vp, c_sz]),
    "tsdr_dev_free": (C.c_int, [vp, vp]),
    "tsdr_upload": (C.c_int, [vp, vp, vp, c_sz]),
    "tsdr_download": (C.c_int, [vp, vp, vp, c_sz]),
    "tsdr_timer_start": (C.c_int, [vp]),
    "tsdr_timer_stop": (C.c_int, [vp, c_d]),
    "tsdr_profile_enable": (C.c_int, [vp, C.c_int]),
    "tsdr_profile_reset": (C.c_int, [vp]),
    "tsdr_profile_count": (C.c_int, [vp]),
    "tsdr_profile_get": (C.c_int, [vp, C.c_int, C.c_char_p, c_sz, c_d, C.POINTER(C.c_longlong)]),
    # Demodulation.jl
    "tsdr_am_demod": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_am_demod_d": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_invert_am": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_invert_am_d": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_fm_demod": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_fm_demod_d": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_abs2": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_abs2_d": (C.c_int, [vp, vp, c_sz, vp]),
    # Resampler.jl
    "tsdr_resize1d": (C.c_int, [vp, vp, c_sz, c_sz, vp]),
    "tsdr_resize1d_d": (C.c_int, [vp, vp, c_sz, c_sz, vp]),
    "tsdr_sig_to_image": (C.c_int, [vp, vp, c_sz, C.c_int, C.c_int, vp]),
    "tsdr_sig_to_image_d": (C.c_int, [vp, vp, c_sz, C.c_int, C.c_int, vp]),
    "tsdr_resize2d": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "tsdr_resize2d_d": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "tsdr_downgrade": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    "tsdr_downgrade_d": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    "tsdr_naive_resample": (C.c_int, [vp, vp, c_sz, C.c_int, vp]),
    "tsdr_naive_resample_d": (C.c_int, [vp, vp, c_sz, C.c_int, vp]),
    "tsdr_resampler_init": (C.c_int, [vp, c_sz, C.c_int, C.POINTER(vp)]),
    "tsdr_resampler_run": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_resampler_run_d": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_resampler_lpf": (C.c_int, [vp, vp]),
    "tsdr_resampler_lpf64": (C.c_int, [vp, vp]),
    "tsdr_fft_z2z": (C.c_int, [vp, vp, vp, c_sz, C.c_int]),
    "tsdr_resampler_free": (None, [vp]),
    # Autocorrelations.jl
    "tsdr_autocorr": (C.c_int, [vp, vp, c_sz, C.c_double, C.c_double, C.c_double, C.c_int, vp, c_szp]),
    "tsdr_autocorr_d": (C.c_int, [vp, vp, c_sz, C.c_double, C.c_double, C.c_double, C.c_int, vp, c_szp]),
    "tsdr_autocorr_iq_d": (C.c_int, [vp, vp, c_sz, C.c_double, C.c_double, C.c_double, C.c_int, vp, c_szp]),
    "tsdr_autocorr_search_d": (C.c_int, [vp, vp, C.c_int, c_sz, C.c_double, C.c_double, C.c_double, C.c_int, vp, c_szp, c_sz, c_sz,
                                         c_szp, c_f]),
    "tsdr_autocorr_search_iq_d": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, C.c_double, C.c_double, C.c_double, C.c_int, vp, c_szp,
                                            c_sz, c_sz, c_szp, c_f]),
    "tsdr_autocorr_partial_d": (C.c_int, [vp, vp, C.c_int, c_sz, c_sz, c_sz, c_sz, vp]),
    "tsdr_autocorr_finish_d": (C.c_int, [vp, vp, c_sz, c_sz, C.c_int, vp]),
    "tsdr_zoom_bounds": (C.c_int, [c_sz, C.c_double, C.c_double, C.c_double, c_szp, c_szp]),
    "tsdr_argmax_d": (C.c_int, [vp, vp, c_sz, c_szp, c_f]),
    # GetSpectrum.jl
    "tsdr_spectrum": (C.c_int, [vp, vp, C.c_int, c_sz, C.c_int, vp]),
    "tsdr_spectrum_d": (C.c_int, [vp, vp, C.c_int, c_sz, C.c_int, vp]),
    "tsdr_welch": (C.c_int, [vp, vp, C.c_int, c_sz, c_sz, C.c_int, vp]),
    "tsdr_welch_d": (C.c_int, [vp, vp, C.c_int, c_sz, c_sz, C.c_int, vp]),
    "tsdr_waterfall": (C.c_int, [vp, vp, C.c_int, c_sz, c_sz, vp]),
    "tsdr_waterfall_d": (C.c_int, [vp, vp, C.c_int, c_sz, c_sz, vp]),
    "tsdr_fft_c2c": (C.c_int, [vp, vp, vp, c_sz, c_sz, C.c_int]),
    "tsdr_fft_c2c_d": (C.c_int, [vp, vp, vp, c_sz, c_sz, C.c_int]),
    # ... and Demodulation.jl's functions on integer IQ (iq, iq_fmt, scale as tsdr_frames_iq_d)
    "tsdr_spectrum_iq": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, C.c_int, vp]),
    "tsdr_welch_iq": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, c_sz, C.c_int, vp]),
    "tsdr_waterfall_iq": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, c_sz, vp]),
    "tsdr_fft_plan": (C.c_int, [c_sz, vp, C.c_int]),
    # FrameSynchronisation.jl
    "tsdr_sync_create": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(vp)]),
    "tsdr_sync_reset": (C.c_int, [vp]),
    "tsdr_sync_free": (None, [vp]),
    "tsdr_sync_bounds": (C.c_int, [vp, c_i]),
    "tsdr_vsync": (C.c_int, [vp, vp, c_i, c_i]),
    "tsdr_vsync_d": (C.c_int, [vp, vp, vp]),
    "tsdr_sync_beta": (C.c_int, [vp, C.c_int, vp]),
    "tsdr_fill_beta": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "tsdr_circshift_neg": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    # Float64 / ComplexF64 element types of the per-function API
    "tsdr_am_demod_f64": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_am_demod_f64_d": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_invert_am_f64": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_invert_am_f64_d": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_fm_demod_f64": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_fm_demod_f64_d": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_abs2_f64": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_abs2_f64_d": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_resize1d_f64": (C.c_int, [vp, vp, c_sz, c_sz, vp]),
    "tsdr_resize1d_f64_d": (C.c_int, [vp, vp, c_sz, c_sz, vp]),
    "tsdr_sig_to_image_f64": (C.c_int, [vp, vp, c_sz, C.c_int, C.c_int, vp]),
    "tsdr_sig_to_image_f64_d": (C.c_int, [vp, vp, c_sz, C.c_int, C.c_int, vp]),
    "tsdr_resize2d_f64": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "tsdr_resize2d_f64_d": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "tsdr_downgrade_f64": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    "tsdr_downgrade_f64_d": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    "tsdr_naive_resample_f64": (C.c_int, [vp, vp, c_sz, C.c_int, vp]),
    "tsdr_naive_resample_f64_d": (C.c_int, [vp, vp, c_sz, C.c_int, vp]),
    "tsdr_sync_create_f64": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(vp)]),
    "tsdr_vsync_f64": (C.c_int, [vp, vp, c_i, c_i]),
    "tsdr_vsync_f64_d": (C.c_int, [vp, vp, vp]),
    "tsdr_sync_beta_f64": (C.c_int, [vp, C.c_int, vp]),
    "tsdr_fill_beta_f64": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "tsdr_autocorr_f64": (C.c_int, [vp, vp, c_sz, C.c_double, C.c_double, C.c_double, C.c_int, vp, c_szp]),
    "tsdr_autocorr_f64_d": (C.c_int, [vp, vp, c_sz, C.c_double, C.c_double, C.c_double, C.c_int, vp, c_szp]),
    "tsdr_spectrum_f64": (C.c_int, [vp, vp, C.c_int, c_sz, C.c_int, vp]),
    "tsdr_spectrum_f64_d": (C.c_int, [vp, vp, C.c_int, c_sz, C.c_int, vp]),
    "tsdr_welch_f64": (C.c_int, [vp, vp, C.c_int, c_sz, c_sz, C.c_int, vp]),
    "tsdr_welch_f64_d": (C.c_int, [vp, vp, C.c_int, c_sz, c_sz, C.c_int, vp]),
    "tsdr_waterfall_f64": (C.c_int, [vp, vp, C.c_int, c_sz, c_sz, vp]),
    "tsdr_waterfall_f64_d": (C.c_int, [vp, vp, C.c_int, c_sz, c_sz, vp]),
    "tsdr_resampler_init_f64": (C.c_int, [vp, c_sz, C.c_int, C.POINTER(vp)]),
    "tsdr_resampler_run_f64": (C.c_int, [vp, vp, c_sz, vp]),
    "tsdr_resampler_run_f64_d": (C.c_int, [vp, vp, c_sz, vp]),
    # frame loop
    "tsdr_frames": (C.c_int, [vp, vp, vp, c_sz, c_sz, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, c_i]),
    "tsdr_frames_d": (C.c_int, [vp, vp, vp, c_sz, c_sz, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, c_i]),
    "tsdr_frames_submit_d": (C.c_int, [vp, vp, vp, c_sz, c_sz, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, c_i]),
    "tsdr_frames_flush": (C.c_int, [vp]),
    "tsdr_frames_sc16_d": (C.c_int, [vp, vp, vp, C.c_float, c_sz, c_sz, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, c_i]),
    "tsdr_frames_submit_sc16_d": (C.c_int, [vp, vp, vp, C.c_float, c_sz, c_sz, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, c_i]),
    "tsdr_frames_iq_d": (C.c_int, [vp, vp, vp, C.c_int, C.c_float, c_sz, c_sz, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, c_i]),
    "tsdr_frames_submit_iq_d": (C.c_int, [vp, vp, vp, C.c_int, C.c_float, c_sz, c_sz, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, c_i]),
    "tsdr_frames_pipeline_info": (C.c_int, [vp, c_i, c_i, c_f, C.c_int, C.c_char_p, c_sz]),
    "tsdr_ring_create": (C.c_int, [vp, c_sz, C.c_int, C.c_int, C.c_float, C.POINTER(vp)]),
    "tsdr_ring_free": (None, [vp]),
    "tsdr_ring_put": (C.c_int, [vp, vp]),
    "tsdr_ring_write_ptr": (vp, [vp]),
    "tsdr_ring_commit": (C.c_int, [vp]),
    "tsdr_ring_take_d": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
    "tsdr_ring_stop": (C.c_int, [vp]),
    "tsdr_ring_stats": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "tsdr_ring_prefetch_stats": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "tsdr_frames_scan_d": (C.c_int, [vp, vp, vp, c_sz, c_sz, C.c_int, C.c_int, C.c_int, vp, vp, vp, c_i]),
    "tsdr_frames_combine_d": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp, vp, vp]),
    # one process, several GPUs (RCCL inside the library)
    "tsdr_group_create": (C.c_int, [c_i, C.c_int, C.POINTER(vp)]),
    "tsdr_group_destroy": (None, [vp]),
    "tsdr_group_size": (C.c_int, [vp]),
    "tsdr_group_ctx": (vp, [vp, C.c_int]),
    "tsdr_group_last_error": (C.c_char_p, [vp]),
    "tsdr_group_set_precision": (C.c_int, [vp, C.c_int]),
    "tsdr_group_set_option": (C.c_int, [vp, C.c_char_p, C.c_int]),
    "tsdr_group_search": (C.c_int, [vp, vp, C.c_int, c_sz, C.c_double, C.c_double, C.c_double, C.c_int, vp, c_szp, c_sz, c_sz,
                                    c_szp, c_f, C.c_int]),
    "tsdr_group_frames": (C.c_int, [vp, vp, c_sz, c_sz, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, c_i]),
    "tsdr_group_sync_reset": (C.c_int, [vp]),
    "tsdr_group_welch": (C.c_int, [vp, vp, C.c_int, c_sz, c_sz, C.c_int, vp]),
    "tsdr_group_timing": (C.c_int, [vp, c_i, c_d]),
}

# include/tempest_hip_iq.h (the header tempest_hip.h includes): the device-pointer forms of the spectra and demodulators on integer
# IQ, and the ring's expansion (iq, iq_fmt, scale as tsdr_frames_iq_d)
_SIGS_IQ = {
    "tsdr_spectrum_iq_d": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, C.c_int, vp]),
    "tsdr_welch_iq_d": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, c_sz, C.c_int, vp]),
    "tsdr_waterfall_iq_d": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, c_sz, vp]),
    "tsdr_am_demod_iq_d": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, vp]),
    "tsdr_abs2_iq_d": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, vp]),
    "tsdr_invert_am_iq_d": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, vp]),
    "tsdr_fm_demod_iq_d": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, vp]),
    "tsdr_iq_expand_d": (C.c_int, [vp, vp, C.c_int, C.c_float, c_sz, vp]),
}

# include/tempest_hip_cplx.h (the other header tempest_hip.h includes): calculate_autocorrelation of complex input -- ComplexF32,
# integer IQ as stored, ComplexF64 -- and its search twin
_AC = [c_sz, C.c_double, C.c_double, C.c_double, C.c_int, vp, c_szp]   # len, Fs, minDelay, maxDelay, log_scale, out, n_out
_SIGS_CPLX = {
    "tsdr_autocorr_cplx": (C.c_int, [vp, vp] + _AC),
    "tsdr_autocorr_cplx_d": (C.c_int, [vp, vp] + _AC),
    "tsdr_autocorr_cplx_iq": (C.c_int, [vp, vp, C.c_int, C.c_float] + _AC),
    "tsdr_autocorr_cplx_search_iq_d": (C.c_int, [vp, vp, C.c_int, C.c_float] + _AC + [c_sz, c_sz, c_szp, c_f]),
    "tsdr_autocorr_cplx_f64": (C.c_int, [vp, vp] + _AC),
    "tsdr_autocorr_cplx_f64_d": (C.c_int, [vp, vp] + _AC),
}

# include/tempest_hip_hires.h (the third header tempest_hip.h includes): the aligned IIR on the y_t x x_t rasters and the frame loop
# that feeds it
_ACC = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp]   # rasters, n, y_t, x_t, shifts, units, img_h, img_w, alpha, state
_SIGS_HIRES = {
    "tsdr_raster_accum": (C.c_int, [vp] + _ACC),
    "tsdr_raster_accum_d": (C.c_int, [vp] + _ACC),
    "tsdr_frames_hires_iq_d": (C.c_int, [vp, vp, vp, C.c_int, C.c_float, c_sz, c_sz, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, C.c_float,
                                         vp, vp, c_i]),
}
SHIFT_RASTER, SHIFT_IMAGE = 0, 1  # TSDR_SHIFT_*

# include/tempest_hip_register.h (included after tempest_hip_hires.h): registration of the full-size rasters to the raster pixel
_REG = [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]  # rasters, n, y_t, x_t, ref, shifts, units, img_h, img_w, d_y, d_x, shifts_out, scores
_SIGS_REGISTER = {
    "tsdr_raster_profiles_d": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "tsdr_raster_register_d": (C.c_int, [vp] + _REG),
    "tsdr_raster_register": (C.c_int, [vp] + _REG),
    "tsdr_frames_hires_shifts": (C.c_int, [vp, C.c_int, c_i, c_i]),
}

# include/tempest_hip_display.h (included after tempest_hip_register.h): ROI crop, range stretch and 8-bit output of f32 pictures
_DISP = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_double, C.c_double,
         C.c_int, vp, vp]  # images, n, h, w, i0, j0, rh, rw, range_mode, lo, hi, p_lo, p_hi, flags, out, ranges_out
_SIGS_DISPLAY = {
    "tsdr_display_u8_d": (C.c_int, [vp] + _DISP),
    "tsdr_display_u8": (C.c_int, [vp] + _DISP),
}
RANGE_FIXED, RANGE_MINMAX, RANGE_PERCENTILE = 0, 1, 2  # TSDR_RANGE_*
DISPLAY_INVERT, DISPLAY_SHARED = 1, 2  # TSDR_DISPLAY_* flags
DISPLAY_BINS = 4096

# include/tempest_hip_fold.h (included after tempest_hip_display.h): coherent frame folding at a fractional period, and its period scan
_FOLD = [vp, vp, C.c_int, C.c_float, c_sz, C.c_double]  # ctx, iq, iq_fmt, scale, n, t0
_GEOM = [C.c_int, C.c_int, C.c_int]  # n_frames, y_t, x_t
_SIGS_FOLD = {
    "tsdr_fold_iq_d": (C.c_int, _FOLD + [C.c_double] + _GEOM + [C.c_float, vp]),                    # T, ..., alpha, state
    "tsdr_fold_iq": (C.c_int, _FOLD + [C.c_double] + _GEOM + [C.c_float, vp]),
    "tsdr_fold_scan_iq_d": (C.c_int, _FOLD + [C.c_double, C.c_double, C.c_int] + _GEOM + [vp]),     # T0, dT, n_trials, ..., score
    "tsdr_fold_scan_iq": (C.c_int, _FOLD + [C.c_double, C.c_double, C.c_int] + _GEOM + [vp, vp]),   # ..., score, best
}
FOLD_MAX_TRIALS, FOLD_STAGE_MAX = 4096, 240  # TSDR_FOLD_*

# include/tempest_hip_cfold.h (included after tempest_hip_fold.h): phase-coherent folding with carrier de-rotation, and its carrier scan
_SIGS_CFOLD = {
    "tsdr_cfold_iq_d": (C.c_int, _FOLD + [C.c_double, C.c_double] + _GEOM + [C.c_float, vp]),                    # T, kappa, ..., alpha, state
    "tsdr_cfold_iq": (C.c_int, _FOLD + [C.c_double, C.c_double] + _GEOM + [C.c_float, vp]),
    "tsdr_cfold_scan_iq_d": (C.c_int, _FOLD + [C.c_double, C.c_double, C.c_double, C.c_int] + _GEOM + [vp]),     # T, kappa0, dkappa, n_trials, ..., score
    "tsdr_cfold_scan_iq": (C.c_int, _FOLD + [C.c_double, C.c_double, C.c_double, C.c_int] + _GEOM + [vp, vp]),   # ..., score, best
}
CFOLD_MAX_TRIALS, CFOLD_STAGE_MAX = 4096, 120  # TSDR_CFOLD_*

# include/tempest_hip_cstack.h (included after tempest_hip_cfold.h): coherent stacking across buffers -- a complex fold state, phase lock
_CSTACK = _FOLD + [C.c_double, C.c_double, C.c_double] + _GEOM + [C.c_float, C.c_int, vp, vp, vp]  # T, kappa, phi, ..., alpha, mode, zstate, mag, info
_SIGS_CSTACK = {
    "tsdr_cstack_iq_d": (C.c_int, list(_CSTACK)),
    "tsdr_cstack_iq": (C.c_int, list(_CSTACK)),
}
CSTACK_GIVEN, CSTACK_LOCK, CSTACK_INFO = 0, 1, 8  # TSDR_CSTACK_*

# include/tempest_hip_ctrack.h (included after tempest_hip_cstack.h): carrier tracking -- a frame phase probe, stacking along a phase track
_CTRACK_STACK = _FOLD + [C.c_double, vp] + _GEOM + [C.c_float, C.c_int, vp, vp, vp]  # T, track, ..., alpha, mode, zstate, mag, info
_CTRACK_PROBE = _FOLD + [C.c_double, vp] + _GEOM + [vp, vp]                           # T, track, ..., zref, out
_SIGS_CTRACK = {
    "tsdr_ctrack_stack_iq_d": (C.c_int, list(_CTRACK_STACK)),
    "tsdr_ctrack_stack_iq": (C.c_int, list(_CTRACK_STACK)),
    "tsdr_ctrack_probe_iq_d": (C.c_int, list(_CTRACK_PROBE)),
    "tsdr_ctrack_probe_iq": (C.c_int, list(_CTRACK_PROBE)),
}

# include/tempest_hip_gram.h (included after tempest_hip_ctrack.h): the frame Gram matrix along a track.  gram.py names the two symbols
# through GRAM_IQ_D / GRAM_IQ: every other module of the package stays free of the tsdr_ctrack prefix, which belongs to ctrack.py
_CTRACK_GRAM = _FOLD + [C.c_double, vp] + _GEOM + [vp]                                # T, track, ..., gram
GRAM_IQ_D, GRAM_IQ = "tsdr_ctrack_gram_iq_d", "tsdr_ctrack_gram_iq"
_SIGS_GRAM = {
    GRAM_IQ_D: (C.c_int, list(_CTRACK_GRAM)),
    GRAM_IQ: (C.c_int, list(_CTRACK_GRAM)),
}
GRAM_MAX_FRAMES, GRAM_CHUNK, GRAM_MAX_TILES = 64, 1024, 65536  # TSDR_GRAM_*

# include/tempest_hip_tune.h (included after tempest_hip_gram.h): the tuner -- frequency shift, FIR low-pass, decimation (tune.py)
c_u64 = C.c_uint64
_TUNE = [vp, vp, C.c_int, C.c_float, c_sz, c_u64, c_u64, c_u64, vp, C.c_int, C.c_int, c_u64, vp, C.c_int, vp, c_sz, vp]
#        ctx, iq, iq_fmt, scale, n, m0, nu_fix, phi_fix, taps, n_taps, decim, j0, hist, n_hist, out, out_cap, n_out
_SIGS_TUNE = {
    "tsdr_tune_iq_d": (C.c_int, list(_TUNE)),
    "tsdr_tune_iq": (C.c_int, list(_TUNE)),
    "tsdr_tune_tile": (C.c_int, [C.c_int, C.c_int]),   # n_taps, decim (no context)
}
TUNE_TAPS_MAX, TUNE_DECIM_MAX = 1024, 64  # TSDR_TUNE_*


def exported_names():
    """Every symbol include/tempest_hip.h declares (kept in sync by tests/test_abi.py)."""
    return sorted(_SIGS)


def exported_names_iq():
    """Every symbol include/tempest_hip_iq.h declares (kept in sync by tests/test_iq_spectra_host.py)."""
    return sorted(_SIGS_IQ)


def exported_names_cplx():
    """Every symbol include/tempest_hip_cplx.h declares (kept in sync by tests/test_autocorr_complex_host.py)."""
    return sorted(_SIGS_CPLX)


def exported_names_hires():
    """Every symbol include/tempest_hip_hires.h declares (kept in sync by tests/test_hires_host.py)."""
    return sorted(_SIGS_HIRES)


def exported_names_register():
    """Every symbol include/tempest_hip_register.h declares (kept in sync by tests/test_register_host.py)."""
    return sorted(_SIGS_REGISTER)


def exported_names_display():
    """Every symbol include/tempest_hip_display.h declares (kept in sync by tests/test_display_host.py)."""
    return sorted(_SIGS_DISPLAY)


def exported_names_fold():
    """Every symbol include/tempest_hip_fold.h declares (kept in sync by tests/test_fold_host.py)."""
    return sorted(_SIGS_FOLD)


def exported_names_cfold():
    """Every symbol include/tempest_hip_cfold.h declares (kept in sync by tests/test_cfold_host.py)."""
    return sorted(_SIGS_CFOLD)


def exported_names_cstack():
    """Every symbol include/tempest_hip_cstack.h declares (kept in sync by tests/test_cstack_host.py)."""
    return sorted(_SIGS_CSTACK)


def exported_names_ctrack():
    """Every symbol include/tempest_hip_ctrack.h declares (kept in sync by tests/test_ctrack_host.py)."""
    return sorted(_SIGS_CTRACK)


def exported_names_gram():
    """Every symbol include/tempest_hip_gram.h declares (kept in sync by tests/test_gram_host.py)."""
    return sorted(_SIGS_GRAM)


def exported_names_tune():
    """Every symbol include/tempest_hip_tune.h declares (kept in sync by tests/test_tune_host.py)."""
    return sorted(_SIGS_TUNE)


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64.  Two HIP runtimes in one
    process cannot both own the GPU (whichever initialises second sees no device), and the dynamic
    loader de-duplicates by SONAME only in load order.  So when torch is installed, import it BEFORE
    dlopen-ing libtempest_hip.so: its runtime then serves both.  Without torch (e.g. under the Julia
    shim) the system ROCm runtime is used.  TSDR_NO_TORCH_PRELOAD=1 skips this."""
    if os.environ.get("TSDR_NO_TORCH_PRELOAD"):
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def load():
    """dlopen the library and attach prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    _share_torch_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise TempestHIPError(
            f"{LIB_PATH} not found: build it with `python tempestsdr.jl_amd/build.py` "
            "(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(_SIGS.items()) + list(_SIGS_IQ.items()) + list(_SIGS_CPLX.items()) + list(_SIGS_HIRES.items()) + \
            list(_SIGS_REGISTER.items()) + list(_SIGS_DISPLAY.items()) + list(_SIGS_FOLD.items()) + list(_SIGS_CFOLD.items()) + \
            list(_SIGS_CSTACK.items()) + list(_SIGS_CTRACK.items()) + list(_SIGS_GRAM.items()) + list(_SIGS_TUNE.items()):
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(ctx_handle, rc, what=""):
    """Map a tsdr_status to the exception class the reference function would throw."""
    if rc == TSDR_OK:
        return
    lib = load()
    detail = lib.tsdr_last_error(ctx_handle).decode() if ctx_handle else ""
    msg = f"{what}: {lib.tsdr_strerror(rc).decode()}" + (f" [{detail}]" if detail else "")
    if rc == TSDR_EINVAL:
        raise AssertionError(msg)  # @assert / MethodError in the reference
    if rc == TSDR_EBOUNDS:
        raise IndexError(msg)  # BoundsError
    if rc == TSDR_ENOMEM:
        raise MemoryError(msg)
    raise TempestHIPError(msg)
