/*
 * tempest_hip_iq.h -- the device-pointer (`_d`) forms of GetSpectrum.jl's and Demodulation.jl's functions on integer IQ as the
 * SDR stored it (sc16, sc8, uc8), and the staging ring's expansion as a call.  Part of the C ABI of libtempest_hip.so:
 * tempest_hip.h includes this file, after the contract these entry points keep ("on integer IQ", BIT IDENTITY / ROUTES /
 * ALIGNMENT / EDGE CASES, above tsdr_spectrum_iq) and after their host-pointer twins; include tempest_hip.h, not this file.
 * `iq`, `iq_fmt` (TSDR_IQ_*) and `scale` mean what they mean in tsdr_frames_iq_d.
 */
#ifndef TEMPEST_HIP_IQ_H
#define TEMPEST_HIP_IQ_H
#ifndef TEMPEST_HIP_H
#error "include tempest_hip.h, which includes tempest_hip_iq.h"
#endif
/* getSpectrum(fs,sig;N) of integer IQ, device pointers          GetSpectrum.jl:21-30 */
int tsdr_spectrum_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t N, int lin, float *y);
/* getWelch(fe,sig;sizeFFT) of integer IQ, device pointers       GetSpectrum.jl:36-52 */
int tsdr_welch_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t len, size_t sizeFFT, int lin, float *y);
/* getWaterfall(fe,sig;sizeFFT) of integer IQ, device pointers   GetSpectrum.jl:54-66 */
int tsdr_waterfall_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t len, size_t sizeFFT, double *sMatrix);
/* amDemod Demodulation.jl:26-28 | abs2 GUI.jl:70 | invert_amDemod Demodulation.jl:31-35 | fmDemod Demodulation.jl:17-23 of integer
 * IQ: 16-byte vector loads (4 sc16 / 8 eight-bit samples) when iq and out are 16-byte aligned, one sample per lane otherwise --
 * the same bits either way */
int tsdr_am_demod_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, float *out);
int tsdr_abs2_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, float *out);
int tsdr_invert_am_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, float *out);
int tsdr_fm_demod_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, float *out);
/* the staging ring's expansion (AtomicAbstractSDRs.jl:177-190 hands recv! ComplexF32 buffers): n samples of iq_fmt -> n
 * ComplexF32 at cf32_out (TSDR_IQ_CF32: a copy) */
int tsdr_iq_expand_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, float *cf32_out);
#endif /* TEMPEST_HIP_IQ_H */
