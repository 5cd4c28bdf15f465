/*
 * tempest_hip_cplx.h -- calculate_autocorrelation (Autocorrelations.jl:23-37) of COMPLEX input: the coherent autocorrelation of
 * the IQ samples themselves, with no squaring before the correlation.  Part of the C ABI of libtempest_hip.so: tempest_hip.h
 * includes this file once; include tempest_hip.h, not this file.
 *
 * The reference function is untyped: ifft(fft(x[1:n]) .* conj(fft(x[1:n]))) followed by abs2 / 10log10 is defined for a complex
 * x, and a TempestSDR.jl user can call it on sigRx directly.  tsdr_autocorr* (tempest_hip.h) takes a real sequence, or IQ whose
 * abs2 it forms first; the entry points below correlate the complex samples.
 *
 *  1. SEMANTICS.  indexMin = 1 + round(minDelay*Fs), indexMax = round(maxDelay*Fs), n = min(2*indexMax, len), k0 = indexMin - 1,
 *     cnt = indexMax - indexMin + 1 and the TSDR_EBOUNDS cases are tsdr_autocorr's, unchanged.  With z = the first n samples,
 *         r[k] = sum_m z[(m+k) mod n] * conj(z[m])  =  ifft(fft(z) .* conj(fft(z)))[k]      (inverse scale 1/n)
 *     and out[i] = p or 10*log10f(p), p = re*re + im*im of r[k0+i], i < cnt (order and rounding of getSpectrum's output).  The
 *     power spectrum between the transforms is re*re + im*im of each bin with a zero imaginary part.  *n_out = cnt.
 *  2. BIT IDENTITY.  The integer forms (TSDR_IQ_SC16 / _SC8 / _UC8; iq, iq_fmt, scale as in tsdr_frames_iq_d) equal, bit for bit,
 *     the ComplexF32 form on the same samples expanded on the host with (q.astype(float32) - offset) * float32(scale): the lags,
 *     and idx and val of the search.  No tolerance: the loaders form the same f32 values and everything behind them is the
 *     ComplexF32 route's arithmetic.
 *  3. ROUTES.  The route depends on n alone, never on the format or the alignment.
 *     - n = 2^a 3^b 5^c taking two or more passes (tsdr_fft_plan(n) >= 2: 4096, 80 000, 4e6, 1e7, 4e7 ...): two native length-n
 *       transforms and nothing else.  The first forward pass reads the samples as stored (integer IQ is never expanded in HBM),
 *       the first inverse pass forms |Z|^2 while it loads, the last inverse pass writes abs2 / 10log10 of the lags k0 .. k0+cnt
 *       and nothing beyond them, and carries the search's findmax.
 *     - every other n (one-pass lengths such as 200 or 1000; lengths with a prime factor above 5, which take Bluestein's
 *       chirp-z transform: 4001, 100 003): forward transform (integer samples are expanded into context workspace first, as
 *       tsdr_spectrum_iq_d does), one pointwise power kernel, inverse transform, one finish kernel; the search runs
 *       tsdr_argmax_d's kernel over the window.
 *     - ComplexF64: fft64.hip's transform around the same three pointwise steps, all in f64 (tsdr_autocorr_f64's sequence with
 *       a copying loader).
 *     tsdr_set_option "ac_mixed" = 0 sends the non-power-of-two lengths of the first route down the second (a measurement switch).
 *  4. ALIGNMENT.  z / iq is aligned to ONE SAMPLE -- 8 bytes for ComplexF32, 4 for sc16, 2 for sc8 / uc8, 16 for ComplexF64 -- and
 *     base + k * bytes_per_sample of a larger buffer is valid for every k and gives the bits of a fresh allocation.  out is
 *     float-aligned (double-aligned in the f64 forms).  A pointer that is not, or an unknown iq_fmt, is TSDR_EINVAL with the
 *     argument's name (z, iq, iq_fmt, out) in tsdr_last_error, before anything is enqueued.
 *  5. EDGE CASES.  cnt == 0 (minDelay*Fs >= maxDelay*Fs) is TSDR_OK with *n_out = 0 and nothing written.  len < indexMax is
 *     TSDR_EBOUNDS (the BoundsError at :33).  NULL ctx / z / iq / out is TSDR_EINVAL.  n >= 2^31 is TSDR_EINVAL.  The input is
 *     never written; nothing is written outside out[0 .. cnt).
 * The host-pointer forms (what the Julia shim binds) stage n samples -- the RAW bytes of an integer format, 2 or 4 per sample, not
 * expanded ones -- run the device form and copy cnt values back.  The `_d` forms enqueue on the context's stream and return;
 * tsdr_autocorr_cplx_search_iq_d with a window blocks like tsdr_argmax_d.
 */
#ifndef TEMPEST_HIP_CPLX_H
#define TEMPEST_HIP_CPLX_H
#ifndef TEMPEST_HIP_H
#error "include tempest_hip.h, which includes tempest_hip_cplx.h"
#endif
/* calculate_autocorrelation(x::Vector{ComplexF32}, ...): z = len interleaved (re, im) pairs     Autocorrelations.jl:23-37 */
int tsdr_autocorr_cplx(tsdr_ctx *ctx, const float *z, size_t len, double Fs, double minDelay, double maxDelay,
                       int log_scale, float *out, size_t *n_out);
int tsdr_autocorr_cplx_d(tsdr_ctx *ctx, const float *z, size_t len, double Fs, double minDelay, double maxDelay,
                         int log_scale, float *out, size_t *n_out);
/* the same of len samples of format iq_fmt (any TSDR_IQ_*; TSDR_IQ_CF32 is tsdr_autocorr_cplx, scale ignored), host pointers */
int tsdr_autocorr_cplx_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t len, double Fs, double minDelay,
                          double maxDelay, int log_scale, float *out, size_t *n_out);
/* the complex twin of tsdr_autocorr_search_iq_d (GUI.jl:73-81 on the raw IQ): the lag vector as above, plus findmax over
 * out[win_lo .. win_lo + win_cnt) -- first maximum, NaN maximal, *idx 0-based inside the window, *val its value; blocking like
 * tsdr_argmax_d.  A window outside the lag vector is TSDR_EBOUNDS.  win_cnt == 0: the plain device call for that format (idx
 * and val are not touched, nothing is waited for). */
int tsdr_autocorr_cplx_search_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t len, double Fs, double minDelay,
                                   double maxDelay, int log_scale, float *out, size_t *n_out, size_t win_lo, size_t win_cnt,
                                   size_t *idx, float *val);
/* calculate_autocorrelation(x::Vector{ComplexF64}, ...): z = len interleaved (re, im) Float64 pairs, out Float64 */
int tsdr_autocorr_cplx_f64(tsdr_ctx *ctx, const double *z, size_t len, double Fs, double minDelay, double maxDelay,
                           int log_scale, double *out, size_t *n_out);
int tsdr_autocorr_cplx_f64_d(tsdr_ctx *ctx, const double *z, size_t len, double Fs, double minDelay, double maxDelay,
                             int log_scale, double *out, size_t *n_out);
#endif /* TEMPEST_HIP_CPLX_H */
