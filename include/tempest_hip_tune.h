/*
 * tempest_hip_tune.h -- the tuner: frequency shift, real FIR low-pass and decimation of an IQ stream, on the GPU.  Part of the C ABI
 * of libtempest_hip.so: tempest_hip.h includes this file once, after tempest_hip_gram.h; include tempest_hip.h, not this file.
 *
 * Every other entry point takes the capture for the channel: the leak at the centre of the sampled band, alone in it.  A wideband
 * capture holds the harmonic the user wants and much beside it; |IQ| is nonlinear, so one strong carrier anywhere in the band ruins
 * the envelope picture, and the coherent paths pay the whole band's noise and samples.  The entry points below move a band to
 * baseband, reject what lies beside it and lower the rate; what they return is a ComplexF32 stream every other entry point takes.
 * They go beyond the reference and change nothing that exists.
 *
 *  1. STREAM, OSCILLATOR.  x[m] is the stream, m an ABSOLUTE sample index (uint64).  The oscillator is a 64-bit phase accumulator,
 *     exact by construction:
 *       p[m] = (phi_fix + nu_fix * m) mod 2^64,   w[m] = exp(2 pi i p[m] / 2^64)
 *     nu_fix, phi_fix: uint64, in turns * 2^64; the integer arithmetic wraps.  No phase error grows with m, and no result depends on
 *     how the stream was cut into calls.  In f32, (c, s) = (cos, sin)(2 pi p / 2^64) are formed as: t = f64(int64(p)) * 2^-63 (p taken
 *     as a signed number: a whole turn less for p >= 2^63; the conversion rounds to nearest), then the f64 sincospi(t), each of the
 *     two rounded to f32.  Phase 0 gives w = (1, 0) exactly.
 *  2. MIXED SAMPLE.  u[m] = x[m] * w[m] in f32, x[m] = (xr, xi) the sample as the loaders of tempest_hip.h expand it (ComplexF32 as
 *     stored; integer IQ (q - offset) * scale, one rounding):
 *       re = fsub(fmul(xr, c), fmul(xi, s)),   im = fadd(fmul(xr, s), fmul(xi, c))
 *     Its bits are a function of x[m]'s bits and of p[m] alone.
 *  3. OUTPUT.  y[j] = sum_{i=0}^{L-1} h[i] * u[j*D + i] for every j whose window [j*D, j*D + L) lies inside the stream:
 *     only complete windows, no padding.  h: L = n_taps real f32 taps, 1 <= L <= TSDR_TUNE_TAPS_MAX; D = decim, 1 <= D <= TSDR_TUNE_DECIM_MAX.
 *     ORDER: one chain per component, i ascending: acc = +0; acc = fmaf(h[i], u[j*D + i], acc) for i = 0, 1, ..., L-1; y[j] = acc.
 *     The order is a function of L only -- never of n, m0, the tile, the format or the chunking.  (A lane runs the chains of four
 *     neighbouring outputs side by side: eight independent chains, which is the instruction-level parallelism; a chain is not split.)
 *  4. A CALL.  iq[0] is x[m0]; iq, iq_fmt, scale as in tsdr_frames_iq_d (TSDR_IQ_*; integer IQ is never expanded in memory).  hist holds
 *     L-1 ComplexF32; its LAST n_hist entries are u[m0 - n_hist .. m0), left by the previous call.  The call writes y[j] for
 *     j0 <= j <= j1 to out[0 .. n_out) (ComplexF32), j1 = floor((m0 + n - L) / D) (no output when m0 + n < L), n_out = j1 - j0 + 1 or 0,
 *     then leaves in hist the last min(L-1, n_hist + n) mixed samples, right-aligned (entries in front of them keep their bytes).
 *     *n_out is a host value, computed before anything is enqueued.  hist == NULL is allowed exactly when n_hist == 0 and the caller
 *     does not chain: then no history is written.  n == 0 or n_out == 0 is TSDR_OK; the history is still carried forward.
 *     Nothing is written outside out[0 .. n_out) and hist; iq and taps are never written.
 *  5. CHAINING.  A stream cut into calls at ANY boundaries -- chunks shorter than L-1, chunks of one sample, chunks that are no multiple
 *     of D -- gives, bit for bit, the outputs (and the final hist) of one call on the whole stream, when every call passes the m0, j0
 *     and n_hist the previous one left (tune_plan of the bindings: m0 += n, j0 += n_out, n_hist = min(L-1, n_hist + n)).
 *  6. FORMATS.  An integer format's outputs equal, bit for bit, the ComplexF32 form's on the samples expanded on the host with
 *     (f32(q) - offset) * f32(scale) (tsdr_iq_expand_d's values).
 *  7. REPEATS.  A repeated call returns the same bits.  No float atomics; every y[j] and every u[m] is computed by one lane.
 *  8. ERROR BOUND.  u = 2^-24; A = the largest modulus of the call's expanded samples (the history's included), H1 = sum |h[i]|;
 *     y_ref: the formulas above in f64 on the f32 samples, the f32 taps and the exact phases.
 *       |y[j] - y_ref[j]| <= (L + 8) * u * A * H1
 *     To first order, in units of u * A * H1: 1 for the sample's conversion (the product by scale); at most 4 for w; 3 for the complex
 *     product (two products and a sum per component); L for a chain of L fmafs.  THE OSCILLATOR'S TERM: int64 -> f64 rounds by at most
 *     2^-53 relative, |t| <= 1, so the angle pi t is off by at most pi 2^-53; the f64 sincospi errs by a few units of 2^-53; rounding
 *     each of c, s to f32 adds at most 2^-25 to each.  |w_computed - w| <= sqrt(2) * 2^-25 + 2^-50 < 0.71 u: inside the 4 u allowed.
 *  9. REFUSALS.  TSDR_EINVAL with the argument's name in tsdr_last_error, before anything is enqueued: a NULL ctx (no message: there is
 *     no context to hold one), iq, taps, out or n_out, whatever n is; an unknown iq_fmt; n_taps outside [1, TSDR_TUNE_TAPS_MAX]; decim outside
 *     [1, TSDR_TUNE_DECIM_MAX]; n >= 2^31; m0 + n >= 2^64 (m0); n_hist outside [0, L-1] or above m0, or n_hist > 0 with hist NULL
 *     (n_hist / hist); j0 * D < m0 - n_hist, the window reaching before the history (j0); out_cap < n_out (out_cap); in the device
 *     form an iq not aligned to one sample of its format, a taps, hist or out not float-aligned (4 bytes).
 * 10. COST.  "tune": one workgroup of 256 lanes makes a tile of tsdr_tune_tile(L, D) outputs (4 neighbouring outputs per lane; 1024 at
 *     (63, 4), 80 at (1024, 64)): it mixes the (tile - 1) * D + L samples the tile needs ONCE into LDS -- the left edge from hist where
 *     the tile reaches before iq[0] --, then every lane reads its (L + 3 D) samples once each and feeds up to four chains per read;
 *     the taps are scalar loads (uniform across a wavefront).  LDS rows of 4 D samples are padded by one, so that the 4 D-strided
 *     reads of a wavefront's lanes fall on different banks; at most 48 KiB.  No grid cap: one workgroup per tile.  "tune_hist": a
 *     second launch of one workgroup behind it on the stream updates hist in place (read, barrier, write).
 *     Measured on one MI355X: profiles/tune.json, DESIGN.md section 4.
 * NOT BUILT: complex taps; rational resampling; a fused tune + detector; a tuner inside the frame loop; L > 1024.
 * The `_d` form takes device pointers (n_out: a host pointer), enqueues on the context's stream and returns.  The host-pointer form
 * uploads iq, taps and hist, runs the device form and copies out[0 .. n_out) and hist back; its wait is bounded like every other host
 * form's (option "wait_ms").
 */
#ifndef TEMPEST_HIP_TUNE_H
#define TEMPEST_HIP_TUNE_H
#ifndef TEMPEST_HIP_GRAM_H
#error "include tempest_hip.h, which includes tempest_hip_tune.h after tempest_hip_gram.h"
#endif
#define TSDR_TUNE_TAPS_MAX 1024
#define TSDR_TUNE_DECIM_MAX 64
/* out[0 .. *n_out) = y[j0 ..], hist carried forward (1. - 10. above), device pointers; n_out is a host pointer */
int tsdr_tune_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, uint64_t m0, uint64_t nu_fix, uint64_t phi_fix,
                   const float *taps, int n_taps, int decim, uint64_t j0, float *hist, int n_hist, float *out, size_t out_cap,
                   size_t *n_out);
/* the same with host pointers: upload, run, download out and hist */
int tsdr_tune_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, uint64_t m0, uint64_t nu_fix, uint64_t phi_fix,
                 const float *taps, int n_taps, int decim, uint64_t j0, float *hist, int n_hist, float *out, size_t out_cap,
                 size_t *n_out);
/* outputs per workgroup of the "tune" kernel for these n_taps and decim (a multiple of 4), or TSDR_EINVAL when either is out of
 * range: what a test needs to place a call at a tile's edge.  No context, nothing enqueued */
int tsdr_tune_tile(int n_taps, int decim);
#endif /* TEMPEST_HIP_TUNE_H */
