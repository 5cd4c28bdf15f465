/*
 * tempest_hip_fold.h -- coherent frame folding at a fractional frame period, on the GPU.  Part of the C ABI of libtempest_hip.so:
 * tempest_hip.h includes this file once, after tempest_hip_display.h; include tempest_hip.h, not this file.
 *
 * The frame loop cuts a buffer into floor(nEch / S) frames of S = round(Fs/fv) samples (GUI.jl:103-109,137,166) and moves every frame
 * onto the previous ones by its own vsync indices.  A monitor's frame period T = Fs/fv is not an integer number of samples, but it
 * is constant: a buffer of n samples holds F = floor((n - t0) / T) frames that are already aligned with each other when they are
 * sampled at t0 + f*T + ... instead of f*S + ....  Summing them pixel by pixel is epoch folding: the noise drops by sqrt(F) before
 * anything has to be detected, the picture's origin is found once, on the folded picture, and the phase t0 carries across buffers.
 * Folding at trial periods and keeping the sharpest picture (SCORE) refines T below the one lag the autocorrelation peak gives.
 * The entry points below go beyond the reference and change nothing that exists.
 *
 *  1. INPUT.  iq: n samples on the device in one of the TSDR_IQ_* formats, converted by the one rule of tempest_hip.h (scale is
 *     ignored for TSDR_IQ_CF32); a[k] = |IQ[k]| as f32.  A geometry y_t x x_t, P = y_t*x_t.  A start t0 and a period T, both double,
 *     in samples.  A frame count F = n_frames.  iq is never written.
 *  2. SAMPLING.  For pixel m = l*x_t + p (line l, pixel p; stored at state[p*y_t + l], the column-major (y_t, x_t) layout of
 *     tsdr_sig_to_image) and frame f = 0 .. F-1:
 *       u_f(m) = (t0 + f*T) + ((m + 1/2)*(T/P) - 1/2)     in f64 -- imresize's pixel-centre rule on a continuous stream
 *       u <- clamp(u, 0, n-1);  k = min(floor(u), n-2);  d = u - k   (d may be 1)
 *       v_f(m) = a[k] + d*(a[k+1] - a[k])                 one f32 result
 *       mean(m) = (1/F) * sum_f v_f(m)
 *       state(m) <- alpha == 0 ? mean(m) : fadd(fmul(alpha, state(m)), fmul(fsub(1, alpha), mean(m)))
 *     With alpha == 0 the state is NOT READ: an uninitialised or NaN state is simply overwritten (the first buffer's call).
 *     With F = 1, t0 = 0, T = n = S this is sig_to_image(amDemod(iq)), because the buffer clamp then equals the frame clamp.
 *     Otherwise the last half pixel of a frame interpolates into the next frame's first sample instead of clamping.
 *     The fold POINT-SAMPLES like imresize does: a strongly oversampled capture (many samples per pixel) is not box-filtered.
 *  3. ACCURACY.  The contract is an error bound, not a bit pattern; the summation order over f and the |IQ| flavour are the
 *     implementation's choice, and the result does not depend on tsdr_set_precision.  Per term: |IQ| <= 1.5 ulp, blend <= 1 ulp,
 *     coordinate error <= 2^-26 samples (t0 + f*T is split into integer and fractional part once per frame, the in-frame part is
 *     evaluated from the pixel index; no sum is carried along a line).  Sum over F non-negative terms: <= (F-1) ulp of the sum.  Division and
 *     the three IIR roundings: <= 4 ulp.  Together |state - ref| <= eps, eps = (F + 8) * 2^-24 * max(amax, max|state_in|),
 *     amax = max_k a[k].
 *  4. REPRODUCIBILITY.  Two calls with the same arguments leave identical bits: no floating-point atomics, partial sums are
 *     combined in a fixed order.
 *  5. FORMAT INVARIANCE.  Integer formats give the bits of the host-expanded ComplexF32 buffer.
 *  6. SCORE of a folded picture (the period scan).  Trial k folds at T0 + k*dT (f64, two roundings).  With x_m = (double)mean(m):
 *       score = sum_m x_m^2 - (sum_m x_m)^2 / P            in f64
 *     the picture's variance times P (not its energy, which the DC level dominates and which moves with the samples a trial
 *     covers).  From 3. (Cauchy-Schwarz): |score - ref| <= 2*eps*sqrt(P*ref) + P*eps^2.  The raster of a trial never leaves the
 *     registers: workgroups write f64 partial sums to the context's workspace, one lane per trial adds them in tile order.
 *     The host form also returns *best = the index of the first maximum; a NaN never wins (-1 when every score is NaN); best may be
 *     NULL.
 *  7. REFUSALS.  TSDR_EINVAL, with nothing written and nothing enqueued, for: a NULL ctx, iq, state or score; an unknown format;
 *     y_t <= 0, x_t <= 0, P >= 2^31; n < 2 or n >= 2^31; F < 0; T (T0), t0 or dT not finite; T < 2; t0 < 0; dT < 0;
 *     t0 + F*T > n, evaluated in f64 at the largest trial period T0 + (n_trials-1)*dT for the scan; alpha outside [0, 1] or NaN;
 *     n_trials < 1 or > TSDR_FOLD_MAX_TRIALS; state not 4-byte or score not 8-byte aligned; iq not aligned to one sample
 *     (TSDR_IQ_CF32: 8 bytes) or, for the integer formats, not 16-byte aligned (as tsdr_autocorr_search_iq_d).  The host forms
 *     have no alignment rule.  F == 0 (with everything else valid) is TSDR_OK and touches nothing.  Nothing is written outside
 *     state[0 .. P) or score[0 .. n_trials).
 *  8. COST.  A fold reads the IQ once and writes ONE raster per buffer: 8n + 8P bytes at ComplexF32 with alpha != 0 (the state is
 *     read and written once, at the end).  Two kernels serve it.  The tiled one: a 512-thread workgroup owns 64 lines x 128 pixels
 *     of the OUTPUT, loops over the F frames, stages per frame the |IQ| span of its lines in LDS (|IQ| once per staged sample) and
 *     keeps its 16 pixels per lane in registers.  It runs while a tile line's span, W = ceil(128*T/P) + 3 samples, is at most
 *     TSDR_FOLD_STAGE_MAX = 240 (64 KiB of LDS): up to about 1.85 samples per pixel.  Above that a direct, LDS-free kernel (64 lines
 *     x 16 pixels per workgroup) loads both taps of every pixel itself.  A scan decides at its largest trial period.
 *     tsdr_profile_get names the path: "fold_tile" / "fold_direct", "fold_scan_tile" / "fold_scan_direct" + "fold_score".
 * The `_d` forms take device pointers, enqueue on the context's stream and return.  The host-pointer forms upload iq (and state
 * when alpha != 0), run the device form and copy state / score back; their wait is bounded like every other host form's (option
 * "wait_ms").
 */
#ifndef TEMPEST_HIP_FOLD_H
#define TEMPEST_HIP_FOLD_H
#ifndef TEMPEST_HIP_DISPLAY_H
#error "include tempest_hip.h, which includes tempest_hip_fold.h after tempest_hip_display.h"
#endif
#define TSDR_FOLD_MAX_TRIALS 4096
#define TSDR_FOLD_STAGE_MAX 240
/* n_frames frames of period T from t0 -> their mean, IIR-averaged into the (y_t, x_t) state (1. - 5. above), device pointers */
int tsdr_fold_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, int n_frames, int y_t,
                   int x_t, float alpha, float *state);
/* the same with host pointers: upload, run, download state */
int tsdr_fold_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, int n_frames, int y_t,
                 int x_t, float alpha, float *state);
/* score[k] of the picture folded at T0 + k*dT, k < n_trials (6. above), device pointers */
int tsdr_fold_scan_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T0, double dT,
                        int n_trials, int n_frames, int y_t, int x_t, double *score);
/* the same with host pointers; *best = the first maximum */
int tsdr_fold_scan_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T0, double dT,
                      int n_trials, int n_frames, int y_t, int x_t, double *score, int *best);
#endif /* TEMPEST_HIP_FOLD_H */
