/*
 * tempest_hip_cfold.h -- phase-coherent frame folding with carrier de-rotation, on the GPU.  Part of the C ABI of libtempest_hip.so:
 * tempest_hip.h includes this file once, after tempest_hip_fold.h; include tempest_hip.h, not this file.
 *
 * tempest_hip_fold.h folds the envelope a[k] = |IQ[k]|: it is coherent with the frame period only and discards the carrier phase
 * before it sums.  Below about 0 dB per sample an envelope detector suppresses the signal: the mean of |s + n| carries the picture
 * only through |s|^2/sigma, the post-detection SNR falls with the square of the input SNR, and sqrt(F) averaging cannot recover it.
 * A frame holds an integer number of pixel clocks, so the emission's phase at a given pixel advances by the same amount from every
 * frame to the next: kappa = frac(nu*T) turns, nu the residual carrier offset in cycles per sample.  Multiply frame f by
 * exp(-j*2*pi*f*kappa), sum the COMPLEX samples, and take the magnitude once at the end: the noise averages down before the
 * detector, not after it.  Scanning kappa and keeping the picture with the most energy (SCORE) finds the carrier: a periodogram
 * over frames.  The entry points below go beyond the reference and change nothing that exists.
 *
 *  1. INPUT.  As tempest_hip_fold.h, 1.: iq, n, the format rule, a geometry y_t x x_t with P = y_t*x_t, t0, T, F = n_frames -- except
 *     that z[k] is the converted sample as a complex f32 pair, not its magnitude; amax = max_k |z[k]|.  kappa (kappa0, dkappa) in
 *     turns per frame, double.  iq is never written.
 *  2. SAMPLING.  Exactly the fold's coordinates, for pixel m = l*x_t + p and frame f = 0 .. F-1:
 *       u_f(m) = (t0 + f*T) + ((m + 1/2)*(T/P) - 1/2)     in f64
 *       u <- clamp(u, 0, n-1);  k = min(floor(u), n-2);  d = u - k   (d may be 1)
 *       z_f(m) = z[k] + d*(z[k+1] - z[k])                 per component, one f32 result each: the blend the fold uses on a
 *     with the same once-per-frame split of t0 + f*T into an integer and a fractional part (coordinate error <= 2^-26 samples).
 *  3. WEIGHT.  x = fl64(f * kappa);  r_f = x - floor(x);  w_f = (f32(cospi(2 r_f)), f32(-sinpi(2 r_f))): the sine and cosine are
 *     evaluated in f64 and rounded once.  Only frac(kappa) matters: kappa and kappa + integer agree within the bound, not in bits.
 *     Any finite kappa, kappa0 and dkappa are accepted, negative ones included (a product f*kappa that overflows gives NaN).
 *  4. RESULT.
 *       Z(m) = (1/F) * sum_f w_f * z_f(m)     accumulated in complex f32, f = 0 .. F-1 in that order: per term the four products,
 *                                             re = fsub(fmul(wr, zr), fmul(wi, zi)), im = fadd(fmul(wr, zi), fmul(wi, zr)), one
 *                                             fadd per component into the sum; one fdiv per component by f32(F) at the end
 *       c(m) = |Z(m)| as f32
 *       state(m) <- alpha == 0 ? c(m) : fadd(fmul(alpha, state(m)), fmul(fsub(1, alpha), c(m)))
 *     stored at state[p*y_t + l], the column-major (y_t, x_t) layout of tsdr_sig_to_image.  With alpha == 0 the state is NOT READ.
 *     Across buffers the magnitudes are averaged, non-coherently: fold_plan carries t0 as it does for the envelope fold;
 *     a complex state across buffers is out of scope.  With kappa = 0 and a real non-negative z the result is
 *     the envelope fold of the same data within the two bounds.
 *  5. ACCURACY.  The contract is an error bound, not a bit pattern; the result does not depend on tsdr_set_precision.  With
 *     u = 2^-24, per component and per term, counted from the operation sequence above (every |component| <= |z| <= amax, |w| <= 1):
 *       blend: the f64 fma rounded once to f32                        <= 1 u*amax   (budgeted 3: the three-rounding f32 form)
 *       weight rounding: (u/2)(|zr| + |zi|)                           <= 1 u*amax   (budgeted 2)
 *       two products and their difference / sum                       <= 3 u*amax
 *       coordinate: 2^-26 samples * |z[k+1] - z[k]|                   <= 1/2 u*amax
 *     together <= 8.5 u*amax per term, which the mean over F terms keeps.  The F-term accumulation (partial sum j is at most j*amax:
 *     sum_j j*u*amax / F) and the division add <= ((F+1)/2 + 1) u*amax per component.  Two components:
 *       |Z - Zref| <= sqrt(2) * (F + 12) * u * amax = eps_z          (Zref: the formulas of 2. - 4. in exact arithmetic, exact weights)
 *     The square root (<= 2u) and the IIR's four roundings (<= 4u):
 *       |state - ref| <= 1.5 * (F + 16) * u * max(amax, max|state_in|) = eps_c
 *  6. REPRODUCIBILITY.  Two calls with the same arguments leave identical bits: no floating-point atomics, partial sums are
 *     combined in a fixed order.
 *  7. FORMAT INVARIANCE.  Integer formats give the bits of the host-expanded ComplexF32 buffer.
 *  8. SCORE of a folded picture (the carrier scan).  Trial k uses kappa_k = fl64(kappa0 + k*dkappa) at the one period T:
 *       score_k = sum_m ((double)Re Z_k(m))^2 + ((double)Im Z_k(m))^2            summed in f64
 *     the folded picture's energy: at a wrong kappa the carrier cancels and the score falls to the noise floor.
 *     No square root is taken and no raster is written.  From 5. (Cauchy-Schwarz): |score - ref| <= 2*eps_z*sqrt(P*ref) + P*eps_z^2.  A trial changes
 *     only the weights, not the sampling: a workgroup samples z_f(m) ONCE per frame for a batch of 8 trials.  Workgroups write f64
 *     partial energies to the context's workspace, one lane per trial adds them in tile order.  The host form also returns
 *     *best = the index of the first maximum; a NaN never wins (-1 when every score is NaN); best may be NULL.
 *  9. REFUSALS.  TSDR_EINVAL, with nothing written and nothing enqueued, for: a NULL ctx, iq, state or score; an unknown format;
 *     y_t <= 0, x_t <= 0, P >= 2^31; n < 2 or n >= 2^31; F < 0; T or t0 not finite; T < 2; t0 < 0;
 *     kappa, kappa0 or dkappa not finite; t0 + F*T > n, evaluated in f64 at the one T; alpha outside [0, 1] or NaN;
 *     n_trials < 1 or > TSDR_CFOLD_MAX_TRIALS; state not 4-byte or score not 8-byte aligned; iq not aligned to one sample
 *     (TSDR_IQ_CF32: 8 bytes) or, for the integer formats, not 16-byte aligned.  The host forms have no alignment rule.
 *     F == 0 (with everything else valid) is TSDR_OK and touches nothing.  Nothing is written outside state[0 .. P) or
 *     score[0 .. n_trials).
 * 10. COST.  A fold reads the IQ once and writes one raster: 8n + 8P bytes at ComplexF32 with alpha != 0.  The tiled kernel has the
 *     envelope fold's shape (512 threads own 64 lines x 128 pixels of the output, 16 pixels per lane, two f32 sums per pixel) but
 *     stages float2 samples, twice the LDS per sample: it runs while a tile line's span W = ceil(128*T/P) + 3 is at most
 *     TSDR_CFOLD_STAGE_MAX = 120 (64 KiB of LDS), about 0.9 samples per pixel; above that the direct kernel (64 lines x 16 pixels)
 *     loads both taps itself.  The scan makes the same choice and runs 64 lines x 32 pixels per workgroup (tiled) or 64 x 16
 *     (direct), 4 pixels per lane x 8 trials in registers: K trials read the IQ ceil(K/8) times and cost 8*F*P flops each.
 *     tsdr_profile_get names the path: "cfold_tile" / "cfold_direct", "cfold_scan_tile" / "cfold_scan_direct" + "cfold_score".
 *     Measured on one MI355X (profiles/cfold.json; 30 frames, ComplexF32): C2 (2576x1125) fold 130.0 us beside the envelope fold's
 *     118.0 us (1.10x), C5 (4400x2250) 301.5 beside 265.0 us (1.14x); a 120-trial scan 48.1 us per trial at C2 beside 79.7 us per
 *     trial of a 17-trial envelope scan (0.60x), 161.9 beside 229.2 us at C5 (0.71x).  Kernels and registers: DESIGN.md section 4.
 * The `_d` forms take device pointers, enqueue on the context's stream and return.  The host-pointer forms upload iq (and state
 * when alpha != 0), run the device form and copy state / score back; their wait is bounded like every other host form's (option
 * "wait_ms").
 */
#ifndef TEMPEST_HIP_CFOLD_H
#define TEMPEST_HIP_CFOLD_H
#ifndef TEMPEST_HIP_FOLD_H
#error "include tempest_hip.h, which includes tempest_hip_cfold.h after tempest_hip_fold.h"
#endif
#define TSDR_CFOLD_MAX_TRIALS 4096
#define TSDR_CFOLD_STAGE_MAX 120
/* n_frames frames of period T from t0, frame f turned by -f*kappa turns, summed as complex samples -> |mean|, IIR-averaged into the
 * (y_t, x_t) state (1. - 7. above), device pointers */
int tsdr_cfold_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, int n_frames,
                    int y_t, int x_t, float alpha, float *state);
/* the same with host pointers: upload, run, download state */
int tsdr_cfold_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, int n_frames,
                  int y_t, int x_t, float alpha, float *state);
/* score[k] = the energy of the complex picture folded at kappa0 + k*dkappa, k < n_trials (8. above), device pointers */
int tsdr_cfold_scan_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa0,
                         double dkappa, int n_trials, int n_frames, int y_t, int x_t, double *score);
/* the same with host pointers; *best = the first maximum */
int tsdr_cfold_scan_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa0,
                       double dkappa, int n_trials, int n_frames, int y_t, int x_t, double *score, int *best);
#endif /* TEMPEST_HIP_CFOLD_H */
