/*
 * tempest_hip_ctrack.h -- carrier tracking: a frame phase probe, and coherent stacking along a phase track, on the GPU.  Part of the C
 * ABI of libtempest_hip.so: tempest_hip.h includes this file once, after tempest_hip_cstack.h; include tempest_hip.h, not this file.
 *
 * tempest_hip_cfold.h and tempest_hip_cstack.h turn frame f by f*kappa (+ phi) turns: ONE constant carrier advance per frame for the
 * whole call, and the same phase on every line of a frame.  Two things a real capture does break that.  A carrier that drifts inside
 * a buffer (an oscillator's few Hz/s at a 700 MHz harmonic are 0.01 turns per frame per frame) has no constant kappa: the best one
 * folds 24 frames at -10 dB to a picture no better than the envelope fold's.  And a retune between buffers moves kappa by whole turns
 * per frame as well as by a fraction: kappa = frac(nu*T) keeps the fraction only, the integer part is a phase ramp ALONG each frame
 * that the state remembers, so the new buffer's picture no longer matches the state line by line and the lock finds no coherence.
 * Both are one capability: the weight of a sample becomes a function of frame and line, given as data (the TRACK); and a frame's phase
 * against a picture is one number measured with the processing gain of all P pixels -- measurable long before the frame's own picture
 * is visible (the PROBE).  The host fits the probe's phases and refolds along the fitted track (refine_track of the bindings).  The
 * entry points below go beyond the reference and change nothing that exists.
 *
 *  1. INPUT.  As tempest_hip_cstack.h, 1.: iq, n, the format rule, the geometry y_t x x_t with P = y_t*x_t, t0, T, F = n_frames, the
 *     converted samples z[k] as complex f32 pairs, amax = max_k |z[k]|; for the stack alpha, mode, zstate, mag, info.  iq is never written.
 *  2. TRACK.  2F doubles: (a_f, b_f) = track[2f], track[2f + 1], in turns, for frame f.  The weight of frame f on raster line l:
 *       c_l = fl64((l + 1/2) / y_t);   x = fma(b_f, c_l, a_f);   w_f(l) = the weight of tempest_hip_cfold.h, 3. at x:
 *       r = x - floor(x),  w = (f32(cospi(2 r)), f32(-sinpi(2 r))), sine and cosine evaluated in f64 and rounded once.
 *     a_f is the frame's phase at its start, b_f its advance over the frame (kappa's integer and fractional part alike).  The phase
 *     is piecewise constant per line: against the linear ramp it stands for, the error inside a line is at most |b_f| / (2 y_t) turns,
 *     and the caller keeps it small (|b_f| <= y_t / 20 keeps it below 1/40 turn: a loss of coherence below 1 %).
 *     With b_f == 0, x = a_f exactly.  The accuracy bounds hold for |a_f| + |b_f| <= 2^20 (x then carries at most 2^-33 turns of f64
 *     rounding; larger entries are accepted and lose phase resolution in proportion).  A device pointer (8-byte aligned) in the `_d`
 *     forms, a host pointer in the host forms.  The track is never written.
 *  3. SAMPLING.  Exactly tempest_hip_cfold.h, 2.: u_f(m), the clamps, the taps and the blend z_f(m) of pixel m = l*x_t + p, frame f.
 *
 * The stack: tsdr_ctrack_stack_iq_d / tsdr_ctrack_stack_iq
 *  4. RESULT.  tempest_hip_cstack.h, 4. - 6. with w_f(l) in place of w_f:  Z(m) = (1/F) sum_f w_f(l) z_f(m), then rho, E_z, E_s, q
 *     (GIVEN / LOCK), the blend into zstate, mag and info, operation for operation.  With alpha == 0 the state is NOT READ.
 *     TIE: with a_f = fl64(fl64(f * kappa) + phi) and b_f = 0 (constant_track of the bindings), zstate, mag and info
 *     have the bits of tsdr_cstack_iq_d at (kappa, phi) in both modes: the two build the weight, the sum, the epilogue, the lock and
 *     the blend from the same code (csrc/coherent_ops.h, csrc/raster_cstack.hip), and fma(0, c_l, a_f) == a_f.
 *  5. ACCURACY.  tempest_hip_cstack.h, 7., every bound as it stands: the fma of 2. is one f64 rounding of the phase (<= 2^-33 turns
 *     inside the domain of 2.: 2 pi 2^-33 of a term's magnitude, below 2^-6 u) where the constant-kappa weight has two.  ref: the
 *     formulas in exact arithmetic on the same z, S, f32(alpha) and the same doubles of the track, with c_l exact.
 *  6. REFUSALS.  tempest_hip_cstack.h, 10. without kappa and phi, and: track NULL; in the device form track not 8-byte aligned; in the
 *     host form a track entry that is not finite.  The device form cannot read the entries: a non-finite a_f or b_f there gives NaN
 *     weights on every line of that frame and so NaN pixels throughout.  F == 0 is TSDR_OK and touches nothing.
 *  7. COST.  The kernel is cstack's with one difference: 64 lanes evaluate the 64 lines' weights of the tile into LDS at each frame's
 *     start (64 f64 sine / cosine pairs per tile and frame, 1 KiB of LDS), under the barrier that publishes the staging table, and a
 *     lane reads its own line's weight.  Nothing is added per pixel.  tsdr_profile_get names "ctrack_stack_tile" /
 *     "ctrack_stack_direct", then "cstack_lock" and "cstack_blend" as tempest_hip_cstack.h, 11. says.
 *
 * The probe: tsdr_ctrack_probe_iq_d / tsdr_ctrack_probe_iq
 *  8. RESULT.  zref: P interleaved (re, im) f32 pairs in state order (pixel (l, p) at pair index p*y_t + l), S(m); never written.
 *     track may be NULL: the zero track (w = (1, -0): the same arithmetic on a = b = 0, the bits of an all-zero track).  For f < F:
 *       v_f(m) = w_f(l) * z_f(m)           in f32: re = fsub(fmul(wr, zr), fmul(wi, zi)), im = fadd(fmul(wr, zi), fmul(wi, zr))
 *       rho_f  = sum_m v_f(m) conj(S(m))   f64: Re += vr*sr + vi*si, Im += vi*sr - vr*si, the products in f64 of the f32 values
 *       E_f    = sum_m |v_f(m)|^2,   E_s = sum_m |S(m)|^2                likewise
 *       out[4f .. 4f+3] = Re rho_f, Im rho_f, E_f, gamma_f;   gamma_f = |rho_f| / sqrt(E_f * E_s), 0 unless that product is > 0
 *       out[4F] = E_s
 *     arg(rho_f) / (2 pi) is the phase, in turns, by which frame f LEADS the reference after the track's turn: adding it to a_f
 *     brings the frame onto S (fit_track of the bindings).  The sums run per lane in pixel order, over the 64 lanes by a fixed
 *     shuffle tree, in wave order, then over the tiles in tile order (one lane per frame).  No float atomics.
 *  9. ACCURACY.  u = 2^-24.  A term v_f(m) is tempest_hip_cfold.h, 5.'s term without the accumulation over frames: blend, weight
 *     rounding, the products and their sum, the coordinate -- <= 8.5 u*amax per component, budgeted as there:
 *       |v - ref| <= sqrt(2) * 12 * u * amax = eps_t                 (the F-independent part of eps_z; the track's fma: 2.)
 *     v enters the f64 sums with that error, S exactly; the sums are less than 2^16 additions deep for every accepted geometry:
 *       |rho_f - ref| <= eps_t * sqrt(P * E_s) + 2^-36 * sqrt(E_f * E_s)                       (Cauchy-Schwarz)
 *       |E_f - ref|   <= 2 * eps_t * sqrt(P * ref) + P * eps_t^2 + 2^-36 * ref,     |E_s - ref| <= 2^-36 * ref
 *     gamma_f follows from the three within those bounds.
 * 10. REPRODUCIBILITY, FORMAT INVARIANCE (both operations).  Two calls with the same arguments leave identical bits in every
 *     output; integer formats give the bits of the host-expanded ComplexF32 buffer.
 * 11. REFUSALS of the probe.  TSDR_EINVAL, with nothing written and nothing enqueued, for everything tempest_hip_cfold.h, 9. refuses of
 *     a fold's geometry (a NULL ctx or iq; an unknown format; y_t <= 0, x_t <= 0, P >= 2^31; n < 2 or n >= 2^31; F < 0; T or t0 not
 *     finite; T < 2; t0 < 0; t0 + F*T > n; iq not aligned), and for: zref or out NULL; in the device form zref, out or a non-NULL track
 *     not 8-byte aligned; in the host form a track entry that is not finite.  F == 0 is TSDR_OK and writes nothing, out[0] included.
 *     Nothing is written outside out[0 .. 4F].
 * 12. COST of the probe.  "ctrack_probe_tile" / "ctrack_probe_direct" have the coherent fold's tiles, staging and staged / direct
 *     choice (TSDR_CFOLD_STAGE_MAX).  A lane holds S of its 16 (direct: 4) pixels in registers for the whole frame loop, reads the
 *     IQ once and the reference once (8n + 8P bytes), and per frame reduces three f64 sums -- six f64 multiply-adds per pixel and
 *     frame, one shuffle tree and one more barrier per frame -- into the context's workspace, [frame][tile][4] doubles.
 *     "ctrack_probe_sum" adds the tiles, one lane per frame.  Measured times: profiles/ctrack.json, DESIGN.md section 4.
 * The `_d` forms take device pointers, enqueue on the context's stream and return.  The host-pointer forms upload iq, the track
 * (and zstate when alpha != 0; zref), run the device form and copy the outputs back; their wait is bounded like every other host
 * form's (option "wait_ms").
 */
#ifndef TEMPEST_HIP_CTRACK_H
#define TEMPEST_HIP_CTRACK_H
#ifndef TEMPEST_HIP_CSTACK_H
#error "include tempest_hip.h, which includes tempest_hip_ctrack.h after tempest_hip_cstack.h"
#endif
/* tsdr_cstack_iq_d along a track: frame f, line l turned by -(a_f + b_f*(l + 1/2)/y_t) turns, (a_f, b_f) = track[2f], track[2f+1]
 * (1. - 7. above), device pointers */
int tsdr_ctrack_stack_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                           int n_frames, int y_t, int x_t, float alpha, int mode, float *zstate, float *mag, double *info);
/* the same with host pointers: upload, run, download zstate, mag, info */
int tsdr_ctrack_stack_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                         int n_frames, int y_t, int x_t, float alpha, int mode, float *zstate, float *mag, double *info);
/* every frame's inner product with the reference picture zref after the track's turn (track may be NULL): out[4f .. 4f+3] = Re rho_f,
 * Im rho_f, E_f, gamma_f, out[4*n_frames] = E_s (8. - 12. above), device pointers */
int tsdr_ctrack_probe_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                           int n_frames, int y_t, int x_t, const float *zref, double *out);
/* the same with host pointers: upload, run, download out */
int tsdr_ctrack_probe_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                         int n_frames, int y_t, int x_t, const float *zref, double *out);
#endif /* TEMPEST_HIP_CTRACK_H */
