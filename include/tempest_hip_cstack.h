/*
 * tempest_hip_cstack.h -- coherent stacking across buffers: a COMPLEX fold state and a phase lock, on the GPU.  Part of the C ABI of
 * libtempest_hip.so: tempest_hip.h includes this file once, after tempest_hip_cfold.h; include tempest_hip.h, not this file.
 *
 * tempest_hip_cfold.h sums complex samples within one call and averages MAGNITUDES across calls: its state is |Z|.  A viewer sits on
 * one target for hundreds of buffers, and below about -12 dB per sample the |Z| of one buffer (8 - 30 frames) is mostly noise floor,
 * which averaging magnitudes cannot undo.  Here the complex state exists: the state keeps Z itself, every call turns its own Z onto
 * the state and blends the two as complex numbers, and the magnitude is taken once, of the blended state.  The turn is either the
 * caller's (GIVEN: the call's start phase phi carries the carrier across buffers, cstack_plan of the bindings) or measured (LOCK: the
 * inner product of Z and the state), which survives a dropped buffer or a carrier phase step (a retune that moves kappa by whole
 * turns per frame also changes the phase ramp along each frame: tempest_hip_ctrack.h).  The entry points below go beyond the reference
 * and change nothing that exists.
 *
 *  1. INPUT.  As tempest_hip_cfold.h, 1.: iq, n, the format rule, the geometry y_t x x_t with P = y_t*x_t, t0, T, F = n_frames, the
 *     converted samples z[k] as complex f32 pairs, amax = max_k |z[k]|, kappa in turns per frame.  phi: the call's start phase in
 *     turns, double.  mode: TSDR_CSTACK_GIVEN or TSDR_CSTACK_LOCK.  zstate: P interleaved (re, im) f32 pairs, pixel (l, p) at
 *     pair index p*y_t + l, the layout of every other state; S(m) denotes its content on entry.  With alpha == 0 the state is NOT READ.
 *     mag (P floats, same order) and info (TSDR_CSTACK_INFO doubles) are outputs and may be NULL.  iq is never written.
 *  2. SAMPLING.  Exactly tempest_hip_cfold.h, 2.: u_f(m), the clamps, the taps and the blend z_f(m) of pixel m = l*x_t + p, frame f.
 *  3. WEIGHT.  x = fl64(f * kappa);  x' = fl64(x + phi);  r_f = x' - floor(x');  w_f = (f32(cospi(2 r_f)), f32(-sinpi(2 r_f))): sine and
 *     cosine evaluated in f64 and rounded once.  Only frac(phi) matters: phi and phi + integer agree within the bound, not in bits.
 *     With phi == 0 the weights, and therefore Z, have the bits of tsdr_cfold_iq_d: both files build w_f, the blend and the sum from
 *     one header (csrc/coherent_ops.h).
 *  4. RESULT.
 *       Z(m)  = (1/F) * sum_f w_f * z_f(m)    exactly tempest_hip_cfold.h, 4., up to the two fdiv by f32(F); no magnitude is taken
 *       rho   = sum_m Z(m) * conj(S(m))       f64: Re += zr*sr + zi*si, Im += zi*sr - zr*si, the products in f64 of the f32 values
 *       E_z   = sum_m |Z(m)|^2,  E_s = sum_m |S(m)|^2                  likewise.  With alpha == 0: S = 0, so rho = E_s = 0
 *       q     = GIVEN: (1, 0).  LOCK (5.): rho / |rho| rounded to f32
 *       Zq(m) = conj(q) * Z(m):  re = fadd(fmul(qr, zr), fmul(qi, zi)),  im = fsub(fmul(qr, zi), fmul(qi, zr))
 *               (GIVEN: the four products are not executed, Zq = Z in bits)
 *       S'(m) = alpha == 0 ? Zq : fadd(fmul(alpha, S), fmul(fsub(1, alpha), Zq))     per component
 *       zstate <- S';   mag[p*y_t + l] <- |S'| as f32, by the operation the coherent fold's pixel uses, if mag != NULL
 *     The sums run per lane in pixel order, then over the 64 lanes by a fixed shuffle tree, then in wave order, then over the tiles:
 *     lane j of one wavefront adds tiles j, j + 64, ... in that order and the same tree combines the lanes.  No float atomics.
 *     With GIVEN, phi == 0 and alpha == 0, mag has the bits of tsdr_cfold_iq_d's state at alpha == 0.
 *  5. LOCK.  If |rho| = hypot(Re rho, Im rho) is finite and > 0: q = (f32(Re rho / |rho|), f32(Im rho / |rho|)), the divisions in f64;
 *     otherwise q = (1, 0) (the first buffer, alpha == 0; an empty or a non-finite state).  Z is turned ONTO the state: the state's
 *     phase is the first buffer's and stays.  phi then only moves Z and rho together: S' does not depend on it beyond the bound.
 *     GIVEN is open loop: it is exact while the caller's phi follows the carrier, and a phase step (a dropped buffer, a retune) turns
 *     Z against the state until the state has forgotten; LOCK follows the step within the call that sees it.
 *  6. INFO.  info[0..3] = Re rho, Im rho, E_z, E_s;  info[4] = theta = atan2(Im rho, Re rho) / (2 pi) in turns, 0 when rho == 0;
 *     info[5] = gamma = |rho| / sqrt(E_z * E_s), 0 unless that product is > 0;  info[6..7] = q widened.  Written in GIVEN mode too: a
 *     caller that carries the phase itself reads the residual theta and the coherence gamma and runs its own loop
 *     (cstack_plan(..., theta) of the bindings).  A device pointer in the `_d` form.
 *  7. ACCURACY.  The contract is an error bound, not a bit pattern; the result does not depend on tsdr_set_precision.  u = 2^-24,
 *     eps_z = sqrt(2) * (F + 12) * u * amax of tempest_hip_cfold.h, 5. (the phase adds nothing: x' is one more f64 rounding, 2^-53 turns),
 *     M = max(amax, max_m |S(m)|).  ref: the formulas of 2. - 6. in exact arithmetic on the same z, S and f32(alpha).
 *       GIVEN  the blend rounds four times per component (fsub, two fmul, fadd), each <= u*M:
 *              |S' - ref| <= sqrt(2) * (F + 16) * u * M = eps_s            |mag - |ref|| <= sqrt(2) * (F + 18) * u * M  (the root: 2u)
 *       sums   Z enters with its error, S exactly; the f64 sums are less than 2^16 additions deep for every accepted geometry:
 *              |rho - ref| <= eps_z * sqrt(P * E_s) + 2^-36 * sqrt(E_z * E_s) = eps_rho      (Cauchy-Schwarz, as 8. there)
 *              |E_z - ref| <= 2 * eps_z * sqrt(P * ref) + P * eps_z^2 + 2^-36 * ref,   |E_s - ref| <= 2^-36 * ref
 *              |theta - ref| <= eps_rho / (4 * |rho_ref|) + 2^-40 turns (mod 1), for eps_rho <= |rho_ref|: the angle of two vectors
 *              that far apart is at most asin(eps_rho / |rho_ref|) <= (pi/2) * eps_rho / |rho_ref| radians
 *       LOCK   q carries that angle and its own rounding (<= u), the rotation two products and a sum per component (<= 2u*|Z| each),
 *              together <= 4u*amax beside the angle term:
 *              |S' - ref| <= sqrt(2) * (F + 19) * u * M + (pi/2) * amax * eps_rho / |rho_ref| = eps_lock
 *              |mag - |ref|| <= sqrt(2) * (F + 21) * u * M + (pi/2) * amax * eps_rho / |rho_ref|
 *              The angle term grows as gamma falls: the bound is a function of |rho_ref|, not a constant.  With rho_ref == 0
 *              (alpha == 0) the angle term is absent.  gamma and q follow from rho, E_z, E_s within those bounds.
 *  8. REPRODUCIBILITY.  Two calls with the same arguments and the same state on entry leave identical bits in zstate, mag and info:
 *     no floating-point atomics, every sum in the fixed order of 4.
 *  9. FORMAT INVARIANCE.  Integer formats give the bits of the host-expanded ComplexF32 buffer, in all three outputs.
 * 10. REFUSALS.  TSDR_EINVAL, with nothing written and nothing enqueued, for everything tempest_hip_cfold.h, 9. refuses of a fold (a NULL
 *     ctx or iq; an unknown format; y_t <= 0, x_t <= 0, P >= 2^31; n < 2 or n >= 2^31; F < 0; T or t0 not finite; T < 2; t0 < 0; kappa
 *     not finite; t0 + F*T > n; alpha outside [0, 1] or NaN; iq not aligned), and for: phi not finite; mode outside {0, 1};
 *     zstate NULL; in the device form zstate not 8-byte aligned, mag not 4-byte aligned, info not 8-byte aligned.  mag and info may be NULL.
 *     The host forms have no alignment rule.  F == 0 (with everything else valid) is TSDR_OK and touches nothing, info included.
 *     Nothing is written outside zstate[0 .. 2P), mag[0 .. P), info[0 .. 8).  Overlapping outputs are undefined.
 * 11. COST.  The fold kernel is the coherent fold's (the same staged / direct choice at TSDR_CFOLD_STAGE_MAX, the same tiles and LDS
 *     plus 256 bytes of partial sums) with another epilogue: it keeps Z complex, reads S when alpha != 0 and writes four f64
 *     partial sums per tile to the context's workspace; a wavefront stores 64 consecutive lines of a column, 512-byte segments.
 *       GIVEN  "cstack_tile" / "cstack_direct" blends and stores zstate and mag itself: one launch does the whole update,
 *              8n + 16P .. 20P bytes at ComplexF32 with alpha != 0.  "cstack_lock" (one wavefront) follows only when info != NULL.
 *       LOCK   the fold stores Z to the workspace (8P), "cstack_lock" adds the partial sums and leaves q, "cstack_blend" streams Z and S,
 *              turns, blends and stores (two pixels per lane, 16-byte accesses, when zstate is 16-byte aligned): 28P bytes and two
 *              launch gaps more.
 *     tsdr_profile_get names the kernels.  Measured on one MI355X (profiles/cstack.json; 30 frames, ComplexF32, alpha 0.1, beside
 *     tsdr_cfold_iq_d in the same process): C2 (2576x1125) GIVEN 134.4 us, LOCK 148.0 us beside the coherent fold's 130.1 us (1.03x,
 *     1.14x); C5 (4400x2250) 336.0 and 381.6 beside 300.5 us (1.12x, 1.27x).  Kernels and registers: DESIGN.md section 4.
 * The `_d` form takes device pointers, enqueues on the context's stream and returns.  The host-pointer form uploads iq (and zstate
 * when alpha != 0), runs the device form and copies zstate (and mag and info when given) back; its wait is bounded like every other
 * host form's (option "wait_ms").
 */
#ifndef TEMPEST_HIP_CSTACK_H
#define TEMPEST_HIP_CSTACK_H
#ifndef TEMPEST_HIP_CFOLD_H
#error "include tempest_hip.h, which includes tempest_hip_cstack.h after tempest_hip_cfold.h"
#endif
#define TSDR_CSTACK_GIVEN 0
#define TSDR_CSTACK_LOCK 1
#define TSDR_CSTACK_INFO 8
/* n_frames frames of period T from t0, frame f turned by -(phi + f*kappa) turns, summed as complex samples -> Z; Z turned by conj(q)
 * (mode) and blended into the complex (y_t, x_t) state; |state| -> mag, the sums -> info (1. - 9. above), device pointers */
int tsdr_cstack_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, double phi,
                     int n_frames, int y_t, int x_t, float alpha, int mode, float *zstate, float *mag, double *info);
/* the same with host pointers: upload, run, download zstate, mag, info */
int tsdr_cstack_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, double phi,
                   int n_frames, int y_t, int x_t, float alpha, int mode, float *zstate, float *mag, double *info);
#endif /* TEMPEST_HIP_CSTACK_H */
