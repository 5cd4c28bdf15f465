/*
 * tempest_hip_register.h -- registration of full-size rasters to the raster pixel, for the average of tempest_hip_hires.h.  Part of
 * the C ABI of libtempest_hip.so: tempest_hip.h includes this file once, after tempest_hip_hires.h; include tempest_hip.h, not this
 * file.
 *
 * tsdr_frames_hires_iq_d registers every raster with the frame loop's sync indices, which live on the 600x800 grid: one grid step is
 * x_t/800 raster pixels (3.2 at 2576x1125, 5.5 at 4400x2250), so a frame lands up to half a cell from where it belongs.  The entry
 * points below refine such a coarse shift by an integer number of raster lines / pixels, by correlating the frame's column and row
 * sums with those of a reference picture.  Like the rest of the full-size average they go beyond the reference implementation and
 * change nothing that exists.
 *
 *  1. PROFILES.  Rasters R_f, f = 0 .. n_frames-1: column-major (y_t, x_t), dense, P = y_t*x_t floats apart.
 *         col_f[j] = sum_i R_f[i,j]  (x_t values per frame),     row_f[i] = sum_j R_f[i,j]  (y_t values per frame)
 *     Every f32 value is converted to f64 exactly and accumulated in f64, starting from +0.  The summation order is the
 *     implementation's, but it is FIXED: per-tile partial sums added in tile order, no floating-point atomics, so two calls on the
 *     same input give the same bits.  Any order is within n_terms * 2^-53 * sum|x| of the exact sum; sums of integers below 2^53
 *     are exact.  tsdr_raster_profiles_d writes col (n_frames*x_t doubles) and row (n_frames*y_t doubles); either may be NULL.
 *  2. COARSE SHIFT.  (r0_y, r0_x) of frame f is exactly what tsdr_raster_accum_d resolves from shifts, shift_units, img_h, img_w
 *     (tempest_hip_hires.h, SHIFT UNITS); shifts == NULL means 0.
 *  3. REFERENCE PROFILES.  cref (x_t values) and rref (y_t values) are the profiles of ref, a (y_t, x_t) f32 raster.  Per axis:
 *     if ref == NULL, or that axis's reference profile is FLAT, the reference on that axis is frame 0's profile rotated by frame
 *     0's coarse shift, cref[j] = col_0[(j + r0_x(0)) mod x_t].  A profile is flat when every element compares IEEE-equal to
 *     element 0 (a profile holding a NaN is not flat).  A fresh all-zero state therefore registers a call's frames to the first
 *     of them, and frame 0 gets d = 0.  The decision is made on the device, with no host round trip.
 *  4. SCORES.  For d = -D_x .. D_x:
 *         s_x(f,d) = sum_{j=0}^{x_t-1} cref[j] * col_f[(j + r0_x + d) mod x_t]
 *     in f64, product then sum, NO FMA; the order over j is the implementation's and FIXED.  s_y likewise with rref, row_f, r0_y,
 *     D_y.  The sign is the accumulator's, which reads R_f[(i + r_y) mod y_t, (j + r_x) mod x_t].
 *  5. CHOICE.  Candidates are visited in the order 0, -1, +1, -2, +2, ..., -D, +D; the running best starts at d = 0 and is replaced
 *     only on a strict >.  A NaN score never wins; among ties the smallest |d| wins, the negative candidate ahead of the positive.
 *  6. OUTPUT.  shifts_out[2f] = (r0_y + d*_y) mod y_t, shifts_out[2f+1] = (r0_x + d*_x) mod x_t: TSDR_SHIFT_RASTER units in
 *     [0, size), ready for tsdr_raster_accum_d.  scores (NULL, or n_frames*((2*d_y+1) + (2*d_x+1)) doubles): per frame the y block,
 *     then the x block; within a block the score of d at index d + D.
 *  7. INDEPENDENCE.  Every frame of a call is scored against the same reference: no dependence between the frames of a call, no
 *     recurrence.
 *  8. REFUSALS.  TSDR_EINVAL, with nothing written and nothing enqueued, for: everything tsdr_raster_accum_d refuses about its
 *     rasters, geometry and shifts; d_y < 0 or d_x < 0; 2*d_y + 1 > y_t or 2*d_x + 1 > x_t (the candidates must be distinct);
 *     shifts_out == NULL with n_frames > 0; a pointer not aligned to its element size (4 bytes for float / int, 8 for double).
 *     n_frames == 0 is TSDR_OK and touches nothing.  The inputs are never written.
 *  9. COST.  One bandwidth-bound pass over the rasters (n_frames*4P bytes read, plus 4P for ref) that writes per-tile partial
 *     sums, one small launch that adds them in tile order, and one small launch of one workgroup per (frame, axis) that scores
 *     and picks: (2D+1)*size multiply-adds per frame and axis.
 * 10. THE LOOP.  Option "hires_refine" (tsdr_set_option; an integer k, 0 .. 8, default 0, no environment preset).  k == 0:
 *     tsdr_frames_hires_iq_d is as tempest_hip_hires.h describes it.  k > 0 and do_align != 0: each chunk runs the frame-loop
 *     call, then the registration with ref = hires_state as the chunk finds it, the chunk's sync_idx in TSDR_SHIFT_IMAGE units on
 *     600x800, D_y = min(ceil(k*y_t/600), (y_t-1)/2), D_x = min(ceil(k*x_t/800), (x_t-1)/2), then the accumulator with the
 *     refined shifts in TSDR_SHIFT_RASTER units.  sync_idx, frames_out and imageOut_state stay exactly what tsdr_frames_iq_d
 *     leaves; only hires_state differs.  do_align == 0: the option has no effect.
 *     tsdr_frames_hires_shifts synchronises (as tsdr_sync_guard_margins does) and returns the raster-unit shifts the most recent
 *     tsdr_frames_hires_iq_d on this context actually applied, refined or not: *n_frames = their number (0 when that call ran
 *     with do_align == 0), min(*n_frames, max_frames) pairs written.
 * The host-pointer form tsdr_raster_register uploads rasters, ref and shifts, runs the device form and copies shifts_out and scores
 * back; its wait is bounded like every other host form's (option "wait_ms").  The `_d` forms enqueue on the context's stream and
 * return.
 */
#ifndef TEMPEST_HIP_REGISTER_H
#define TEMPEST_HIP_REGISTER_H
#ifndef TEMPEST_HIP_HIRES_H
#error "include tempest_hip.h, which includes tempest_hip_register.h after tempest_hip_hires.h"
#endif
/* column and row sums of n_frames rasters in f64, device pointers; col or row may be NULL */
int tsdr_raster_profiles_d(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, double *col, double *row);
/* the registration of n_frames rasters against ref (1. - 8. above), device pointers */
int tsdr_raster_register_d(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const float *ref, const int *shifts,
                           int shift_units, int img_h, int img_w, int d_y, int d_x, int *shifts_out, double *scores);
/* the same with host pointers: upload, run, download shifts_out and scores */
int tsdr_raster_register(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const float *ref, const int *shifts,
                         int shift_units, int img_h, int img_w, int d_y, int d_x, int *shifts_out, double *scores);
/* the shifts (2 per frame, raster units, host memory) the most recent tsdr_frames_hires_iq_d applied (10. above) */
int tsdr_frames_hires_shifts(tsdr_ctx *ctx, int max_frames, int *shifts, int *n_frames);
#endif /* TEMPEST_HIP_REGISTER_H */
