/*
 * tempest_hip_display.h -- display export: ROI crop, range stretch and 8-bit output of the library's f32 pictures, on the GPU.  Part
 * of the C ABI of libtempest_hip.so: tempest_hip.h includes this file once, after tempest_hip_register.h; include tempest_hip.h,
 * not this file.
 *
 * Every picture the library produces (frames_out, imageOut_state, hires_state, raster_out) is f32 amplitude in arbitrary units.
 * The reference normalises a picture before showing it -- fullScale! (ScreenRenderer.jl:35-39) is (mat .- min) / (max - min) -- on
 * the host.  The entry points below do that on the device and return bytes: a quarter of the download, and the statistics taken
 * over a region of interest instead of over the blanking band.  They go beyond the reference (whose fullScale! they restate as
 * one of three range modes) and change nothing that exists.
 *
 *  1. INPUT.  images: n_images pictures, each column-major (h, w) f32, dense, h*w floats apart -- what frames_out,
 *     imageOut_state, hires_state and raster_out are.  The inputs are never written.
 *  2. ROI.  Rows i0 .. i0+rh-1 and columns j0 .. j0+rw-1 of every picture, NO WRAP (the aligned picture's active area is
 *     contiguous: the blanking band is centred on index 0).  R = rh*rw.
 *  3. OUTPUT.  out: n_images column-major (rh, rw) byte pictures, dense, R bytes apart, at ANY byte alignment; NULL when only
 *     the ranges are wanted.  ranges_out: NULL, or 2*n_images floats, the (lo, hi) each picture was mapped with; the sign of a
 *     zero in it is unspecified.  Nothing is written outside out[0 .. n_images*R) and ranges_out[0 .. 2*n_images).
 *  4. GROUP.  A group is one picture; with TSDR_DISPLAY_SHARED it is all pictures of the call (a buffer's frames then do not
 *     flicker against each other).  Every picture of a group is mapped with, and reports, the group's range.
 *  5. RANGE of a group.  Every operation below is IEEE f32, individually rounded: fsub, fadd, fmul, fdiv are the correctly
 *     rounded operations, NO FMA, no fast division.  N = the number of FINITE ROI pixels of the group; mn, mx = their minimum and
 *     maximum by value; N == 0: mn = mx = 0.
 *       TSDR_RANGE_FIXED       (lo, hi) are the arguments.
 *       TSDR_RANGE_MINMAX      (lo, hi) = (mn, mx).  With no flags this is fullScale! times 255, rounded.
 *       TSDR_RANGE_PERCENTILE  B = TSDR_DISPLAY_BINS = 4096, d = fsub(mx, mn), invw = fdiv((float)B, d), wd = fdiv(d, (float)B).
 *         If !(d > 0), or d or invw is not finite: (lo, hi) = (mn, mx).  Otherwise every finite ROI pixel v falls into
 *         bin(v) = min(B-1, (int)floorf(fmul(fsub(v, mn), invw))); the counts are exact unsigned integers, cum(b) the inclusive
 *         prefix count.  k_lo = floor(p_lo*(N-1)), k_hi = ceil(p_hi*(N-1)), computed in f64.
 *         b_lo = the smallest b with cum(b) > k_lo, b_hi = the smallest b with cum(b) > k_hi.
 *         edge(b) = b == B ? mx : fadd(mn, fmul((float)b, wd)).  lo = edge(b_lo), hi = edge(b_hi + 1).
 *         Consequently p = (0, 1) gives exactly (mn, mx).
 *  6. MAPPING of a pixel v.  dd = fsub(hi, lo), s = fdiv(255.0f, dd), once per group.  If !(dd > 0), or dd or s is not finite,
 *     EVERY byte of the group is 0 (the reference would give NaN there), TSDR_DISPLAY_INVERT or not.  Otherwise
 *     q = fmul(fsub(v, lo), s); a NaN becomes 0; clamp to [0, 255]; round half to even (rintf); the byte is q, or 255 - q with
 *     TSDR_DISPLAY_INVERT.  A NaN pixel is 0 either way.  +-Inf pixels clamp; they never enter mn, mx, N or the histogram.
 *  7. REFUSALS.  n_images == 0 is TSDR_OK and touches nothing.  TSDR_EINVAL, with nothing written and nothing enqueued, for: a
 *     NULL ctx; NULL images with n_images > 0; both out and ranges_out NULL; h, w, rh or rw <= 0; i0 < 0, j0 < 0, i0+rh > h or
 *     j0+rw > w; h*w >= 2^31; n_images < 0; an unknown range_mode or unknown flag bits; PERCENTILE with a NaN fraction or not
 *     0 <= p_lo <= p_hi <= 1; FIXED with a NaN bound; images or ranges_out not 4-byte aligned.
 *  8. REPEATABILITY.  Two calls on the same input give the same bytes: minimum, maximum and the counters are integers combined
 *     with integer atomics (order-independent); there are no floating-point atomics.
 *  9. STATE.  Scratch -- per group mn, mx, the range and the B counters, whose total is N -- lives in the context's workspace
 *     and is cleared ON THE STREAM BY EVERY CALL: a call never sees what an earlier one left.
 * 10. COST per picture (bytes of device memory traffic; one launch per pass, plus one small launch that picks the range):
 *       FIXED       reads 4*R, writes R        (the mapping pass alone)
 *       MINMAX      reads 8*R, writes R        (statistics pass + mapping pass)
 *       PERCENTILE  reads 12*R, writes R       (statistics pass + histogram pass + mapping pass)
 *     A 16-byte load path is taken where a picture's columns allow it (h a multiple of 4, images 16-byte aligned; in the mapping
 *     pass additionally the output's four-row groups falling on the input's), dword loads otherwise; the mapping pass stores one
 *     dword per four rows where the OUTPUT address allows and single bytes at a column's head and tail.
 * The `_d` form takes device pointers, enqueues on the context's stream and returns.  The host-pointer form tsdr_display_u8
 * uploads images, runs the device form and copies out and ranges_out back; its wait is bounded like every other host form's
 * (option "wait_ms").
 */
#ifndef TEMPEST_HIP_DISPLAY_H
#define TEMPEST_HIP_DISPLAY_H
#ifndef TEMPEST_HIP_REGISTER_H
#error "include tempest_hip.h, which includes tempest_hip_display.h after tempest_hip_register.h"
#endif
enum { TSDR_RANGE_FIXED = 0, TSDR_RANGE_MINMAX = 1, TSDR_RANGE_PERCENTILE = 2 };
enum { TSDR_DISPLAY_INVERT = 1, TSDR_DISPLAY_SHARED = 2 }; /* flags, or-ed */
#define TSDR_DISPLAY_BINS 4096
/* n_images (h, w) f32 pictures -> their (rh, rw) ROI as bytes (1. - 10. above), device pointers */
int tsdr_display_u8_d(tsdr_ctx *ctx, const float *images, int n_images, int h, int w, int i0, int j0, int rh, int rw, int range_mode,
                      float lo, float hi, double p_lo, double p_hi, int flags, uint8_t *out, float *ranges_out);
/* the same with host pointers: upload, run, download out and ranges_out */
int tsdr_display_u8(tsdr_ctx *ctx, const float *images, int n_images, int h, int w, int i0, int j0, int rh, int rw, int range_mode,
                    float lo, float hi, double p_lo, double p_hi, int flags, uint8_t *out, float *ranges_out);
#endif /* TEMPEST_HIP_DISPLAY_H */
