/*
 * tempest_hip_hires.h -- frame averaging at the monitor's own resolution: the aligned one-pole IIR of GUI.jl:171-175 on the
 * y_t x x_t raster instead of the 600x800 rendering image.  Part of the C ABI of libtempest_hip.so: tempest_hip.h includes this
 * file once; include tempest_hip.h, not this file.
 *
 * The reference aligns and averages at 600x800 only (downgradeImage, Resampler.jl:124-126); full resolution exists there, and in
 * tsdr_frames_* (raster_out), as one noisy, unregistered raster per frame.  The entry points below go beyond the reference, as the
 * option "vsync_current_sy" does: they change nothing that exists.
 *
 *  1. SEMANTICS.  Rasters R_f, f = 0 .. n_frames-1: each column-major (y_t, x_t) as tsdr_sig_to_image writes it, dense, P = y_t*x_t
 *     floats apart.  A state A of the same shape, in and out.  For every frame in order, for every pixel (i, j):
 *         A[i,j] <- fadd(fmul(alpha, A[i,j]), fmul(fsub(1, alpha), R_f[(i + r_y) mod y_t, (j + r_x) mod x_t]))
 *     -- GUI.jl:172,175 at raster size: three separately rounded f32 operations (1 - alpha once per call, two products, one sum),
 *     NO FMA, the rounding sequence of the 600x800 shift + IIR and of the CPU oracle.  NaN / Inf propagate.
 *     shifts: NULL (r = 0 for every frame), or 2*n_frames ints on the device in sync_idx order ([2f] = s_y, [2f+1] = s_x of
 *     frame f): (a, b) below.  Any int is accepted; every modulus and division is FLOORED, so negatives wrap as circshift does.
 *  2. SHIFT UNITS.
 *     TSDR_SHIFT_RASTER: r_y = a mod y_t, r_x = b mod x_t (raster lines / pixels).  img_h, img_w are ignored.
 *     TSDR_SHIFT_IMAGE:  (a, b) are indices of an img_h x img_w sync grid (the frame loop's is 600x800):
 *         r_y = floor((2*a*y_t + img_h) / (2*img_h)) mod y_t,   r_x = floor((2*b*x_t + img_w) / (2*img_w)) mod x_t
 *     in 64-bit integers.  circshift(image, -s_y) brings image row s_y + 1 to the top; that row starts at raster offset
 *     s_y * y_t / img_h, rounded half up.  The full-size picture is then registered exactly as the 600x800 one is -- the stale-s_y
 *     ordering and the polarity options included -- because it consumes the loop's own sync_idx.
 *  3. EDGE CASES.  n_frames == 0 is TSDR_OK and touches nothing.  TSDR_EINVAL, with nothing written and nothing enqueued, for:
 *     y_t <= 0, x_t <= 0, n_frames < 0, P >= 2^31; a NULL ctx or state, NULL rasters with n_frames > 0; an unknown shift_units;
 *     img_h <= 0 or img_w <= 0 under TSDR_SHIFT_IMAGE; rasters, shifts or state not aligned to 4 bytes.  Beyond 4 bytes nothing
 *     is asked of a pointer: base + 4k of a larger buffer gives the bits of a fresh allocation.  The rasters and the shifts are
 *     never written; nothing is written outside state[0 .. P).
 *  4. COST.  One launch per call; every output pixel belongs to one lane; the state is read once and written once and the
 *     n_frames raster reads are the stream: n_frames*4P + 8P bytes.
 *  5. THE WHOLE LOOP.  tsdr_frames_hires_iq_d is tsdr_frames_iq_d plus that recurrence on the buffer's rasters.  It orders itself
 *     behind pending tsdr_frames_submit_* buffers as tsdr_frames_d does, then walks the buffer in chunks of k frames: per chunk
 *     one tsdr_frames_iq_d on iq + f0*S samples with the rasters going to context workspace (sync_idx to the caller's array, or
 *     to workspace when that is NULL), then one raster_accum launch with TSDR_SHIFT_IMAGE, 600, 800 over the chunk's rasters
 *     and indices (do_align == 0: no shifts).  imageOut_state, frames_out, sync_idx and *n_frames are what tsdr_frames_iq_d
 *     leaves; hires_state (y_t x x_t, in / out) is the full-size average.
 *     Option "hires_chunk_frames" (tsdr_set_option): k > 0 means exactly k frames per chunk and bounds the raster workspace at
 *     k*4P bytes; 0, the default, is the whole buffer in one chunk (workspace: n_frames*4P bytes -- 348 MB for 30 frames of
 *     2576x1125, 1.2 GB for 30 frames of 4400x2250).  One chunk is the default because it measured fastest: chunks held at or
 *     under 192 MiB, meant to be re-read from the Infinity Cache, lost 4 % at the first geometry and 34 % at the second.
 *     In TSDR_EXACT every output is bit-identical to the unchunked loop and to the oracle's rasters and indices run through the
 *     recurrence above.  In TSDR_FAST the sync guard's adaptive route decides per call, so chunking may move frames between the
 *     exact and the fast route: what is promised there is the tolerance of the FAST rasters (indices identical, hires_state
 *     within the raster bar plus the recurrence's own roundings), NOT bit identity with the unchunked loop.
 * The host-pointer form tsdr_raster_accum (what the Julia shim binds) uploads rasters, shifts and state, runs the device form and
 * copies the state back; its wait is bounded like every other host form's (option "wait_ms").  The `_d` forms enqueue on the
 * context's stream and return.
 */
#ifndef TEMPEST_HIP_HIRES_H
#define TEMPEST_HIP_HIRES_H
#ifndef TEMPEST_HIP_H
#error "include tempest_hip.h, which includes tempest_hip_hires.h"
#endif
enum { TSDR_SHIFT_RASTER = 0, TSDR_SHIFT_IMAGE = 1 };
/* the aligned IIR over n_frames rasters, device pointers */
int tsdr_raster_accum_d(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const int *shifts, int shift_units,
                        int img_h, int img_w, float alpha, float *state);
/* the same with host pointers: upload, run, download state */
int tsdr_raster_accum(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const int *shifts, int shift_units,
                      int img_h, int img_w, float alpha, float *state);
/* tsdr_frames_iq_d + the full-size average of the same frames (5. above); device pointers, sync_idx may be NULL */
int tsdr_frames_hires_iq_d(tsdr_ctx *ctx, tsdr_sync *sync, const void *iq, int iq_fmt, float scale, size_t nEch, size_t S, int y_t,
                           int x_t, float alpha, int do_align, float *imageOut_state, float *frames_out, float alpha_hires,
                           float *hires_state, int *sync_idx, int *n_frames);
#endif /* TEMPEST_HIP_HIRES_H */
