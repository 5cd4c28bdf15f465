// raster_shift.h -- what raster_accum.hip and raster_register.hip share: the shift rule of include/tempest_hip_hires.h (SHIFT
// UNITS) as one device function, and the internal entry points through which the two files call each other.
#pragma once
#include "common.h"

namespace tsdr {

#ifdef __HIPCC__
// floored modulus of a 64-bit value by a positive int
__device__ inline int mod_floor(long long v, int m) {
  const long long r = v % (long long)m;
  return (int)(r < 0 ? r + m : r);
}

// one frame's shift in raster lines / pixels, 0 <= r < size (tempest_hip_hires.h, SHIFT UNITS).  |2*a*size + img| < 2^63 for
// every int a and every size, img < 2^31.
__device__ inline int resolve_shift(int a, int size, int units, int img) {
  if (units == TSDR_SHIFT_RASTER) return mod_floor((long long)a, size);
  const long long num = 2ll * (long long)a * (long long)size + (long long)img, den = 2ll * (long long)img;
  long long q = num / den;
  if (num % den < 0) --q;   // floored division
  return mod_floor(q, size);
}
#endif

// raster_accum.hip: what tsdr_raster_accum_d refuses about the rasters, the geometry and the shifts (tempest_hip_hires.h, EDGE
// CASES) -- everything but its state -- before anything is enqueued or staged
int raster_args_check(tsdr_ctx *ctx, const char *fn, const float *rasters, int n_frames, int y_t, int x_t, const int *shifts, int shift_units,
                      int img_h, int img_w);

// raster_register.hip (include/tempest_hip_register.h), checked arguments, device pointers, n_frames > 0:
// the registration of n_frames rasters against ref (or frame 0): shifts_out = 2*n_frames ints in TSDR_SHIFT_RASTER units
int register_launch(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const float *ref, const int *shifts, int shift_units,
                    int img_h, int img_w, int d_y, int d_x, int *shifts_out, double *scores);
// shifts_out = the coarse shifts alone (what k_raster_accum resolves from the same arguments), for tsdr_frames_hires_shifts
int resolve_launch(tsdr_ctx *ctx, int n_frames, int y_t, int x_t, const int *shifts, int shift_units, int img_h, int img_w, int *shifts_out);

}  // namespace tsdr
