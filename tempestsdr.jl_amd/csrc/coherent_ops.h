// coherent_ops.h -- the device arithmetic the two coherent flavours of fold_engine.h share: raster_cfold.hip (the phase-coherent fold,
// include/tempest_hip_cfold.h) and raster_cstack.hip (the complex state across buffers, include/tempest_hip_cstack.h) build the
// weight of a frame, the interpolated sample, its accumulation and the mean Z from these functions, so a call of the second with
// phi == 0 leaves the first one's bits by construction.
#pragma once
#include "common.h"
#include "down_fused.h"

namespace tsdr {

// the weight of a frame whose turn is x (f * kappa, or f * kappa + phi), in turns: r = x - floor(x), (f32(cospi(2r)), f32(-sinpi(2r)))
__device__ inline float2 coh_weight(double x) {
  const double r = x - floor(x);
  double s, c;
  sincospi(2.0 * r, &s, &c);
  return make_float2((float)c, (float)(-s));
}
__device__ inline float2 coh_blend(float2 a, float2 b, double d) { return make_float2(fast_blend(a.x, b.x, d), fast_blend(a.y, b.y, d)); }
__device__ inline void coh_add(float2 &a, float2 z, float2 w) {
  a.x = __fadd_rn(a.x, __fsub_rn(__fmul_rn(w.x, z.x), __fmul_rn(w.y, z.y)));
  a.y = __fadd_rn(a.y, __fadd_rn(__fmul_rn(w.x, z.y), __fmul_rn(w.y, z.x)));
}
// Z = acc / F: one fdiv per component
__device__ inline float2 coh_mean(float2 a, float Ff) { return make_float2(__fdiv_rn(a.x, Ff), __fdiv_rn(a.y, Ff)); }

}  // namespace tsdr
