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
// w * z alone, the term coh_add sums: two products and one sum per component, each rounded
__device__ inline float2 coh_mul(float2 z, float2 w) {
  return make_float2(__fsub_rn(__fmul_rn(w.x, z.x), __fmul_rn(w.y, z.y)), __fadd_rn(__fmul_rn(w.x, z.y), __fmul_rn(w.y, z.x)));
}
// the weight of frame f on raster line l of y_t along a track (include/tempest_hip_ctrack.h, TRACK): a, b in turns,
// c_l = fl64((l + 1/2) / y_t), x = fma(b, c_l, a); b == 0 leaves x = a exactly
__device__ inline float2 coh_line_weight(double a, double b, int l, int y_t) {
  const double c = ((double)l + 0.5) / (double)y_t;
  return coh_weight(fma(b, c, a));
}
// Z = acc / F: one fdiv per component
__device__ inline float2 coh_mean(float2 a, float Ff) { return make_float2(__fdiv_rn(a.x, Ff), __fdiv_rn(a.y, Ff)); }

}  // namespace tsdr
