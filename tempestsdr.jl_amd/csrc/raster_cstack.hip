// raster_cstack.hip -- coherent stacking across buffers (include/tempest_hip_cstack.h): the phase-coherent fold of raster_cfold.hip
// with a start phase phi, whose picture Z stays COMPLEX, is turned onto a complex state by conj(q) and blended into it; q is (1, 0)
// (GIVEN) or the direction of rho = sum Z conj(S) (LOCK).  |state| is taken once, of the blended state.
//
// The fold is fold_engine.h's kernel with a flavour that `stacks`: the frame loop, the staging and the tiles are the coherent fold's,
// the device arithmetic up to Z is coherent_ops.h's (shared with raster_cfold.hip), and the epilogue is the scan's reduction with
// one trial and four f64 sums (Re rho, Im rho, E_z, E_s) per tile.  Three launches at most:
//   cstack_tile / cstack_direct   per pixel Z = acc / F, S (read only when alpha != 0), the pixel's share of the four sums.
//                                 GIVEN: blends and stores zstate and mag -- the whole update.  LOCK: stores Z to the workspace.
//   cstack_lock                   one wavefront: lane j adds the partial sums of tiles j, j + 64, ... in that order, the fixed shuffle tree
//                                 adds the lanes; lane 0 forms |rho|, theta, gamma and q in f64, writes info (if asked) and q.
//                                 GIVEN: only when info != NULL.
//   cstack_blend                  LOCK only: streams Z and S, turns Z by conj(q), blends, stores zstate and mag; two pixels per lane
//                                 as 16-byte accesses when zstate is 16-byte aligned, with a one-pixel tail; else one pixel per lane.
// Workspace WS_CSTACK: [tiles][4] f64 partial sums, q (16 bytes), then (LOCK) P float2 of Z.
#include "coherent_ops.h"
#include "fold_engine.h"

namespace tsdr {
namespace {

constexpr int kBlendThreads = 256;
static_assert((TSDR_CFOLD_STAGE_MAX | 1) * kFoldLines * 8 + 4 * kFoldLines * 2 + 2 * 8 + 8 * 4 * kFoldTileWaves <= 65536,
              "staged span + first-sample table + weight + the four sums' partials (red) fit 64 KiB of LDS");

// the pixel's share of rho = sum Z conj(S), E_z, E_s: products in f64 of the f32 values (exact), one f64 addition each
__device__ inline void stack_sums(double *s, float2 Z, float2 S) {
  const double zr = (double)Z.x, zi = (double)Z.y, sr = (double)S.x, si = (double)S.y;
  s[0] += zr * sr + zi * si;
  s[1] += zi * sr - zr * si;
  s[2] += zr * zr + zi * zi;
  s[3] += sr * sr + si * si;
}
// conj(q) * Z
__device__ inline float2 stack_turn(float2 q, float2 Z) {
  return make_float2(__fadd_rn(__fmul_rn(q.x, Z.x), __fmul_rn(q.y, Z.y)), __fsub_rn(__fmul_rn(q.x, Z.y), __fmul_rn(q.y, Z.x)));
}
// S' = alpha == 0 ? Zq : alpha * S + (1 - alpha) * Zq, per component
__device__ inline float2 stack_mix(float alpha, float beta, float2 S, float2 Zq) {
  if (alpha == 0.f) return Zq;
  return make_float2(__fadd_rn(__fmul_rn(alpha, S.x), __fmul_rn(beta, Zq.x)), __fadd_rn(__fmul_rn(alpha, S.y), __fmul_rn(beta, Zq.y)));
}

struct Stacked {
  using Sample = float2;
  struct Trial {
    double T, kappa, phi;   // frame f is turned by -(phi + f * kappa) turns
    int mode;
    float *mag;             // GIVEN: |S'| (may be null)
    float2 *zws;            // LOCK: Z, in state order
  };
  static constexpr bool has_weights = true, stacks = true, line_weights = false;
  static constexpr int NS = 4, kMaxTrials = 1, kStageMax = TSDR_CFOLD_STAGE_MAX, kSlot = WS_CSTACK;
  static constexpr const char *name = "cstack";
  static int tile_p(bool) { return kFoldTileP; }
  static int batch(bool) { return 1; }

  __device__ static float2 stage(float2 z) { return z; }
  __device__ static double period(const Trial &t, unsigned) { return t.T; }
  __device__ static bool live(const Trial &, int) { return true; }
  // w_f of tempest_hip_cstack.h (WEIGHT): x = fl64(f * kappa), x' = fl64(x + phi)
  __device__ static float2 weight(const Trial &t, int f, int) {
    const double x = (double)f * t.kappa;
    return coh_weight(x + t.phi);
  }
  __device__ static float2 blend(float2 a, float2 b, double d) { return coh_blend(a, b, d); }
  __device__ static void add(float2 &a, float2 z, float2 w) { coh_add(a, z, w); }
  // Args: FoldArgs of a stacking flavour, whose Trial has mode, mag and zws (this one's, or raster_ctrack.hip's)
  template <class Args>
  __device__ static void stack(const Args &A, double *s, float2 acc, float Ff, size_t at) {
    const float2 Z = coh_mean(acc, Ff);
    float2 *zp = reinterpret_cast<float2 *>(A.state) + at;
    float2 S = make_float2(0.f, 0.f);
    if (A.alpha != 0.f) S = *zp;
    stack_sums(s, Z, S);
    if (A.tr.mode == TSDR_CSTACK_GIVEN) {
      const float2 o = stack_mix(A.alpha, __fsub_rn(1.f, A.alpha), S, Z);
      *zp = o;
      if (A.tr.mag) A.tr.mag[at] = abs_iq_rn(o.x, o.y);
    } else {
      A.tr.zws[at] = Z;
    }
  }

  static int refuse(tsdr_ctx *ctx, const char *fn, const FoldCall &c) {
    if (!std::isfinite(c.T) || !std::isfinite(c.t0)) return set_err(ctx, TSDR_EINVAL, "%s: the period and t0 must be finite", fn);
    if (!std::isfinite(c.kappa0) || !std::isfinite(c.phi)) return set_err(ctx, TSDR_EINVAL, "%s: kappa and phi must be finite", fn);
    if (c.T < 2.0 || c.t0 < 0.0)
      return set_err(ctx, TSDR_EINVAL, "%s: the period must be at least 2 and t0 not negative (got %g, %g)", fn, c.T, c.t0);
    if (c.mode != TSDR_CSTACK_GIVEN && c.mode != TSDR_CSTACK_LOCK)
      return set_err(ctx, TSDR_EINVAL, "%s: mode must be TSDR_CSTACK_GIVEN or TSDR_CSTACK_LOCK (got %d)", fn, c.mode);
    return TSDR_OK;
  }
  static Trial trial(const FoldCall &c) { return Trial{c.T, c.kappa0, c.phi, c.mode, c.mag, nullptr}; }
  static int launch(tsdr_ctx *ctx, const FoldCall &c, const FoldGeom &g, const FoldArgs<Trial> &A);
};

// the tiles' partial sums in a fixed order, then |rho|, theta, gamma, q (tempest_hip_cstack.h, 4. - 6.)
__global__ __launch_bounds__(64) void k_cstack_lock(const double *__restrict__ part, unsigned tiles, int mode, double *__restrict__ info,
                                                    float2 *__restrict__ q_out) {
  const int lane = threadIdx.x;
  const double2 *p2 = reinterpret_cast<const double2 *>(part);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (unsigned t = (unsigned)lane; t < tiles; t += 64u) {
    const double2 a = p2[2 * (size_t)t], b = p2[2 * (size_t)t + 1];
    s[0] += a.x;
    s[1] += a.y;
    s[2] += b.x;
    s[3] += b.y;
  }
  for (int off = 32; off > 0; off >>= 1) {   // the same tree on every run
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] += __shfl_down(s[i], off);
  }
  if (lane != 0) return;
  const double mag = hypot(s[0], s[1]);
  const bool usable = isfinite(mag) && mag > 0.0;
  float2 q = make_float2(1.f, 0.f);
  if (mode == TSDR_CSTACK_LOCK && usable) q = make_float2((float)(s[0] / mag), (float)(s[1] / mag));
  *q_out = q;
  if (info) {
    const double den = s[2] * s[3];
    info[0] = s[0];
    info[1] = s[1];
    info[2] = s[2];
    info[3] = s[3];
    info[4] = (s[0] == 0.0 && s[1] == 0.0) ? 0.0 : atan2(s[1], s[0]) / 6.283185307179586476925;
    info[5] = den > 0.0 ? mag / sqrt(den) : 0.0;
    info[6] = (double)q.x;
    info[7] = (double)q.y;
  }
}

__device__ inline float2 blend_one(float2 q, float alpha, float beta, float2 Z, float2 S) { return stack_mix(alpha, beta, S, stack_turn(q, Z)); }

// LOCK: zstate <- alpha * zstate + (1 - alpha) * conj(q) * Z, mag <- |zstate|.  VEC: lane i owns pixels 2i and 2i + 1 (zstate 16-byte aligned)
template <bool VEC>
__global__ __launch_bounds__(kBlendThreads) void k_cstack_blend(const float2 *__restrict__ Z, const float2 *__restrict__ qp, unsigned P,
                                                                float alpha, float2 *__restrict__ zs, float *__restrict__ mag) {
  const unsigned i = blockIdx.x * (unsigned)kBlendThreads + threadIdx.x;
  const float2 q = *qp;
  const float beta = __fsub_rn(1.f, alpha);
  unsigned m = i;   // the pixel of the one-pixel path
  if constexpr (VEC) {
    m = 2u * i;
    if (m + 1u < P) {
      const float4 z = reinterpret_cast<const float4 *>(Z)[i];
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      if (alpha != 0.f) s = reinterpret_cast<const float4 *>(zs)[i];
      const float2 a = blend_one(q, alpha, beta, make_float2(z.x, z.y), make_float2(s.x, s.y));
      const float2 b = blend_one(q, alpha, beta, make_float2(z.z, z.w), make_float2(s.z, s.w));
      reinterpret_cast<float4 *>(zs)[i] = make_float4(a.x, a.y, b.x, b.y);
      if (mag) {
        mag[m] = abs_iq_rn(a.x, a.y);
        mag[m + 1u] = abs_iq_rn(b.x, b.y);
      }
      return;
    }
  }
  if (m < P) {   // VEC: the last pixel of an odd P
    float2 s = make_float2(0.f, 0.f);
    if (alpha != 0.f) s = zs[m];
    const float2 a = blend_one(q, alpha, beta, Z[m], s);
    zs[m] = a;
    if (mag) mag[m] = abs_iq_rn(a.x, a.y);
  }
}

// the workspace of a stacking call (WS_CSTACK, above): the fold's partial sums, q, Z
struct StackWs {
  double *part;
  float2 *q, *zws;
};
bool stack_ws(tsdr_ctx *ctx, const FoldCall &c, const FoldGeom &g, StackWs &w) {
  const size_t part_bytes = 32 * g.tiles, z_off = part_bytes + 16;
  char *ws = (char *)ctx->scratch(WS_CSTACK, z_off + (c.mode == TSDR_CSTACK_LOCK ? 8 * (size_t)c.y_t * (size_t)c.x_t : 0));
  if (!ws) return false;
  w = StackWs{reinterpret_cast<double *>(ws), reinterpret_cast<float2 *>(ws + part_bytes), reinterpret_cast<float2 *>(ws + z_off)};
  return true;
}

// what follows the fold of a stacking flavour: cstack_lock when the mode or info asks for it, cstack_blend in LOCK mode
int stack_finish(tsdr_ctx *ctx, const FoldCall &c, const FoldGeom &g, const StackWs &w) {
  const size_t P = (size_t)c.y_t * (size_t)c.x_t;
  const bool lock = c.mode == TSDR_CSTACK_LOCK;
  if (lock || c.info)
    TSDR_LAUNCH(ctx, "cstack_lock", k_cstack_lock, dim3(1), dim3(64), 0, (const double *)w.part, (unsigned)g.tiles, c.mode, c.info, w.q);
  if (!lock) return TSDR_OK;
  float2 *zs = reinterpret_cast<float2 *>(c.state);
  if ((reinterpret_cast<uintptr_t>(zs) & 15u) == 0)
    TSDR_LAUNCH(ctx, "cstack_blend", k_cstack_blend<true>, dim3((unsigned)ceil_div(ceil_div(P, 2), kBlendThreads)), dim3(kBlendThreads), 0,
                (const float2 *)w.zws, (const float2 *)w.q, (unsigned)P, c.alpha, zs, c.mag);
  else
    TSDR_LAUNCH(ctx, "cstack_blend", k_cstack_blend<false>, dim3((unsigned)ceil_div(P, kBlendThreads)), dim3(kBlendThreads), 0,
                (const float2 *)w.zws, (const float2 *)w.q, (unsigned)P, c.alpha, zs, c.mag);
  return TSDR_OK;
}

}  // namespace
}  // namespace tsdr

// raster_ctrack.hip (stacking along a phase track: a weight per frame and line) includes this file for everything above -- the
// epilogue, cstack_lock, cstack_blend, the workspace -- and leaves this flavour's launches and entry points to this translation unit
#ifndef TSDR_CSTACK_NO_ENTRY_POINTS
namespace tsdr {
namespace {

int Stacked::launch(tsdr_ctx *ctx, const FoldCall &c, const FoldGeom &g, const FoldArgs<Trial> &A0) {
  StackWs w;
  if (!stack_ws(ctx, c, g, w)) return TSDR_ENOMEM;
  FoldArgs<Trial> A = A0;
  A.part = w.part;
  A.tr.zws = w.zws;
  const dim3 wg_tile(kFoldTileWaves * 64), wg_direct(kFoldDirectWaves * 64);
  if (g.staged) TSDR_LAUNCH(ctx, "cstack_tile", (k_fold_engine<Stacked, kFoldTileP, kFoldTileWaves, 1, true, false>), g.grid, wg_tile, g.lds, A);
  else TSDR_LAUNCH(ctx, "cstack_direct", (k_fold_engine<Stacked, kFoldDirectP, kFoldDirectWaves, 1, false, false>), g.grid, wg_direct, 0, A);
  return stack_finish(ctx, c, g, w);
}

// an entry point: the refusals, then the device form, or the host form around it (upload iq -- and zstate if alpha != 0 --, launch,
// download zstate and, when given, mag and info, wait)
int stack_entry(tsdr_ctx *ctx, const char *fn, const char *what, FoldCall c, bool device) {
  IqFmt f;
  if (int rc = fold_check<Stacked>(ctx, fn, c, device, f)) return rc;
  if (device) {
    TSDR_PTR_ALIGNED(ctx, fn, c.state, 8);
    TSDR_PTR_ALIGNED(ctx, fn, c.mag, 4);
    TSDR_PTR_ALIGNED(ctx, fn, c.info, 8);
  }
  if (c.F == 0) return TSDR_OK;
  if (device) return fold_launch<Stacked>(ctx, c, f);
  const size_t P = (size_t)c.y_t * (size_t)c.x_t;
  const size_t in_bytes = c.n * iq_bytes(f), z_bytes = 8 * P, mag_bytes = (4 * P + 7) & ~(size_t)7;
  HostStage st(ctx);
  c.iq = st.in(WS_IN, c.iq, in_bytes);
  c.state = (float *)st.inout(WS_OUT, c.state, z_bytes, c.alpha != 0.f);
  (void)st.reserve(WS_AUX, mag_bytes + 8 * TSDR_CSTACK_INFO);   // mag, then info (8-byte aligned), either absent or present
  c.mag = (float *)st.out(WS_AUX, c.mag, 4 * P);
  c.info = (double *)st.out(WS_AUX, c.info, 8 * TSDR_CSTACK_INFO);
  return st.run(what, [&] { return fold_launch<Stacked>(ctx, c, f); });
}

FoldCall stack_call(const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, double phi, int n_frames, int y_t,
                    int x_t, float alpha, int mode, float *zstate, float *mag, double *info) {
  FoldCall c{iq, iq_fmt, scale, n, t0, T, 0.0, kappa, 0.0, 1, n_frames, y_t, x_t, alpha, zstate, nullptr, false};
  c.phi = phi;
  c.mode = mode;
  c.mag = mag;
  c.info = info;
  return c;
}

}  // namespace
}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_cstack_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, double phi,
                     int n_frames, int y_t, int x_t, float alpha, int mode, float *zstate, float *mag, double *info) {
  return stack_entry(ctx, "cstack_iq", __func__, stack_call(iq, iq_fmt, scale, n, t0, T, kappa, phi, n_frames, y_t, x_t, alpha, mode, zstate, mag, info),
                     true);
}

int tsdr_cstack_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, double phi,
                   int n_frames, int y_t, int x_t, float alpha, int mode, float *zstate, float *mag, double *info) {
  return stack_entry(ctx, "cstack_iq", __func__, stack_call(iq, iq_fmt, scale, n, t0, T, kappa, phi, n_frames, y_t, x_t, alpha, mode, zstate, mag, info),
                     false);
}

}  // extern "C"
#endif  // TSDR_CSTACK_NO_ENTRY_POINTS
