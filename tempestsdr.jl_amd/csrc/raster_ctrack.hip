// raster_ctrack.hip -- carrier tracking (include/tempest_hip_ctrack.h): the weight of a sample is a function of frame AND raster line,
// given as data -- a track of (a_f, b_f) turns per frame, w_f(l) = coh_weight(fma(b_f, (l + 1/2) / y_t, a_f)) -- so a carrier that
// drifts inside a buffer, or that was retuned by whole turns per frame, folds coherently.  Two operations:
//
//   the stack   tsdr_ctrack_stack_iq*: coherent stacking (raster_cstack.hip) along a track.  A third coherent flavour of fold_engine.h,
//               `Tracked`, whose weights are per line (Flavour::line_weights: 64 lanes fill a [2][64] LDS table per frame under the
//               barrier that publishes the staging table); the epilogue (Stacked::stack), cstack_lock, cstack_blend and the workspace
//               are raster_cstack.hip's own, included below without its entry points: a track that is constant along the lines
//               leaves cstack's bits by construction.  Profile names ctrack_stack_tile / ctrack_stack_direct.
//   the probe   tsdr_ctrack_probe_iq*: every frame's inner product with a reference picture S, rho_f = sum_m w_f(l) z_f(m) conj(S(m)),
//               with E_f and E_s.  ctrack_probe_tile / ctrack_probe_direct have the fold's tiles, staging and walk (frame_pos,
//               fold_s, fold_tap, the same staged / direct choice and W: fold_launch makes the geometry), but a lane
//               keeps S of its pixels in registers for the whole frame loop and sums nothing across frames: per frame it reduces its
//               pixels' three f64 sums (lane pixel order, the fixed shuffle tree, wave order) into the workspace WS_CTRACK,
//               [frame][tile][4] with the tile's share of E_s in the fourth place.  ctrack_probe_sum, one lane per frame, adds the tiles
//               in tile order and forms gamma_f.  No atomics.
#define TSDR_CSTACK_NO_ENTRY_POINTS
#include "raster_cstack.hip"

namespace tsdr {
namespace {

static_assert((TSDR_CFOLD_STAGE_MAX | 1) * kFoldLines * 8 + 4 * kFoldLines * 2 + 2 * 8 + 8 * kFoldLines * 2 + 8 * 4 * kFoldTileWaves <= 65536,
              "the stack: staged span + first-sample table + weight + line weights + the four sums' partials fit 64 KiB of LDS");
static_assert((TSDR_CFOLD_STAGE_MAX | 1) * kFoldLines * 8 + 4 * kFoldLines * 2 + 8 * kFoldLines * 2 + 8 * (2 * 3 + 1) * kFoldTileWaves <= 65536,
              "the probe: staged span + first-sample table + line weights + the partials of two frames and of E_s fit 64 KiB of LDS");

// (a_f, b_f) of a track; a null track is the zero track, evaluated by the same arithmetic
__device__ inline float2 track_weight(const double *track, int f, int l, int y_t) {
  const double a = track ? track[2 * (size_t)f] : 0.0, b = track ? track[2 * (size_t)f + 1] : 0.0;
  return coh_line_weight(a, b, l, y_t);
}

int refuse_period(tsdr_ctx *ctx, const char *fn, const FoldCall &c) {
  if (!std::isfinite(c.T) || !std::isfinite(c.t0)) return set_err(ctx, TSDR_EINVAL, "%s: the period and t0 must be finite", fn);
  if (c.T < 2.0 || c.t0 < 0.0)
    return set_err(ctx, TSDR_EINVAL, "%s: the period must be at least 2 and t0 not negative (got %g, %g)", fn, c.T, c.t0);
  return TSDR_OK;
}

// the host forms read the track: every entry finite
int refuse_track_values(tsdr_ctx *ctx, const char *fn, const FoldCall &c) {
  for (size_t i = 0; c.track && i < 2 * (size_t)c.F; ++i)
    if (!std::isfinite(c.track[i]))
      return set_err(ctx, TSDR_EINVAL, "%s: track[%zu] (frame %zu) is not finite", fn, i, i / 2);
  return TSDR_OK;
}

// ---------------------------------------------------------------- the stack
struct Tracked {
  using Sample = float2;
  struct Trial {
    double T;
    const double *track;    // frame f on line l is turned by -(a_f + b_f * c_l) turns
    int mode;
    float *mag;             // GIVEN: |S'| (may be null)
    float2 *zws;            // LOCK: Z, in state order
  };
  static constexpr bool has_weights = true, stacks = true, line_weights = true;
  static constexpr int NS = 4, kMaxTrials = 1, kStageMax = TSDR_CFOLD_STAGE_MAX, kSlot = WS_CSTACK;
  static constexpr const char *name = "ctrack_stack";
  static int tile_p(bool) { return kFoldTileP; }
  static int batch(bool) { return 1; }

  __device__ static float2 stage(float2 z) { return z; }
  __device__ static double period(const Trial &t, unsigned) { return t.T; }
  __device__ static bool live(const Trial &, int) { return true; }
  __device__ static float2 line_weight(const Trial &t, int f, int l, int y_t) { return track_weight(t.track, f, l, y_t); }
  __device__ static float2 blend(float2 a, float2 b, double d) { return coh_blend(a, b, d); }
  __device__ static void add(float2 &a, float2 z, float2 w) { coh_add(a, z, w); }
  __device__ static void stack(const FoldArgs<Trial> &A, double *s, float2 acc, float Ff, size_t at) { Stacked::stack(A, s, acc, Ff, at); }

  static int refuse(tsdr_ctx *ctx, const char *fn, const FoldCall &c) {
    if (int rc = refuse_period(ctx, fn, c)) return rc;
    if (c.mode != TSDR_CSTACK_GIVEN && c.mode != TSDR_CSTACK_LOCK)
      return set_err(ctx, TSDR_EINVAL, "%s: mode must be TSDR_CSTACK_GIVEN or TSDR_CSTACK_LOCK (got %d)", fn, c.mode);
    if (!c.track) return set_err(ctx, TSDR_EINVAL, "%s: track is NULL", fn);
    return TSDR_OK;
  }
  static Trial trial(const FoldCall &c) { return Trial{c.T, c.track, c.mode, c.mag, nullptr}; }
  static int launch(tsdr_ctx *ctx, const FoldCall &c, const FoldGeom &g, const FoldArgs<Trial> &A0) {
    StackWs w;
    if (!stack_ws(ctx, c, g, w)) return TSDR_ENOMEM;
    FoldArgs<Trial> A = A0;
    A.part = w.part;
    A.tr.zws = w.zws;
    const dim3 wg_tile(kFoldTileWaves * 64), wg_direct(kFoldDirectWaves * 64);
    if (g.staged)
      TSDR_LAUNCH(ctx, "ctrack_stack_tile", (k_fold_engine<Tracked, kFoldTileP, kFoldTileWaves, 1, true, false>), g.grid, wg_tile, g.lds, A);
    else
      TSDR_LAUNCH(ctx, "ctrack_stack_direct", (k_fold_engine<Tracked, kFoldDirectP, kFoldDirectWaves, 1, false, false>), g.grid, wg_direct, 0, A);
    return stack_finish(ctx, c, g, w);
  }
};

// an entry point of the stack: the refusals, then the device form, or the host form around it (upload iq, the track -- and zstate
// if alpha != 0 --, launch, download zstate and, when given, mag and info, wait)
int track_stack_entry(tsdr_ctx *ctx, const char *fn, const char *what, FoldCall c, bool device) {
  IqFmt f;
  if (int rc = fold_check<Tracked>(ctx, fn, c, device, f)) return rc;
  if (device) {
    TSDR_PTR_ALIGNED(ctx, fn, c.state, 8);
    TSDR_PTR_ALIGNED(ctx, fn, c.mag, 4);
    TSDR_PTR_ALIGNED(ctx, fn, c.info, 8);
    TSDR_PTR_ALIGNED(ctx, fn, c.track, 8);
  } else if (int rc = refuse_track_values(ctx, fn, c)) {
    return rc;
  }
  if (c.F == 0) return TSDR_OK;
  if (device) return fold_launch<Tracked>(ctx, c, f);
  const size_t P = (size_t)c.y_t * (size_t)c.x_t;
  const size_t in_bytes = c.n * iq_bytes(f), z_bytes = 8 * P, mag_bytes = (4 * P + 7) & ~(size_t)7, track_bytes = 16 * (size_t)c.F;
  HostStage st(ctx);
  c.iq = st.in(WS_IN, c.iq, in_bytes);
  c.state = (float *)st.inout(WS_OUT, c.state, z_bytes, c.alpha != 0.f);
  (void)st.reserve(WS_AUX, mag_bytes + 8 * TSDR_CSTACK_INFO + track_bytes);   // mag, then info, then the track (8-byte aligned ranges)
  c.mag = (float *)st.out(WS_AUX, c.mag, 4 * P);
  c.info = (double *)st.out(WS_AUX, c.info, 8 * TSDR_CSTACK_INFO);
  c.track = (const double *)st.in(WS_AUX, c.track, track_bytes);
  return st.run(what, [&] { return fold_launch<Tracked>(ctx, c, f); });
}

// ---------------------------------------------------------------- the probe
struct ProbeTrial {
  double T;
  const double *track;    // may be null: the zero track
  const float2 *zref;     // S, in state order
};

// v conj(S) and |v|^2: products in f64 of the f32 values (exact), one f64 addition each -- stack_sums without E_s
__device__ inline void probe_sums(double *s, float2 v, float2 S) {
  const double vr = (double)v.x, vi = (double)v.y, sr = (double)S.x, si = (double)S.y;
  s[0] += vr * sr + vi * si;
  s[1] += vi * sr - vr * si;
  s[2] += vr * vr + vi * vi;
}

// The host side of a flavour (fold_check, fold_launch: the refusals, the staged / direct choice, W, the tiles) with kernels of its own.
// FoldCall::state carries `out`.
struct Probe {
  using Sample = float2;
  using Trial = ProbeTrial;
  static constexpr int NS = 4, kMaxTrials = 1, kStageMax = TSDR_CFOLD_STAGE_MAX, kSlot = WS_CTRACK;   // (NS: doubles per frame and tile)
  static constexpr const char *name = "ctrack_probe";
  static int tile_p(bool) { return kFoldTileP; }
  static int batch(bool) { return 1; }
  static int refuse(tsdr_ctx *ctx, const char *fn, const FoldCall &c) { return refuse_period(ctx, fn, c); }
  static Trial trial(const FoldCall &c) { return Trial{c.T, c.track, reinterpret_cast<const float2 *>(c.zref)}; }
  static int launch(tsdr_ctx *ctx, const FoldCall &c, const FoldGeom &g, const FoldArgs<Trial> &A);
};

template <int TP, int NW, bool STAGED>
__global__ __launch_bounds__(NW * 64) void k_ctrack_probe(FoldArgs<ProbeTrial> A) {
  constexpr int PW = TP / NW;
  constexpr unsigned NT = NW * 64;
  extern __shared__ float2 smp[];              // STAGED: [64][W | 1] samples
  __shared__ int kfirst[2][kFoldLines];        // STAGED: first staged sample of every line, by frame parity
  __shared__ float2 lwts[2][kFoldLines];       // the tile's 64 lines' weights of a frame, by frame parity
  __shared__ double red[2][3][NW];             // the wavefronts' partial sums of a frame, by frame parity
  __shared__ double red_s[NW];                 // ... of E_s
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tp = (int)(blockIdx.x / (unsigned)A.tiles_l), tl = (int)(blockIdx.x - (unsigned)tp * (unsigned)A.tiles_l);
  const int l0 = tl * kFoldLines, p0 = tp * TP;
  const double T = A.tr.T;
  const unsigned P = (unsigned)A.y_t * (unsigned)A.x_t;
  const double spp = T / (double)P;
  const int l = l0 + lane;
  const bool lane_on = l < A.y_t;
  const unsigned mrow = (unsigned)min(l, A.y_t - 1) * (unsigned)A.x_t;
  const int pbeg = p0 + wave * PW;
  const int Wp = A.W | 1;

  float2 S[PW];   // the reference at this lane's pixels: read once, kept for every frame
  double es = 0.0;
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    S[i] = make_float2(0.f, 0.f);
    if (lane_on && pbeg + i < A.x_t) {
      S[i] = A.tr.zref[(size_t)(pbeg + i) * (size_t)A.y_t + (size_t)l];
      const double sr = (double)S[i].x, si = (double)S[i].y;
      es += sr * sr + si * si;
    }
  }
  for (int off = 32; off > 0; off >>= 1) es += __shfl_down(es, off);
  if (lane == 0) red_s[wave] = es;
  __syncthreads();
  double es_tile = red_s[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) es_tile += red_s[w];   // wave order

  for (int f = 0; f < A.F; ++f) {
    const FramePos fp = frame_pos(A, T, f);
    if (tid < kFoldLines) {
      lwts[f & 1][tid] = track_weight(A.tr.track, f, min(l0 + tid, A.y_t - 1), A.y_t);
      if constexpr (STAGED) {
        double d;
        kfirst[f & 1][tid] = fold_tap(fp, fold_s(fp, spp, (unsigned)min(l0 + tid, A.y_t - 1) * (unsigned)A.x_t + (unsigned)p0), d);
      }
    }
    __syncthreads();   // the tables are complete, and every wavefront has left the previous frame's walk
    if constexpr (STAGED) {   // the engine's staging, statement for statement (kept in its kernel: hoisting it into a shared function
                              // moved the fold kernels' register allocation)
      const int *kf = kfirst[f & 1];
      const unsigned tot = (unsigned)kFoldLines * (unsigned)A.W;
      for (unsigned base = (unsigned)tid; base < tot; base += 4u * NT) {
        float2 z[4];
        unsigned at[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // the loads first, back to back
          const unsigned idx = base + (unsigned)u * NT;
          z[u] = make_float2(0.f, 0.f);
          at[u] = 0u;
          if (idx < tot) {
            const unsigned r = __umulhi(idx, A.wmagic), j = idx - r * (unsigned)A.W;
            const long long k = min(fp.bi + (long long)kf[r] + (long long)j, A.n - 1);
            z[u] = ld_iq(A.iq, (unsigned)k, A.fmt);
            at[u] = r * (unsigned)Wp + j;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (base + (unsigned)u * NT < tot) smp[at[u]] = z[u];
      }
      __syncthreads();
    }
    double st[3] = {0.0, 0.0, 0.0};
    if (lane_on) {
      const float2 w = lwts[f & 1][lane];
      const int rb = STAGED ? lane * Wp - kfirst[f & 1][lane] : 0;   // smp[rb + k]: sample k of this lane's line
      const double s0 = fold_s(fp, spp, mrow + (unsigned)pbeg);
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        if (pbeg + i < A.x_t) {
          double d;
          const int k = fold_tap(fp, i == 0 ? s0 : fma((double)i, spp, s0), d);
          float2 a, b;
          if constexpr (STAGED) {
            a = smp[rb + k];
            b = smp[rb + k + 1];
          } else {
            const unsigned ka = (unsigned)(fp.bi + (long long)k);
            a = ld_iq(A.iq, ka, A.fmt);
            b = ld_iq(A.iq, ka + 1u, A.fmt);
          }
          probe_sums(st, coh_mul(coh_blend(a, b, d), w), S[i]);
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) {   // the same tree on every run
#pragma unroll
      for (int s = 0; s < 3; ++s) st[s] += __shfl_down(st[s], off);
    }
    if (lane == 0) {
#pragma unroll
      for (int s = 0; s < 3; ++s) red[f & 1][s][wave] = st[s];
    }
    __syncthreads();   // (red is by frame parity: the next frame's partials land beside these)
    if (tid == 0) {
      double *o = A.part + ((size_t)f * (size_t)gridDim.x + (size_t)blockIdx.x) * 4;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        double v = red[f & 1][s][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) v += red[f & 1][s][w];   // wave order
        o[s] = v;
      }
      o[3] = es_tile;
    }
  }
}

// one lane per frame: the tiles' partial sums in tile order, then gamma_f; frame 0's lane also leaves E_s
__global__ __launch_bounds__(kFoldThreads) void k_ctrack_probe_sum(const double *__restrict__ part, unsigned tiles, int F,
                                                                   double *__restrict__ out) {
  const int f = (int)(blockIdx.x * kFoldThreads + threadIdx.x);
  if (f >= F) return;
  const double2 *q = reinterpret_cast<const double2 *>(part) + 2 * (size_t)f * tiles;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (unsigned t = 0; t < tiles; ++t) {
    const double2 a = q[2 * (size_t)t], b = q[2 * (size_t)t + 1];
    s[0] += a.x;
    s[1] += a.y;
    s[2] += b.x;
    s[3] += b.y;
  }
  const double den = s[2] * s[3];
  double *o = out + 4 * (size_t)f;
  o[0] = s[0];
  o[1] = s[1];
  o[2] = s[2];
  o[3] = den > 0.0 ? hypot(s[0], s[1]) / sqrt(den) : 0.0;
  if (f == 0) out[4 * (size_t)F] = s[3];
}

int Probe::launch(tsdr_ctx *ctx, const FoldCall &c, const FoldGeom &g, const FoldArgs<Trial> &A0) {
  FoldArgs<Trial> A = A0;
  A.part = (double *)ctx->scratch(WS_CTRACK, (size_t)c.F * g.tiles * 32);
  if (!A.part) return TSDR_ENOMEM;
  if (g.staged) TSDR_LAUNCH(ctx, "ctrack_probe_tile", (k_ctrack_probe<kFoldTileP, kFoldTileWaves, true>), g.grid, dim3(kFoldTileWaves * 64), g.lds, A);
  else TSDR_LAUNCH(ctx, "ctrack_probe_direct", (k_ctrack_probe<kFoldDirectP, kFoldDirectWaves, false>), g.grid, dim3(kFoldDirectWaves * 64), 0, A);
  TSDR_LAUNCH(ctx, "ctrack_probe_sum", k_ctrack_probe_sum, dim3((unsigned)ceil_div((size_t)c.F, kFoldThreads)), dim3(kFoldThreads), 0,
              (const double *)A.part, (unsigned)g.tiles, c.F, reinterpret_cast<double *>(c.state));
  return TSDR_OK;
}

// an entry point of the probe: the refusals, then the device form, or the host form around it (upload iq, zref and the track, launch,
// download out, wait)
int track_probe_entry(tsdr_ctx *ctx, const char *fn, const char *what, FoldCall c, double *out, bool device) {
  if (!ctx) return TSDR_EINVAL;
  if (!c.zref) return set_err(ctx, TSDR_EINVAL, "%s: zref is NULL", fn);
  if (!out) return set_err(ctx, TSDR_EINVAL, "%s: out is NULL", fn);
  c.state = reinterpret_cast<float *>(out);
  IqFmt f;
  if (int rc = fold_check<Probe>(ctx, fn, c, device, f)) return rc;
  if (device) {
    TSDR_PTR_ALIGNED(ctx, fn, out, 8);
    TSDR_PTR_ALIGNED(ctx, fn, c.zref, 8);
    TSDR_PTR_ALIGNED(ctx, fn, c.track, 8);
  } else if (int rc = refuse_track_values(ctx, fn, c)) {
    return rc;
  }
  if (c.F == 0) return TSDR_OK;
  if (device) return fold_launch<Probe>(ctx, c, f);
  const size_t P = (size_t)c.y_t * (size_t)c.x_t, track_bytes = 16 * (size_t)c.F;
  HostStage st(ctx);
  c.iq = st.in(WS_IN, c.iq, c.n * iq_bytes(f));
  c.state = (float *)st.out(WS_OUT, out, 8 * (4 * (size_t)c.F + 1));
  (void)st.reserve(WS_AUX, 8 * P + track_bytes);   // zref, then the track (absent or present)
  c.zref = (const float *)st.in(WS_AUX, c.zref, 8 * P);
  c.track = (const double *)st.in(WS_AUX, c.track, track_bytes);
  return st.run(what, [&] { return fold_launch<Probe>(ctx, c, f); });
}

FoldCall track_call(const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track, int n_frames, int y_t,
                    int x_t) {
  FoldCall c{iq, iq_fmt, scale, n, t0, T, 0.0, 0.0, 0.0, 1, n_frames, y_t, x_t, 0.f, nullptr, nullptr, false};
  c.track = track;
  return c;
}

FoldCall track_stack_call(const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track, int n_frames, int y_t,
                          int x_t, float alpha, int mode, float *zstate, float *mag, double *info) {
  FoldCall c = track_call(iq, iq_fmt, scale, n, t0, T, track, n_frames, y_t, x_t);
  c.alpha = alpha;
  c.state = zstate;
  c.mode = mode;
  c.mag = mag;
  c.info = info;
  return c;
}

FoldCall track_probe_call(const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track, int n_frames, int y_t,
                          int x_t, const float *zref) {
  FoldCall c = track_call(iq, iq_fmt, scale, n, t0, T, track, n_frames, y_t, x_t);
  c.zref = zref;
  return c;
}

}  // namespace
}  // namespace tsdr

// raster_gram.hip (the frame Gram matrix along a track) includes this file for everything above -- the track's weight, the refusals
// of a period and of a track's values, the call record -- and leaves the entry points to this translation unit
#ifndef TSDR_CTRACK_NO_ENTRY_POINTS
using namespace tsdr;

extern "C" {

int tsdr_ctrack_stack_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                           int n_frames, int y_t, int x_t, float alpha, int mode, float *zstate, float *mag, double *info) {
  return track_stack_entry(ctx, "ctrack_stack_iq", __func__,
                           track_stack_call(iq, iq_fmt, scale, n, t0, T, track, n_frames, y_t, x_t, alpha, mode, zstate, mag, info), true);
}

int tsdr_ctrack_stack_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                         int n_frames, int y_t, int x_t, float alpha, int mode, float *zstate, float *mag, double *info) {
  return track_stack_entry(ctx, "ctrack_stack_iq", __func__,
                           track_stack_call(iq, iq_fmt, scale, n, t0, T, track, n_frames, y_t, x_t, alpha, mode, zstate, mag, info), false);
}

int tsdr_ctrack_probe_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                           int n_frames, int y_t, int x_t, const float *zref, double *out) {
  return track_probe_entry(ctx, "ctrack_probe_iq", __func__, track_probe_call(iq, iq_fmt, scale, n, t0, T, track, n_frames, y_t, x_t, zref), out,
                           true);
}

int tsdr_ctrack_probe_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                         int n_frames, int y_t, int x_t, const float *zref, double *out) {
  return track_probe_entry(ctx, "ctrack_probe_iq", __func__, track_probe_call(iq, iq_fmt, scale, n, t0, T, track, n_frames, y_t, x_t, zref), out,
                           false);
}

}  // extern "C"
#endif  // TSDR_CTRACK_NO_ENTRY_POINTS
