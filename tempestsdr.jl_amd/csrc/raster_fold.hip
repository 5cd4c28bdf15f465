// raster_fold.hip -- coherent frame folding at a fractional frame period (include/tempest_hip_fold.h): the mean of the F frames a
// buffer holds when they are sampled at t0 + f*T, IIR-averaged into a y_t x x_t state, and the period scan that scores the
// pictures folded at trial periods.
//
//   k_fold<128, 8, true, .>  the tiled kernel: a workgroup (eight wavefronts) owns 64 lines x 128 pixels of the OUTPUT and loops over
//                           the frames.  Per frame it stages the |IQ| span of its 64 lines in LDS ([line][sample], odd pitch; |IQ|
//                           once per staged sample, four loads in flight per lane), then every lane walks its line: lanes are
//                           consecutive lines, a wavefront owns 16 pixel columns, a lane's 16 sums stay in registers.  The state
//                           is touched once, at the end, in contiguous 256-byte column segments per wavefront.
//   k_fold<16, 4, false, .>  the direct kernel for ratios whose span does not fit (W > TSDR_FOLD_STAGE_MAX): 64 lines x 16 pixels
//                           per workgroup, both taps of every pixel loaded and converted by the lane itself.
//   k_fold<., ., ., true>   the scan: the same body with the trial index in blockIdx.y and a score-only epilogue -- the means never
//                           leave the registers; a workgroup writes its f64 (sum x, sum x^2) to the workspace (fixed shuffle tree,
//                           then wave order), and k_fold_score adds them with one lane per trial, in tile order.
//
// Coordinates (fold_pos.h, shared with raster_cfold.hip): B = t0 + f*T is split once per frame into bi = floor(B) and bf = B - bi (exact); a pixel's position relative to bi
// is s = bf + ((m + 1/2)*(T/P) - 1/2), evaluated from m for the first pixel of a lane's run and as fma(i, T/P, s) for its i-th (one
// rounding each, no sum carried along the line), so the f64 rounding happens at the magnitude of one frame, not of the buffer.
// The buffer clamps act on s as [-bi, n-1-bi].
// Every grid is exact; sums over frames run f = 0 .. F-1 in that order in every lane: a call repeats its bits.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "down_fused.h"
#include "fold_pos.h"

namespace tsdr {
namespace {

constexpr int kThreads = 256, kLines = 64;
constexpr int kTileP = 128, kTileWaves = 8;      // pixels per tile and wavefronts per workgroup of the tiled kernel
constexpr int kDirectP = 16, kDirectWaves = 4;   // ... of the direct kernel
static_assert((TSDR_FOLD_STAGE_MAX | 1) * kLines * 4 + 4 * kLines * 2 + 2 * 8 * kTileWaves <= 65536,
              "staged span + first-sample table + partials fit 64 KiB of LDS");

struct FoldArgs {
  const float *iq;
  IqFmt fmt;
  long long n;          // samples of the buffer
  double t0, T0, dT;    // the launch's trial blockIdx.y folds at T0 + blockIdx.y * dT
  int F, y_t, x_t;
  int tiles_l;          // line tiles; tile t = (t % tiles_l, t / tiles_l): the tiles stacked over one pixel strip are neighbours
  int W;                // staged samples per line (tiled kernel)
  unsigned wmagic;      // floor(2^32 / W) + 1: idx / W == umulhi(idx, wmagic) for idx < 64 * W
  float alpha;
  float *state;         // fold
  double *part;         // scan: [trial][tile][2]
};

// FramePos, frame_pos, fold_s, fold_tap: fold_pos.h (shared with raster_cfold.hip)

template <int TP, int NW, bool STAGED, bool SCAN>
__global__ __launch_bounds__(NW * 64) void k_fold(FoldArgs A) {
  constexpr int PW = TP / NW;   // pixel columns per wavefront
  constexpr unsigned NT = NW * 64;
  extern __shared__ float smp[];             // STAGED: [64][W | 1] |IQ|
  __shared__ int kfirst[2][kLines];          // STAGED: first staged sample of every line (relative to the frame's bi), by frame parity
  __shared__ double red[2][NW];              // SCAN: the wavefronts' partial sums
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tp = (int)(blockIdx.x / (unsigned)A.tiles_l), tl = (int)(blockIdx.x - (unsigned)tp * (unsigned)A.tiles_l);
  const int l0 = tl * kLines, p0 = tp * TP;
  const double T = A.T0 + (double)blockIdx.y * A.dT;
  const unsigned P = (unsigned)A.y_t * (unsigned)A.x_t;
  const double spp = T / (double)P;
  const int l = l0 + lane;
  const bool lane_on = l < A.y_t;
  const unsigned mrow = (unsigned)min(l, A.y_t - 1) * (unsigned)A.x_t;
  const int pbeg = p0 + wave * PW;
  const int Wp = A.W | 1;
  float acc[PW];
#pragma unroll
  for (int i = 0; i < PW; ++i) acc[i] = 0.f;

  for (int f = 0; f < A.F; ++f) {
    const FramePos fp = frame_pos(A, T, f);
    if (STAGED) {
      int *kf = kfirst[f & 1];
      if (tid < kLines) {
        double d;
        kf[tid] = fold_tap(fp, fold_s(fp, spp, (unsigned)min(l0 + tid, A.y_t - 1) * (unsigned)A.x_t + (unsigned)p0), d);
      }
      __syncthreads();   // the table is complete, and every wavefront has left the previous frame's walk
      const unsigned tot = (unsigned)kLines * (unsigned)A.W;
      for (unsigned base = (unsigned)tid; base < tot; base += 4u * NT) {
        float re[4], im[4];
        unsigned at[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // the loads first, back to back
          const unsigned idx = base + (unsigned)u * NT;
          re[u] = im[u] = 0.f;
          at[u] = 0u;
          if (idx < tot) {
            const unsigned r = __umulhi(idx, A.wmagic), j = idx - r * (unsigned)A.W;
            const long long k = min(fp.bi + (long long)kf[r] + (long long)j, A.n - 1);
            const float2 z = ld_iq(A.iq, (unsigned)k, A.fmt);
            re[u] = z.x;
            im[u] = z.y;
            at[u] = r * (unsigned)Wp + j;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (base + (unsigned)u * NT < tot) smp[at[u]] = abs_iq_rn(re[u], im[u]);
      }
      __syncthreads();
    }
    if (lane_on) {
      const int rb = STAGED ? lane * Wp - kfirst[f & 1][lane] : 0;   // smp[rb + k]: sample k of this lane's line
      const double s0 = fold_s(fp, spp, mrow + (unsigned)pbeg);
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        const int p = pbeg + i;
        if (p < A.x_t) {
          double d;
          const int k = fold_tap(fp, i == 0 ? s0 : fma((double)i, spp, s0), d);
          float a, b;
          if (STAGED) {
            a = smp[rb + k];
            b = smp[rb + k + 1];
          } else {
            const unsigned ka = (unsigned)(fp.bi + (long long)k);
            const float2 za = ld_iq(A.iq, ka, A.fmt), zb = ld_iq(A.iq, ka + 1u, A.fmt);
            a = abs_iq_rn(za.x, za.y);
            b = abs_iq_rn(zb.x, zb.y);
          }
          acc[i] = __fadd_rn(acc[i], fast_blend(a, b, d));
        }
      }
    }
  }

  const float Ff = (float)A.F;
  if (!SCAN) {
    if (lane_on) {
      const float alpha = A.alpha, beta = __fsub_rn(1.f, alpha);
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        const int p = pbeg + i;
        if (p < A.x_t) {
          float *o = A.state + (size_t)p * (size_t)A.y_t + (size_t)l;
          const float mean = __fdiv_rn(acc[i], Ff);
          *o = alpha == 0.f ? mean : __fadd_rn(__fmul_rn(alpha, *o), __fmul_rn(beta, mean));
        }
      }
    }
  } else {
    double sx = 0.0, sxx = 0.0;
    if (lane_on) {
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        if (pbeg + i < A.x_t) {
          const double x = (double)__fdiv_rn(acc[i], Ff);
          sx += x;
          sxx += x * x;
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) {   // the same tree on every run
      sx += __shfl_down(sx, off);
      sxx += __shfl_down(sxx, off);
    }
    if (lane == 0) { red[0][wave] = sx; red[1][wave] = sxx; }
    __syncthreads();
    if (tid == 0) {
      double *o = A.part + ((size_t)blockIdx.y * (size_t)gridDim.x + (size_t)blockIdx.x) * 2;
      double sx = red[0][0], sxx = red[1][0];
#pragma unroll
      for (int w = 1; w < NW; ++w) {   // wave order
        sx += red[0][w];
        sxx += red[1][w];
      }
      o[0] = sx;
      o[1] = sxx;
    }
  }
}

// one lane per trial: the tiles' partial sums in tile order, then sum x^2 - (sum x)^2 / P
__global__ __launch_bounds__(kThreads) void k_fold_score(const double *__restrict__ part, unsigned tiles, int n_trials, double P,
                                                         double *__restrict__ score) {
  const int k = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (k >= n_trials) return;
  const double *q = part + (size_t)k * tiles * 2;
  double sx = 0.0, sxx = 0.0;
  unsigned t = 0;
  for (; t + 8 <= tiles; t += 8) {   // eight tiles' loads in flight, added in tile order
    double2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = reinterpret_cast<const double2 *>(q)[t + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      sx += v[u].x;
      sxx += v[u].y;
    }
  }
  for (; t < tiles; ++t) {
    sx += q[2 * t];
    sxx += q[2 * t + 1];
  }
  score[k] = sxx - sx * sx / P;
}

struct Call {
  const void *iq;
  int iq_fmt;
  float scale;
  size_t n;
  double t0, T0, dT;
  int n_trials, F, y_t, x_t;
  float alpha;
  float *state;    // fold (else null)
  double *score;   // scan (else null)
  bool scan;
};

// everything tempest_hip_fold.h (REFUSALS) refuses, before anything is enqueued or staged; device: the pointers are device pointers
int fold_check(tsdr_ctx *ctx, const char *fn, const Call &c, bool device, IqFmt &f) {
  if (!ctx) return TSDR_EINVAL;
  if (!c.iq) return set_err(ctx, TSDR_EINVAL, "%s: iq is NULL", fn);
  if (!c.scan && !c.state) return set_err(ctx, TSDR_EINVAL, "%s: state is NULL", fn);
  if (c.scan && !c.score) return set_err(ctx, TSDR_EINVAL, "%s: score is NULL", fn);
  TSDR_IQ_FMT_ARG(ctx, fn, c.iq_fmt);
  f = IqFmt{c.iq_fmt, c.iq_fmt == TSDR_IQ_CF32 ? 1.0f : c.scale};
  if (c.y_t <= 0 || c.x_t <= 0) return set_err(ctx, TSDR_EINVAL, "%s: y_t and x_t must be positive (got %d, %d)", fn, c.y_t, c.x_t);
  if ((long long)c.y_t * c.x_t >= (1ll << 31)) return set_err(ctx, TSDR_EINVAL, "%s: y_t*x_t must be below 2^31", fn);
  if (c.n < 2 || c.n >= ((size_t)1 << 31)) return set_err(ctx, TSDR_EINVAL, "%s: n must be in [2, 2^31) (got %zu)", fn, c.n);
  if (c.F < 0) return set_err(ctx, TSDR_EINVAL, "%s: n_frames must not be negative (got %d)", fn, c.F);
  if (c.n_trials < 1 || c.n_trials > TSDR_FOLD_MAX_TRIALS)
    return set_err(ctx, TSDR_EINVAL, "%s: n_trials must be in [1, %d] (got %d)", fn, TSDR_FOLD_MAX_TRIALS, c.n_trials);
  if (!std::isfinite(c.T0) || !std::isfinite(c.t0) || !std::isfinite(c.dT))
    return set_err(ctx, TSDR_EINVAL, "%s: the period, t0 and dT must be finite", fn);
  if (c.T0 < 2.0 || c.t0 < 0.0 || c.dT < 0.0)
    return set_err(ctx, TSDR_EINVAL, "%s: the period must be at least 2, t0 and dT not negative (got %g, %g, %g)", fn, c.T0, c.t0, c.dT);
  const double Tmax = c.T0 + (double)(c.n_trials - 1) * c.dT;
  if (!(c.t0 + (double)c.F * Tmax <= (double)c.n))
    return set_err(ctx, TSDR_EINVAL, "%s: t0 + n_frames*T = %.17g exceeds the %zu samples of the buffer", fn, c.t0 + (double)c.F * Tmax, c.n);
  if (!c.scan && !(c.alpha >= 0.f && c.alpha <= 1.f)) return set_err(ctx, TSDR_EINVAL, "%s: alpha must be in [0, 1] (got %g)", fn, (double)c.alpha);
  if (device) {
    TSDR_PTR_ALIGNED(ctx, fn, c.state, 4);
    TSDR_PTR_ALIGNED(ctx, fn, c.score, 8);
    const uintptr_t a = reinterpret_cast<uintptr_t>(c.iq);
    if (c.iq_fmt == TSDR_IQ_CF32 ? (a & 7u) : (a & 15u))
      return set_err(ctx, TSDR_EINVAL, "%s: iq is not aligned (ComplexF32: one sample, integer IQ: 16 bytes)", fn);
  }
  return TSDR_OK;
}

// the device form: checked arguments, F > 0
int fold_launch(tsdr_ctx *ctx, const Call &c, const IqFmt &f) {
  const double P = (double)c.y_t * (double)c.x_t;
  const double Tmax = c.T0 + (double)(c.n_trials - 1) * c.dT;
  const double wd = std::ceil((double)kTileP * (Tmax / P)) + 3.0;   // a line's span at the largest trial (tempest_hip_fold.h, COST)
  const bool staged = wd <= (double)TSDR_FOLD_STAGE_MAX;
  const int TP = staged ? kTileP : kDirectP;
  FoldArgs A{};
  A.iq = reinterpret_cast<const float *>(c.iq);
  A.fmt = f;
  A.n = (long long)c.n;
  A.t0 = c.t0; A.T0 = c.T0; A.dT = c.dT;
  A.F = c.F; A.y_t = c.y_t; A.x_t = c.x_t;
  A.tiles_l = (int)ceil_div((size_t)c.y_t, kLines);
  A.W = staged ? (int)wd : 0;
  A.wmagic = staged ? (unsigned)((1ull << 32) / (unsigned long long)A.W + 1ull) : 0u;
  A.alpha = c.alpha;
  A.state = c.state;
  const size_t tiles = (size_t)A.tiles_l * ceil_div((size_t)c.x_t, (size_t)TP);
  if (tiles >= (1ull << 31)) return set_err(ctx, TSDR_EINVAL, "fold: %zu tiles exceed the grid", tiles);
  const dim3 grid((unsigned)tiles, (unsigned)c.n_trials), wg_tile(kTileWaves * 64), wg_direct(kDirectWaves * 64);
  const size_t lds = staged ? (size_t)kLines * (size_t)(A.W | 1) * 4 : 0;
  if (!c.scan) {
    if (staged) TSDR_LAUNCH(ctx, "fold_tile", (k_fold<kTileP, kTileWaves, true, false>), grid, wg_tile, lds, A);
    else TSDR_LAUNCH(ctx, "fold_direct", (k_fold<kDirectP, kDirectWaves, false, false>), grid, wg_direct, 0, A);
    return TSDR_OK;
  }
  A.part = (double *)ctx->scratch(WS_FOLD, (size_t)c.n_trials * tiles * 16);
  if (!A.part) return TSDR_ENOMEM;
  if (staged) TSDR_LAUNCH(ctx, "fold_scan_tile", (k_fold<kTileP, kTileWaves, true, true>), grid, wg_tile, lds, A);
  else TSDR_LAUNCH(ctx, "fold_scan_direct", (k_fold<kDirectP, kDirectWaves, false, true>), grid, wg_direct, 0, A);
  TSDR_LAUNCH(ctx, "fold_score", k_fold_score, dim3((unsigned)ceil_div((size_t)c.n_trials, kThreads)), dim3(kThreads), 0,
              (const double *)A.part, (unsigned)tiles, c.n_trials, P, c.score);
  return TSDR_OK;
}

}  // namespace
}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_fold_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, int n_frames, int y_t, int x_t,
                   float alpha, float *state) {
  const Call c{iq, iq_fmt, scale, n, t0, T, 0.0, 1, n_frames, y_t, x_t, alpha, state, nullptr, false};
  IqFmt f;
  if (int rc = fold_check(ctx, "fold_iq", c, true, f)) return rc;
  if (n_frames == 0) return TSDR_OK;
  return fold_launch(ctx, c, f);
}

int tsdr_fold_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, int n_frames, int y_t, int x_t,
                 float alpha, float *state) {
  Call c{iq, iq_fmt, scale, n, t0, T, 0.0, 1, n_frames, y_t, x_t, alpha, state, nullptr, false};
  IqFmt f;
  if (int rc = fold_check(ctx, "fold_iq", c, false, f)) return rc;
  if (n_frames == 0) return TSDR_OK;
  const size_t in_bytes = n * iq_bytes(f), st_bytes = (size_t)y_t * (size_t)x_t * 4;
  void *d_iq = ctx->scratch(WS_IN, in_bytes);
  float *d_state = (float *)ctx->scratch(WS_OUT, st_bytes);
  if (!d_iq || !d_state) return TSDR_ENOMEM;
  TSDR_HIP(ctx, hipMemcpyAsync(d_iq, iq, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (alpha != 0.f) TSDR_HIP(ctx, hipMemcpyAsync(d_state, state, st_bytes, hipMemcpyHostToDevice, ctx->stream));
  c.iq = d_iq;
  c.state = d_state;
  if (int rc = fold_launch(ctx, c, f)) return rc;
  TSDR_HIP(ctx, hipMemcpyAsync(state, d_state, st_bytes, hipMemcpyDeviceToHost, ctx->stream));
  return wait_stream(ctx, ctx->stream, __func__);
}

int tsdr_fold_scan_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T0, double dT, int n_trials,
                        int n_frames, int y_t, int x_t, double *score) {
  const Call c{iq, iq_fmt, scale, n, t0, T0, dT, n_trials, n_frames, y_t, x_t, 0.f, nullptr, score, true};
  IqFmt f;
  if (int rc = fold_check(ctx, "fold_scan_iq", c, true, f)) return rc;
  if (n_frames == 0) return TSDR_OK;
  return fold_launch(ctx, c, f);
}

int tsdr_fold_scan_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T0, double dT, int n_trials,
                      int n_frames, int y_t, int x_t, double *score, int *best) {
  Call c{iq, iq_fmt, scale, n, t0, T0, dT, n_trials, n_frames, y_t, x_t, 0.f, nullptr, score, true};
  IqFmt f;
  if (int rc = fold_check(ctx, "fold_scan_iq", c, false, f)) return rc;
  if (n_frames == 0) return TSDR_OK;
  const size_t in_bytes = n * iq_bytes(f);
  void *d_iq = ctx->scratch(WS_IN, in_bytes);
  double *d_score = (double *)ctx->scratch(WS_OUT, (size_t)n_trials * 8);
  if (!d_iq || !d_score) return TSDR_ENOMEM;
  TSDR_HIP(ctx, hipMemcpyAsync(d_iq, iq, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  c.iq = d_iq;
  c.score = d_score;
  if (int rc = fold_launch(ctx, c, f)) return rc;
  TSDR_HIP(ctx, hipMemcpyAsync(score, d_score, (size_t)n_trials * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (int rc = wait_stream(ctx, ctx->stream, __func__)) return rc;
  if (best) {
    *best = -1;
    for (int k = 0; k < n_trials; ++k)
      if (score[k] == score[k] && (*best < 0 || score[k] > score[*best])) *best = k;
  }
  return TSDR_OK;
}

}  // extern "C"
