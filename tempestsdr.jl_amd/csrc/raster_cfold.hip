// raster_cfold.hip -- phase-coherent frame folding (include/tempest_hip_cfold.h): the F frames a buffer holds, sampled at t0 + f*T
// as COMPLEX samples, frame f turned by -f*kappa turns, summed, and the magnitude taken once; and the carrier scan that scores the
// energy of the pictures folded at trial kappas.
//
//   k_cfold<128, 8, 1, true, false>  the tiled fold: raster_fold.hip's k_fold with float2 samples.  A workgroup (eight wavefronts) owns
//                                    64 lines x 128 pixels of the OUTPUT and loops over the frames; per frame it stages the IQ span of
//                                    its 64 lines in LDS ([line][sample] float2, odd pitch: a lane's 8-byte reads of consecutive lines
//                                    fall on distinct bank pairs), then every lane walks its line: 16 pixels, two f32 sums each.  The
//                                    state is touched once, at the end, in contiguous 256-byte column segments per wavefront.
//   k_cfold<16, 4, 1, false, false>  the direct fold (W > TSDR_CFOLD_STAGE_MAX): 64 lines x 16 pixels, both taps loaded by the lane.
//   k_cfold<32, 8, 8, true, true>    the scan: a trial changes only the weights, so the workgroup samples z_f(m) ONCE per frame and
//   k_cfold<16, 4, 8, false, true>   accumulates w_{f,k} * z into the sums of a batch of KB = 8 trials (blockIdx.y): 4 pixels per lane
//                                    x 8 trials x 2 = 64 accumulator registers.  The pictures never leave the registers: a workgroup
//                                    writes its f64 energy per trial to the workspace (fixed shuffle tree, then wave order), and
//                                    k_cfold_score adds them with one lane per trial, in tile order.
//
// Weights: lanes 0 .. KB-1 evaluate the batch's weights of frame f (f64 sincospi, rounded once) into LDS at the frame's start, by
// frame parity, under the barrier that also publishes the staging table.  Coordinates: fold_pos.h, the envelope fold's.
// Every grid is exact; sums over frames run f = 0 .. F-1 in that order in every lane: a call repeats its bits.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "down_fused.h"
#include "fold_pos.h"

namespace tsdr {
namespace {

constexpr int kThreads = 256, kLines = 64;
constexpr int kTileP = 128, kTileWaves = 8;      // pixels per tile and wavefronts per workgroup of the tiled fold
constexpr int kScanP = 32, kScanWaves = 8;       // ... of the tiled scan
constexpr int kDirectP = 16, kDirectWaves = 4;   // ... of both direct kernels
constexpr int kBatch = 8;                        // trials per workgroup of the scan
static_assert((TSDR_CFOLD_STAGE_MAX | 1) * kLines * 8 + 4 * kLines * 2 + 2 * 8 * kBatch + 8 * kBatch * kTileWaves <= 65536,
              "staged span + first-sample table + weights + partials fit 64 KiB of LDS");

struct CfoldArgs {
  const float *iq;
  IqFmt fmt;
  long long n;              // samples of the buffer
  double t0, T;
  double kappa0, dkappa;    // trial k = blockIdx.y * KB + j turns frame f by -f * (kappa0 + k * dkappa) turns
  int n_trials;
  int F, y_t, x_t;
  int tiles_l;          // line tiles; tile t = (t % tiles_l, t / tiles_l): the tiles stacked over one pixel strip are neighbours
  int W;                // staged samples per line (tiled kernels)
  unsigned wmagic;      // floor(2^32 / W) + 1: idx / W == umulhi(idx, wmagic) for idx < 64 * W
  float alpha;
  float *state;         // fold
  double *part;         // scan: [trial][tile]
};

// w_f of tempest_hip_cfold.h (WEIGHT): x = fl64(f * kappa), r = x - floor(x), (f32(cospi(2r)), f32(-sinpi(2r)))
__device__ inline float2 cfold_weight(int f, double kappa) {
  const double x = (double)f * kappa;
  const double r = x - floor(x);
  double s, c;
  sincospi(2.0 * r, &s, &c);
  return make_float2((float)c, (float)(-s));
}

template <int TP, int NW, int KB, bool STAGED, bool SCAN>
__global__ __launch_bounds__(NW * 64) void k_cfold(CfoldArgs A) {
  constexpr int PW = TP / NW;   // pixel columns per wavefront
  constexpr unsigned NT = NW * 64;
  extern __shared__ float2 smp[];            // STAGED: [64][W | 1] IQ
  __shared__ int kfirst[2][kLines];          // STAGED: first staged sample of every line (relative to the frame's bi), by frame parity
  __shared__ float2 wts[2][KB];              // the batch's weights of a frame, by frame parity
  __shared__ double red[KB][NW];             // SCAN: the wavefronts' partial energies
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tp = (int)(blockIdx.x / (unsigned)A.tiles_l), tl = (int)(blockIdx.x - (unsigned)tp * (unsigned)A.tiles_l);
  const int l0 = tl * kLines, p0 = tp * TP;
  const int trial0 = (int)blockIdx.y * KB;
  const unsigned P = (unsigned)A.y_t * (unsigned)A.x_t;
  const double spp = A.T / (double)P;
  const int l = l0 + lane;
  const bool lane_on = l < A.y_t;
  const unsigned mrow = (unsigned)min(l, A.y_t - 1) * (unsigned)A.x_t;
  const int pbeg = p0 + wave * PW;
  const int Wp = A.W | 1;
  float accr[PW][KB], acci[PW][KB];
#pragma unroll
  for (int i = 0; i < PW; ++i)
#pragma unroll
    for (int j = 0; j < KB; ++j) accr[i][j] = acci[i][j] = 0.f;

  for (int f = 0; f < A.F; ++f) {
    const FramePos fp = frame_pos(A, A.T, f);
    if (tid < KB) wts[f & 1][tid] = cfold_weight(f, A.kappa0 + (double)(trial0 + tid) * A.dkappa);
    if (STAGED) {
      if (tid < kLines) {
        double d;
        kfirst[f & 1][tid] = fold_tap(fp, fold_s(fp, spp, (unsigned)min(l0 + tid, A.y_t - 1) * (unsigned)A.x_t + (unsigned)p0), d);
      }
    }
    __syncthreads();   // the tables are complete, and every wavefront has left the previous frame's walk
    if (STAGED) {
      const int *kf = kfirst[f & 1];
      const unsigned tot = (unsigned)kLines * (unsigned)A.W;
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
    if (lane_on) {
      float2 w[KB];
#pragma unroll
      for (int j = 0; j < KB; ++j) w[j] = wts[f & 1][j];
      const int rb = STAGED ? lane * Wp - kfirst[f & 1][lane] : 0;   // smp[rb + k]: sample k of this lane's line
      const double s0 = fold_s(fp, spp, mrow + (unsigned)pbeg);
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        const int p = pbeg + i;
        if (p < A.x_t) {
          double d;
          const int k = fold_tap(fp, i == 0 ? s0 : fma((double)i, spp, s0), d);
          float2 a, b;
          if (STAGED) {
            a = smp[rb + k];
            b = smp[rb + k + 1];
          } else {
            const unsigned ka = (unsigned)(fp.bi + (long long)k);
            a = ld_iq(A.iq, ka, A.fmt);
            b = ld_iq(A.iq, ka + 1u, A.fmt);
          }
          const float zr = fast_blend(a.x, b.x, d), zi = fast_blend(a.y, b.y, d);
#pragma unroll
          for (int j = 0; j < KB; ++j) {
            accr[i][j] = __fadd_rn(accr[i][j], __fsub_rn(__fmul_rn(w[j].x, zr), __fmul_rn(w[j].y, zi)));
            acci[i][j] = __fadd_rn(acci[i][j], __fadd_rn(__fmul_rn(w[j].x, zi), __fmul_rn(w[j].y, zr)));
          }
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
          const float c = abs_iq_rn(__fdiv_rn(accr[i][0], Ff), __fdiv_rn(acci[i][0], Ff));
          *o = alpha == 0.f ? c : __fadd_rn(__fmul_rn(alpha, *o), __fmul_rn(beta, c));
        }
      }
    }
  } else {
    double e[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) e[j] = 0.0;
    if (lane_on) {
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        if (pbeg + i < A.x_t) {
#pragma unroll
          for (int j = 0; j < KB; ++j) {
            const double zr = (double)__fdiv_rn(accr[i][j], Ff), zi = (double)__fdiv_rn(acci[i][j], Ff);
            e[j] += zr * zr + zi * zi;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      for (int off = 32; off > 0; off >>= 1) e[j] += __shfl_down(e[j], off);   // the same tree on every run
      if (lane == 0) red[j][wave] = e[j];
    }
    __syncthreads();
    if (tid < KB && trial0 + tid < A.n_trials) {
      double s = red[tid][0];
#pragma unroll
      for (int w = 1; w < NW; ++w) s += red[tid][w];   // wave order
      A.part[(size_t)(trial0 + tid) * (size_t)gridDim.x + (size_t)blockIdx.x] = s;
    }
  }
}

// one lane per trial: the tiles' partial energies in tile order
__global__ __launch_bounds__(kThreads) void k_cfold_score(const double *__restrict__ part, unsigned tiles, int n_trials,
                                                          double *__restrict__ score) {
  const int k = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (k >= n_trials) return;
  const double *q = part + (size_t)k * tiles;
  double s = 0.0;
  unsigned t = 0;
  for (; t + 8 <= tiles; t += 8) {   // eight tiles' loads in flight, added in tile order
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = q[t + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; t < tiles; ++t) s += q[t];
  score[k] = s;
}

struct Call {
  const void *iq;
  int iq_fmt;
  float scale;
  size_t n;
  double t0, T, kappa0, dkappa;
  int n_trials, F, y_t, x_t;
  float alpha;
  float *state;    // fold (else null)
  double *score;   // scan (else null)
  bool scan;
};

// everything tempest_hip_cfold.h (REFUSALS) refuses, before anything is enqueued or staged; device: the pointers are device pointers
int cfold_check(tsdr_ctx *ctx, const char *fn, const Call &c, bool device, IqFmt &f) {
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
  if (c.n_trials < 1 || c.n_trials > TSDR_CFOLD_MAX_TRIALS)
    return set_err(ctx, TSDR_EINVAL, "%s: n_trials must be in [1, %d] (got %d)", fn, TSDR_CFOLD_MAX_TRIALS, c.n_trials);
  if (!std::isfinite(c.T) || !std::isfinite(c.t0)) return set_err(ctx, TSDR_EINVAL, "%s: the period and t0 must be finite", fn);
  if (!std::isfinite(c.kappa0) || !std::isfinite(c.dkappa)) return set_err(ctx, TSDR_EINVAL, "%s: kappa and dkappa must be finite", fn);
  if (c.T < 2.0 || c.t0 < 0.0)
    return set_err(ctx, TSDR_EINVAL, "%s: the period must be at least 2 and t0 not negative (got %g, %g)", fn, c.T, c.t0);
  if (!(c.t0 + (double)c.F * c.T <= (double)c.n))
    return set_err(ctx, TSDR_EINVAL, "%s: t0 + n_frames*T = %.17g exceeds the %zu samples of the buffer", fn, c.t0 + (double)c.F * c.T, c.n);
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
int cfold_launch(tsdr_ctx *ctx, const Call &c, const IqFmt &f) {
  const double P = (double)c.y_t * (double)c.x_t;
  const double wd = std::ceil((double)kTileP * (c.T / P)) + 3.0;   // a 128-pixel line span (tempest_hip_cfold.h, COST): the choice
  const bool staged = wd <= (double)TSDR_CFOLD_STAGE_MAX;
  const int TP = !staged ? kDirectP : c.scan ? kScanP : kTileP;
  CfoldArgs A{};
  A.iq = reinterpret_cast<const float *>(c.iq);
  A.fmt = f;
  A.n = (long long)c.n;
  A.t0 = c.t0; A.T = c.T;
  A.kappa0 = c.kappa0; A.dkappa = c.dkappa;
  A.n_trials = c.n_trials;
  A.F = c.F; A.y_t = c.y_t; A.x_t = c.x_t;
  A.tiles_l = (int)ceil_div((size_t)c.y_t, kLines);
  A.W = staged ? (int)(std::ceil((double)TP * (c.T / P)) + 3.0) : 0;   // the span of the kernel's own tile
  A.wmagic = staged ? (unsigned)((1ull << 32) / (unsigned long long)A.W + 1ull) : 0u;
  A.alpha = c.alpha;
  A.state = c.state;
  const size_t tiles = (size_t)A.tiles_l * ceil_div((size_t)c.x_t, (size_t)TP);
  if (tiles >= (1ull << 31)) return set_err(ctx, TSDR_EINVAL, "cfold: %zu tiles exceed the grid", tiles);
  const dim3 grid((unsigned)tiles, (unsigned)ceil_div((size_t)c.n_trials, c.scan ? kBatch : 1));
  const dim3 wg_tile(kTileWaves * 64), wg_direct(kDirectWaves * 64);
  const size_t lds = staged ? (size_t)kLines * (size_t)(A.W | 1) * 8 : 0;
  if (!c.scan) {
    if (staged) TSDR_LAUNCH(ctx, "cfold_tile", (k_cfold<kTileP, kTileWaves, 1, true, false>), grid, wg_tile, lds, A);
    else TSDR_LAUNCH(ctx, "cfold_direct", (k_cfold<kDirectP, kDirectWaves, 1, false, false>), grid, wg_direct, 0, A);
    return TSDR_OK;
  }
  A.part = (double *)ctx->scratch(WS_CFOLD, (size_t)c.n_trials * tiles * 8);
  if (!A.part) return TSDR_ENOMEM;
  if (staged) TSDR_LAUNCH(ctx, "cfold_scan_tile", (k_cfold<kScanP, kScanWaves, kBatch, true, true>), grid, wg_tile, lds, A);
  else TSDR_LAUNCH(ctx, "cfold_scan_direct", (k_cfold<kDirectP, kDirectWaves, kBatch, false, true>), grid, wg_direct, 0, A);
  TSDR_LAUNCH(ctx, "cfold_score", k_cfold_score, dim3((unsigned)ceil_div((size_t)c.n_trials, kThreads)), dim3(kThreads), 0,
              (const double *)A.part, (unsigned)tiles, c.n_trials, c.score);
  return TSDR_OK;
}

}  // namespace
}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_cfold_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, int n_frames,
                    int y_t, int x_t, float alpha, float *state) {
  const Call c{iq, iq_fmt, scale, n, t0, T, kappa, 0.0, 1, n_frames, y_t, x_t, alpha, state, nullptr, false};
  IqFmt f;
  if (int rc = cfold_check(ctx, "cfold_iq", c, true, f)) return rc;
  if (n_frames == 0) return TSDR_OK;
  return cfold_launch(ctx, c, f);
}

int tsdr_cfold_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, int n_frames,
                  int y_t, int x_t, float alpha, float *state) {
  Call c{iq, iq_fmt, scale, n, t0, T, kappa, 0.0, 1, n_frames, y_t, x_t, alpha, state, nullptr, false};
  IqFmt f;
  if (int rc = cfold_check(ctx, "cfold_iq", c, false, f)) return rc;
  if (n_frames == 0) return TSDR_OK;
  const size_t in_bytes = n * iq_bytes(f), st_bytes = (size_t)y_t * (size_t)x_t * 4;
  void *d_iq = ctx->scratch(WS_IN, in_bytes);
  float *d_state = (float *)ctx->scratch(WS_OUT, st_bytes);
  if (!d_iq || !d_state) return TSDR_ENOMEM;
  TSDR_HIP(ctx, hipMemcpyAsync(d_iq, iq, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (alpha != 0.f) TSDR_HIP(ctx, hipMemcpyAsync(d_state, state, st_bytes, hipMemcpyHostToDevice, ctx->stream));
  c.iq = d_iq;
  c.state = d_state;
  if (int rc = cfold_launch(ctx, c, f)) return rc;
  TSDR_HIP(ctx, hipMemcpyAsync(state, d_state, st_bytes, hipMemcpyDeviceToHost, ctx->stream));
  return wait_stream(ctx, ctx->stream, __func__);
}

int tsdr_cfold_scan_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa0,
                         double dkappa, int n_trials, int n_frames, int y_t, int x_t, double *score) {
  const Call c{iq, iq_fmt, scale, n, t0, T, kappa0, dkappa, n_trials, n_frames, y_t, x_t, 0.f, nullptr, score, true};
  IqFmt f;
  if (int rc = cfold_check(ctx, "cfold_scan_iq", c, true, f)) return rc;
  if (n_frames == 0) return TSDR_OK;
  return cfold_launch(ctx, c, f);
}

int tsdr_cfold_scan_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa0,
                       double dkappa, int n_trials, int n_frames, int y_t, int x_t, double *score, int *best) {
  Call c{iq, iq_fmt, scale, n, t0, T, kappa0, dkappa, n_trials, n_frames, y_t, x_t, 0.f, nullptr, score, true};
  IqFmt f;
  if (int rc = cfold_check(ctx, "cfold_scan_iq", c, false, f)) return rc;
  if (n_frames == 0) return TSDR_OK;
  const size_t in_bytes = n * iq_bytes(f);
  void *d_iq = ctx->scratch(WS_IN, in_bytes);
  double *d_score = (double *)ctx->scratch(WS_OUT, (size_t)n_trials * 8);
  if (!d_iq || !d_score) return TSDR_ENOMEM;
  TSDR_HIP(ctx, hipMemcpyAsync(d_iq, iq, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  c.iq = d_iq;
  c.score = d_score;
  if (int rc = cfold_launch(ctx, c, f)) return rc;
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
