// fold_engine.h -- the one body of frame folding: raster_fold.hip (the envelope fold, include/tempest_hip_fold.h) and raster_cfold.hip
// (the phase-coherent fold, include/tempest_hip_cfold.h) sample frame f of a buffer at the same positions, stage, walk, average and
// score it the same way, and differ in a Flavour only (below).  Each file holds its flavour, its launches and its entry points.
//
//   k_fold_engine<Fl, 128, 8, 1, true, .>  the tiled kernel: a workgroup (eight wavefronts) owns 64 lines x 128 pixels of the OUTPUT and
//                           loops over the frames.  Per frame it stages the span of its 64 lines in LDS ([line][sample] of Fl::Sample,
//                           odd pitch; Fl::stage once per staged sample, four loads in flight per lane), then every lane walks its line:
//                           lanes are consecutive lines, a wavefront owns 16 pixel columns, a lane's sums stay in registers.  The state
//                           is touched once, at the end, in contiguous 256-byte column segments per wavefront.
//   k_fold_engine<Fl, 16, 4, ., false, .>  the direct kernel for ratios whose span does not fit (W > Fl::kStageMax): 64 lines x 16 pixels
//                           per workgroup, both taps of every pixel loaded and staged by the lane itself.
//   k_fold_engine<., ., ., KB, ., true>    the scan: the same body with a batch of KB trials in blockIdx.y, KB sums per pixel and a
//                           score-only epilogue -- the pictures never leave the registers; a workgroup writes Fl::NS f64 statistics per
//                           trial to the workspace (fixed shuffle tree, then wave order), and k_fold_score adds them with one lane per
//                           trial, in tile order.
//   k_fold_engine<Fl with stacks, ., ., 1, ., false>   the fold of a flavour that keeps its picture complex: the scan's epilogue
//                           with one trial, in which Fl::stack also stores the pixel (raster_cstack.hip).
//
// A Flavour is a struct of constants and static functions:
//   Sample, Trial              the staged sample, the trial parameters a launch carries (FoldArgs::tr)
//   has_weights, NS            whether frame f of trial k has a weight; f64 statistics per trial of the scan
//   line_weights               the weight of frame f is a function of the raster line too (raster_ctrack.hip; one trial): the lane is
//                              the line, so lanes 0 .. 63 evaluate line_weight(tr, f, l, y_t) of the tile's 64 lines into LDS where
//                              `weight` would fill its KB entries, and a lane's walk reads its own line's entry
//   stacks                     the fold keeps its picture complex (raster_cstack.hip): its epilogue is the scan's with one trial, and
//                              stack(A, s, acc, Ff, at) per pixel -- the pixel's share of the NS statistics and its stores at state
//                              index `at` -- in place of stat; the tile's NS sums land at part[tile][NS]
//   kMaxTrials, kStageMax      the header's limits;  kSlot: the scan's workspace;  name: the prefix of its launch's message
//   tile_p(scan), batch(scan)  host: pixels per tile of the call's staged kernel, and its trials per workgroup
//   stage(float2) -> Sample    __device__: what is kept of an IQ sample
//   period(tr, y)              __device__: the frame period of the workgroups at blockIdx.y == y
//   live(tr, k)                __device__: trial k exists (the last batch of a scan may be ragged)
//   weight(tr, f, k)           __device__, has_weights only: lanes 0 .. KB-1 evaluate the batch's weights of frame f into LDS at the
//                              frame's start, by frame parity, under the barrier that also publishes the staging table
//   blend(a, b, d) -> Sample, add(acc, z, w)   __device__: the interpolated sample, and its accumulation into one trial's sum (a float2)
//   pixel(acc, Ff) -> float    __device__: the fold's picture element;  stat(s, acc, Ff): its contribution to the scan's statistics
//   finish(s, P) -> double     __device__: a trial's score from its summed statistics
//   refuse(ctx, fn, c)         host: the flavour's refusals of the period, t0 and the trial parameters
//   trial(c) -> Trial, launch(ctx, c, g, A)    host: FoldArgs::tr of a call, and the five TSDR_LAUNCH lines
//
// Coordinates: B = t0 + f*T is split once per frame into bi = floor(B) and bf = B - bi (exact); a pixel's position relative to bi
// is s = bf + ((m + 1/2)*(T/P) - 1/2), evaluated from m for the first pixel of a lane's run and as fma(i, T/P, s) for its i-th (one
// rounding each, no sum carried along the line), so the f64 rounding happens at the magnitude of one frame, not of the buffer.
// The buffer clamps act on s as [-bi, n-1-bi].
// Every grid is exact; sums over frames run f = 0 .. F-1 in that order in every lane: a call repeats its bits.
#pragma once
#include <algorithm>
#include <cmath>

#include "common.h"
#include "down_fused.h"

namespace tsdr {

constexpr int kFoldThreads = 256, kFoldLines = 64;
constexpr int kFoldTileP = 128, kFoldTileWaves = 8;      // pixels per tile and wavefronts per workgroup of the tiled kernel
constexpr int kFoldDirectP = 16, kFoldDirectWaves = 4;   // ... of the direct kernel

template <typename Trial>
struct FoldArgs {
  const float *iq;
  IqFmt fmt;
  long long n;          // samples of the buffer
  double t0;
  int F, y_t, x_t;
  int tiles_l;          // line tiles; tile t = (t % tiles_l, t / tiles_l): the tiles stacked over one pixel strip are neighbours
  int W;                // staged samples per line (tiled kernels)
  unsigned wmagic;      // floor(2^32 / W) + 1: idx / W == umulhi(idx, wmagic) for idx < 64 * W
  float alpha;
  float *state;         // fold
  double *part;         // scan: [trial][tile][NS]
  Trial tr;
};

struct FramePos {   // one frame's origin: integer part, and the clamps relative to it
  double bf, lo, hi, hik;
  long long bi;
};

// A: a launch's arguments with t0 (double) and n (long long, samples of the buffer)
template <typename Args>
__device__ inline FramePos frame_pos(const Args &A, double T, int f) {
  const double B = A.t0 + (double)f * T;
  const double bi = floor(B);
  return FramePos{B - bi, -bi, (double)(A.n - 1) - bi, (double)(A.n - 2) - bi, (long long)bi};
}

// position of pixel m of the frame at `fp`, relative to fp.bi, before the buffer clamps
__device__ inline double fold_s(const FramePos &fp, double spp, unsigned m) { return fp.bf + (((double)m + 0.5) * spp - 0.5); }
// ... its left tap (relative to fp.bi) and the weight of the right one
__device__ inline int fold_tap(const FramePos &fp, double s, double &d) {
  s = fmin(fmax(s, fp.lo), fp.hi);
  const double k = fmin(floor(s), fp.hik);
  d = s - k;
  return (int)k;
}

template <class Fl, int TP, int NW, int KB, bool STAGED, bool SCAN>
__global__ __launch_bounds__(NW * 64) void k_fold_engine(FoldArgs<typename Fl::Trial> A) {
  using Sample = typename Fl::Sample;
  constexpr int PW = TP / NW, NS = Fl::NS;   // pixel columns per wavefront
  constexpr unsigned NT = NW * 64;
  extern __shared__ Sample smp[];              // STAGED: [64][W | 1] samples
  __shared__ int kfirst[2][kFoldLines];        // STAGED: first staged sample of every line (relative to the frame's bi), by frame parity
  __shared__ float2 wts[2][KB];                // has_weights: the batch's weights of a frame, by frame parity
  __shared__ float2 lwts[2][Fl::line_weights ? kFoldLines : 1];   // line_weights: the tile's 64 lines' weights of a frame instead
  __shared__ double red[KB][NS][NW];           // SCAN: the wavefronts' partial statistics
  static_assert(!Fl::line_weights || (Fl::has_weights && KB == 1), "weights per line: one trial");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tp = (int)(blockIdx.x / (unsigned)A.tiles_l), tl = (int)(blockIdx.x - (unsigned)tp * (unsigned)A.tiles_l);
  const int l0 = tl * kFoldLines, p0 = tp * TP;
  const int trial0 = (int)blockIdx.y * KB;
  const double T = Fl::period(A.tr, blockIdx.y);
  const unsigned P = (unsigned)A.y_t * (unsigned)A.x_t;
  const double spp = T / (double)P;
  const int l = l0 + lane;
  const bool lane_on = l < A.y_t;
  const unsigned mrow = (unsigned)min(l, A.y_t - 1) * (unsigned)A.x_t;
  const int pbeg = p0 + wave * PW;
  const int Wp = A.W | 1;
  // a pixel's running sum of one trial is (accr, acci); a flavour that sums real values leaves acci alone, and it is gone.  Two arrays,
  // not one of float2: the register allocation of the scan kernels, and with it their occupancy, follows this
  float accr[PW][KB], acci[PW][KB];
#pragma unroll
  for (int i = 0; i < PW; ++i)
#pragma unroll
    for (int j = 0; j < KB; ++j) accr[i][j] = acci[i][j] = 0.f;

  for (int f = 0; f < A.F; ++f) {
    const FramePos fp = frame_pos(A, T, f);
    if constexpr (Fl::line_weights) {
      if (tid < kFoldLines) lwts[f & 1][tid] = Fl::line_weight(A.tr, f, min(l0 + tid, A.y_t - 1), A.y_t);
    } else if constexpr (Fl::has_weights) {
      if (tid < KB) wts[f & 1][tid] = Fl::weight(A.tr, f, trial0 + tid);
    }
    if constexpr (STAGED) {
      if (tid < kFoldLines) {
        double d;
        kfirst[f & 1][tid] = fold_tap(fp, fold_s(fp, spp, (unsigned)min(l0 + tid, A.y_t - 1) * (unsigned)A.x_t + (unsigned)p0), d);
      }
    }
    if constexpr (STAGED || Fl::has_weights) __syncthreads();   // the tables are complete, and every wavefront has left the previous frame's walk
    if constexpr (STAGED) {
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
          if (base + (unsigned)u * NT < tot) smp[at[u]] = Fl::stage(z[u]);
      }
      __syncthreads();
    }
    if (lane_on) {
      float2 w[KB];
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        w[j] = make_float2(0.f, 0.f);
        if constexpr (Fl::line_weights) w[j] = lwts[f & 1][lane];
        else if constexpr (Fl::has_weights) w[j] = wts[f & 1][j];
      }
      const int rb = STAGED ? lane * Wp - kfirst[f & 1][lane] : 0;   // smp[rb + k]: sample k of this lane's line
      const double s0 = fold_s(fp, spp, mrow + (unsigned)pbeg);
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        const int p = pbeg + i;
        if (p < A.x_t) {
          double d;
          const int k = fold_tap(fp, i == 0 ? s0 : fma((double)i, spp, s0), d);
          Sample a, b;
          if constexpr (STAGED) {
            a = smp[rb + k];
            b = smp[rb + k + 1];
          } else {
            const unsigned ka = (unsigned)(fp.bi + (long long)k);
            const float2 za = ld_iq(A.iq, ka, A.fmt), zb = ld_iq(A.iq, ka + 1u, A.fmt);
            a = Fl::stage(za);
            b = Fl::stage(zb);
          }
          const Sample z = Fl::blend(a, b, d);
#pragma unroll
          for (int j = 0; j < KB; ++j) {
            float2 a = make_float2(accr[i][j], acci[i][j]);
            Fl::add(a, z, w[j]);
            accr[i][j] = a.x;
            acci[i][j] = a.y;
          }
        }
      }
    }
  }

  const float Ff = (float)A.F;
  if constexpr (!SCAN && !Fl::stacks) {
    if (lane_on) {
      const float alpha = A.alpha, beta = __fsub_rn(1.f, alpha);
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        const int p = pbeg + i;
        if (p < A.x_t) {
          float *o = A.state + (size_t)p * (size_t)A.y_t + (size_t)l;
          const float c = Fl::pixel(make_float2(accr[i][0], acci[i][0]), Ff);
          *o = alpha == 0.f ? c : __fadd_rn(__fmul_rn(alpha, *o), __fmul_rn(beta, c));
        }
      }
    }
  } else {
    double st[KB][NS];
#pragma unroll
    for (int j = 0; j < KB; ++j)
#pragma unroll
      for (int s = 0; s < NS; ++s) st[j][s] = 0.0;
    if (lane_on) {
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        if (pbeg + i < A.x_t) {
          if constexpr (SCAN) {
#pragma unroll
            for (int j = 0; j < KB; ++j) Fl::stat(st[j], make_float2(accr[i][j], acci[i][j]), Ff);
          } else {
            Fl::stack(A, st[0], make_float2(accr[i][0], acci[i][0]), Ff, (size_t)(pbeg + i) * (size_t)A.y_t + (size_t)l);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      for (int off = 32; off > 0; off >>= 1) {   // the same tree on every run
#pragma unroll
        for (int s = 0; s < NS; ++s) st[j][s] += __shfl_down(st[j][s], off);
      }
      if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) red[j][s][wave] = st[j][s];
      }
    }
    __syncthreads();
    if (tid < KB && Fl::live(A.tr, trial0 + tid)) {
      double *o = A.part + ((size_t)(trial0 + tid) * (size_t)gridDim.x + (size_t)blockIdx.x) * NS;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        double v = red[tid][s][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) v += red[tid][s][w];   // wave order
        o[s] = v;
      }
    }
  }
}

// one lane per trial: the tiles' partial statistics in tile order, then the flavour's score
template <class Fl>
__global__ __launch_bounds__(kFoldThreads) void k_fold_score(const double *__restrict__ part, unsigned tiles, int n_trials, double P,
                                                             double *__restrict__ score) {
  constexpr int NS = Fl::NS;
  struct alignas(8 * NS) Stat { double v[NS]; };   // NS == 2: one 16-byte load
  const int k = (int)(blockIdx.x * kFoldThreads + threadIdx.x);
  if (k >= n_trials) return;
  const Stat *q = reinterpret_cast<const Stat *>(part) + (size_t)k * tiles;
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  unsigned t = 0;
  for (; t + 8 <= tiles; t += 8) {   // eight tiles' loads in flight, added in tile order
    Stat v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = q[t + u];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int i = 0; i < NS; ++i) s[i] += v[u].v[i];
  }
  for (; t < tiles; ++t)
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] += q[t].v[i];
  score[k] = Fl::finish(s, P);
}

// ---------------------------------------------------------------- host
struct FoldCall {
  const void *iq;
  int iq_fmt;
  float scale;
  size_t n;
  double t0, T, dT;         // trial k folds at T + k * dT (the coherent fold: dT = 0)
  double kappa0, dkappa;    // the coherent fold: trial k turns frame f by -f * (kappa0 + k * dkappa) turns
  int n_trials, F, y_t, x_t;
  float alpha;
  float *state;    // fold (else null); a stacking flavour: the complex state, P (re, im) pairs
  double *score;   // scan (else null)
  bool scan;
  double phi = 0.0;        // a stacking flavour: the call's start phase in turns, its mode, and its optional outputs
  int mode = 0;
  float *mag = nullptr;
  double *info = nullptr;
  const double *track = nullptr;   // raster_ctrack.hip: (a_f, b_f) per frame in turns (the probe: may be null), and the probe's reference
  const float *zref = nullptr;
  double t_max() const { return T + (double)(n_trials - 1) * dT; }   // the largest trial period
};

struct FoldGeom {   // a launch's geometry
  bool staged;
  size_t tiles, lds;
  dim3 grid;
};

// everything the flavour's header (REFUSALS) refuses, before anything is enqueued or staged; device: the pointers are device pointers
template <class Fl>
int fold_check(tsdr_ctx *ctx, const char *fn, const FoldCall &c, bool device, IqFmt &f) {
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
  if (c.n_trials < 1 || c.n_trials > Fl::kMaxTrials)
    return set_err(ctx, TSDR_EINVAL, "%s: n_trials must be in [1, %d] (got %d)", fn, Fl::kMaxTrials, c.n_trials);
  if (int rc = Fl::refuse(ctx, fn, c)) return rc;
  if (!(c.t0 + (double)c.F * c.t_max() <= (double)c.n))
    return set_err(ctx, TSDR_EINVAL, "%s: t0 + n_frames*T = %.17g exceeds the %zu samples of the buffer", fn, c.t0 + (double)c.F * c.t_max(),
                   c.n);
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

// The staged/direct choice of a call, made on a 128-pixel line span at the largest trial (the headers' COST), and its tiles of 64 lines
// x tile_p or 16 pixels: fold_launch's geometry, which a flavour's refusals may ask for before anything is enqueued.
template <class Fl>
inline bool fold_staged(const FoldCall &c) {
  const double P = (double)c.y_t * (double)c.x_t;
  return std::ceil((double)kFoldTileP * (c.t_max() / P)) + 3.0 <= (double)Fl::kStageMax;
}
template <class Fl>
inline size_t fold_tiles(const FoldCall &c, bool staged) {
  const int TP = staged ? Fl::tile_p(c.scan) : kFoldDirectP;
  return ceil_div((size_t)c.y_t, kFoldLines) * ceil_div((size_t)c.x_t, (size_t)TP);
}

// the device form: checked arguments, F > 0.  W is the span of the kernel's own tile.
template <class Fl>
int fold_launch(tsdr_ctx *ctx, const FoldCall &c, const IqFmt &f) {
  const double P = (double)c.y_t * (double)c.x_t;
  FoldGeom g{};
  g.staged = fold_staged<Fl>(c);
  const int TP = g.staged ? Fl::tile_p(c.scan) : kFoldDirectP;
  FoldArgs<typename Fl::Trial> A{};
  A.iq = reinterpret_cast<const float *>(c.iq);
  A.fmt = f;
  A.n = (long long)c.n;
  A.t0 = c.t0;
  A.F = c.F; A.y_t = c.y_t; A.x_t = c.x_t;
  A.tiles_l = (int)ceil_div((size_t)c.y_t, kFoldLines);
  A.W = g.staged ? (int)(std::ceil((double)TP * (c.t_max() / P)) + 3.0) : 0;
  A.wmagic = g.staged ? (unsigned)((1ull << 32) / (unsigned long long)A.W + 1ull) : 0u;
  A.alpha = c.alpha;
  A.state = c.state;
  A.tr = Fl::trial(c);
  g.tiles = fold_tiles<Fl>(c, g.staged);
  if (g.tiles >= (1ull << 31)) return set_err(ctx, TSDR_EINVAL, "%s: %zu tiles exceed the grid", Fl::name, g.tiles);
  g.grid = dim3((unsigned)g.tiles, (unsigned)ceil_div((size_t)c.n_trials, (size_t)Fl::batch(c.scan)));
  g.lds = g.staged ? (size_t)kFoldLines * (size_t)(A.W | 1) * sizeof(typename Fl::Sample) : 0;
  if (c.scan) {
    A.part = (double *)ctx->scratch(Fl::kSlot, (size_t)c.n_trials * g.tiles * 8 * Fl::NS);
    if (!A.part) return TSDR_ENOMEM;
  }
  return Fl::launch(ctx, c, g, A);
}

// an entry point: the refusals, then the device form, or the host form around it (upload iq -- and the state if alpha != 0 --, launch,
// download the state or the scores, wait; best: the first maximum of a scan's scores)
template <class Fl>
int fold_entry(tsdr_ctx *ctx, const char *fn, const char *what, FoldCall c, bool device, int *best = nullptr) {
  IqFmt f;
  if (int rc = fold_check<Fl>(ctx, fn, c, device, f)) return rc;
  if (c.F == 0) return TSDR_OK;
  if (device) return fold_launch<Fl>(ctx, c, f);
  const size_t in_bytes = c.n * iq_bytes(f), out_bytes = c.scan ? (size_t)c.n_trials * 8 : (size_t)c.y_t * (size_t)c.x_t * 4;
  void *out = c.scan ? (void *)c.score : (void *)c.state;
  HostStage st(ctx);
  c.iq = st.in(WS_IN, c.iq, in_bytes);
  void *d_out = st.inout(WS_OUT, out, out_bytes, !c.scan && c.alpha != 0.f);
  if (c.scan) c.score = (double *)d_out;
  else c.state = (float *)d_out;
  if (int rc = st.run(what, [&] { return fold_launch<Fl>(ctx, c, f); })) return rc;
  if (c.scan && best) {
    const double *score = (const double *)out;
    *best = -1;
    for (int k = 0; k < c.n_trials; ++k)
      if (score[k] == score[k] && (*best < 0 || score[k] > score[*best])) *best = k;
  }
  return TSDR_OK;
}

}  // namespace tsdr
