// raster_cfold.hip -- phase-coherent frame folding (include/tempest_hip_cfold.h): the F frames a buffer holds, sampled at t0 + f*T
// as COMPLEX samples, frame f turned by -f*kappa turns, summed, and the magnitude taken once; and the carrier scan that scores the
// energy of the pictures folded at trial kappas.
//
// The kernels, the refusals and the host forms are fold_engine.h's (shared with raster_fold.hip); this file holds the coherent
// flavour: float2 samples are staged as they are (odd pitch: a lane's 8-byte reads of consecutive lines fall on distinct bank pairs),
// a pixel has two f32 sums per trial, and a trial of the scan changes only the weights, so a scan workgroup samples z_f(m) ONCE per
// frame and accumulates w_{f,k} * z into the sums of a batch of kBatch = 8 trials (blockIdx.y): with the scan's 32-pixel tile that is
// 4 pixels per lane x 8 trials x 2 = 64 accumulator registers.  A trial's score is the energy sum |Z|^2 of its picture.
// The device arithmetic (weight, blend, sum, mean) is coherent_ops.h's, shared with raster_cstack.hip.
#include "coherent_ops.h"
#include "fold_engine.h"

namespace tsdr {
namespace {

constexpr int kScanP = 32;   // pixels per tile of the tiled scan (eight wavefronts, as the tiled fold)
constexpr int kBatch = 8;    // trials per workgroup of the scan
static_assert((TSDR_CFOLD_STAGE_MAX | 1) * kFoldLines * 8 + 4 * kFoldLines * 2 + 2 * 8 * kBatch + 8 * kBatch * kFoldTileWaves <= 65536,
              "staged span + first-sample table + weights + partials fit 64 KiB of LDS");

struct Coherent {
  using Sample = float2;
  struct Trial {
    double T;
    double kappa0, dkappa;   // trial k = blockIdx.y * KB + j turns frame f by -f * (kappa0 + k * dkappa) turns
    int n_trials;
  };
  static constexpr bool has_weights = true, stacks = false, line_weights = false;
  static constexpr int NS = 1, kMaxTrials = TSDR_CFOLD_MAX_TRIALS, kStageMax = TSDR_CFOLD_STAGE_MAX, kSlot = WS_CFOLD;
  static constexpr const char *name = "cfold";
  static int tile_p(bool scan) { return scan ? kScanP : kFoldTileP; }
  static int batch(bool scan) { return scan ? kBatch : 1; }

  __device__ static float2 stage(float2 z) { return z; }
  __device__ static double period(const Trial &t, unsigned) { return t.T; }
  __device__ static bool live(const Trial &t, int k) { return k < t.n_trials; }
  // w_f of tempest_hip_cfold.h (WEIGHT): x = fl64(f * kappa), r = x - floor(x), (f32(cospi(2r)), f32(-sinpi(2r)))
  __device__ static float2 weight(const Trial &t, int f, int k) {
    const double kappa = t.kappa0 + (double)k * t.dkappa;
    return coh_weight((double)f * kappa);
  }
  __device__ static float2 blend(float2 a, float2 b, double d) { return coh_blend(a, b, d); }
  __device__ static void add(float2 &a, float2 z, float2 w) { coh_add(a, z, w); }
  __device__ static float pixel(float2 a, float Ff) {
    const float2 z = coh_mean(a, Ff);
    return abs_iq_rn(z.x, z.y);
  }
  __device__ static void stat(double *s, float2 a, float Ff) {
    const float2 z = coh_mean(a, Ff);
    const double zr = (double)z.x, zi = (double)z.y;
    s[0] += zr * zr + zi * zi;
  }
  __device__ static double finish(const double *s, double) { return s[0]; }

  static int refuse(tsdr_ctx *ctx, const char *fn, const FoldCall &c) {
    if (!std::isfinite(c.T) || !std::isfinite(c.t0)) return set_err(ctx, TSDR_EINVAL, "%s: the period and t0 must be finite", fn);
    if (!std::isfinite(c.kappa0) || !std::isfinite(c.dkappa)) return set_err(ctx, TSDR_EINVAL, "%s: kappa and dkappa must be finite", fn);
    if (c.T < 2.0 || c.t0 < 0.0)
      return set_err(ctx, TSDR_EINVAL, "%s: the period must be at least 2 and t0 not negative (got %g, %g)", fn, c.T, c.t0);
    return TSDR_OK;
  }
  static Trial trial(const FoldCall &c) { return Trial{c.T, c.kappa0, c.dkappa, c.n_trials}; }
  static int launch(tsdr_ctx *ctx, const FoldCall &c, const FoldGeom &g, const FoldArgs<Trial> &A) {
    const dim3 wg_tile(kFoldTileWaves * 64), wg_direct(kFoldDirectWaves * 64);
    if (!c.scan) {
      if (g.staged) TSDR_LAUNCH(ctx, "cfold_tile", (k_fold_engine<Coherent, kFoldTileP, kFoldTileWaves, 1, true, false>), g.grid, wg_tile, g.lds, A);
      else TSDR_LAUNCH(ctx, "cfold_direct", (k_fold_engine<Coherent, kFoldDirectP, kFoldDirectWaves, 1, false, false>), g.grid, wg_direct, 0, A);
      return TSDR_OK;
    }
    if (g.staged)
      TSDR_LAUNCH(ctx, "cfold_scan_tile", (k_fold_engine<Coherent, kScanP, kFoldTileWaves, kBatch, true, true>), g.grid, wg_tile, g.lds, A);
    else
      TSDR_LAUNCH(ctx, "cfold_scan_direct", (k_fold_engine<Coherent, kFoldDirectP, kFoldDirectWaves, kBatch, false, true>), g.grid, wg_direct, 0, A);
    TSDR_LAUNCH(ctx, "cfold_score", k_fold_score<Coherent>, dim3((unsigned)ceil_div((size_t)c.n_trials, kFoldThreads)), dim3(kFoldThreads), 0,
                (const double *)A.part, (unsigned)g.tiles, c.n_trials, (double)c.y_t * (double)c.x_t, c.score);
    return TSDR_OK;
  }
};

}  // namespace
}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_cfold_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, int n_frames,
                    int y_t, int x_t, float alpha, float *state) {
  return fold_entry<Coherent>(ctx, "cfold_iq", __func__,
                              {iq, iq_fmt, scale, n, t0, T, 0.0, kappa, 0.0, 1, n_frames, y_t, x_t, alpha, state, nullptr, false}, true);
}

int tsdr_cfold_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa, int n_frames,
                  int y_t, int x_t, float alpha, float *state) {
  return fold_entry<Coherent>(ctx, "cfold_iq", __func__,
                              {iq, iq_fmt, scale, n, t0, T, 0.0, kappa, 0.0, 1, n_frames, y_t, x_t, alpha, state, nullptr, false}, false);
}

int tsdr_cfold_scan_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa0,
                         double dkappa, int n_trials, int n_frames, int y_t, int x_t, double *score) {
  return fold_entry<Coherent>(ctx, "cfold_scan_iq", __func__,
                              {iq, iq_fmt, scale, n, t0, T, 0.0, kappa0, dkappa, n_trials, n_frames, y_t, x_t, 0.f, nullptr, score, true}, true);
}

int tsdr_cfold_scan_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, double kappa0,
                       double dkappa, int n_trials, int n_frames, int y_t, int x_t, double *score, int *best) {
  return fold_entry<Coherent>(ctx, "cfold_scan_iq", __func__,
                              {iq, iq_fmt, scale, n, t0, T, 0.0, kappa0, dkappa, n_trials, n_frames, y_t, x_t, 0.f, nullptr, score, true}, false, best);
}

}  // extern "C"
