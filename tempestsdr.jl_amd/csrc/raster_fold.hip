// raster_fold.hip -- coherent frame folding at a fractional frame period (include/tempest_hip_fold.h): the mean of the F frames a
// buffer holds when they are sampled at t0 + f*T, IIR-averaged into a y_t x x_t state, and the period scan that scores the
// pictures folded at trial periods.
//
// The kernels, the refusals and the host forms are fold_engine.h's (shared with raster_cfold.hip); this file holds the envelope
// flavour: |IQ| is taken once per staged sample, a pixel has one f32 sum, a trial of the scan changes the period (one trial per
// blockIdx.y), and a trial's score is sum x^2 - (sum x)^2 / P of its means x.
#include "fold_engine.h"

namespace tsdr {
namespace {

static_assert((TSDR_FOLD_STAGE_MAX | 1) * kFoldLines * 4 + 4 * kFoldLines * 2 + 2 * 8 * kFoldTileWaves <= 65536,
              "staged span + first-sample table + partials fit 64 KiB of LDS");

struct Envelope {
  using Sample = float;
  struct Trial { double T0, dT; };   // the launch's trial blockIdx.y folds at T0 + blockIdx.y * dT
  static constexpr bool has_weights = false, stacks = false, line_weights = false;
  static constexpr int NS = 2, kMaxTrials = TSDR_FOLD_MAX_TRIALS, kStageMax = TSDR_FOLD_STAGE_MAX, kSlot = WS_FOLD;
  static constexpr const char *name = "fold";
  static int tile_p(bool) { return kFoldTileP; }
  static int batch(bool) { return 1; }

  __device__ static float stage(float2 z) { return abs_iq_rn(z.x, z.y); }
  __device__ static double period(const Trial &t, unsigned y) { return t.T0 + (double)y * t.dT; }
  __device__ static bool live(const Trial &, int) { return true; }
  __device__ static float blend(float a, float b, double d) { return fast_blend(a, b, d); }
  __device__ static void add(float2 &a, float z, float2) { a.x = __fadd_rn(a.x, z); }
  __device__ static float pixel(float2 a, float Ff) { return __fdiv_rn(a.x, Ff); }
  __device__ static void stat(double *s, float2 a, float Ff) {
    const double x = (double)__fdiv_rn(a.x, Ff);
    s[0] += x;
    s[1] += x * x;
  }
  __device__ static double finish(const double *s, double P) { return s[1] - s[0] * s[0] / P; }

  static int refuse(tsdr_ctx *ctx, const char *fn, const FoldCall &c) {
    if (!std::isfinite(c.T) || !std::isfinite(c.t0) || !std::isfinite(c.dT))
      return set_err(ctx, TSDR_EINVAL, "%s: the period, t0 and dT must be finite", fn);
    if (c.T < 2.0 || c.t0 < 0.0 || c.dT < 0.0)
      return set_err(ctx, TSDR_EINVAL, "%s: the period must be at least 2, t0 and dT not negative (got %g, %g, %g)", fn, c.T, c.t0, c.dT);
    return TSDR_OK;
  }
  static Trial trial(const FoldCall &c) { return Trial{c.T, c.dT}; }
  static int launch(tsdr_ctx *ctx, const FoldCall &c, const FoldGeom &g, const FoldArgs<Trial> &A) {
    const dim3 wg_tile(kFoldTileWaves * 64), wg_direct(kFoldDirectWaves * 64);
    if (!c.scan) {
      if (g.staged) TSDR_LAUNCH(ctx, "fold_tile", (k_fold_engine<Envelope, kFoldTileP, kFoldTileWaves, 1, true, false>), g.grid, wg_tile, g.lds, A);
      else TSDR_LAUNCH(ctx, "fold_direct", (k_fold_engine<Envelope, kFoldDirectP, kFoldDirectWaves, 1, false, false>), g.grid, wg_direct, 0, A);
      return TSDR_OK;
    }
    if (g.staged) TSDR_LAUNCH(ctx, "fold_scan_tile", (k_fold_engine<Envelope, kFoldTileP, kFoldTileWaves, 1, true, true>), g.grid, wg_tile, g.lds, A);
    else TSDR_LAUNCH(ctx, "fold_scan_direct", (k_fold_engine<Envelope, kFoldDirectP, kFoldDirectWaves, 1, false, true>), g.grid, wg_direct, 0, A);
    TSDR_LAUNCH(ctx, "fold_score", k_fold_score<Envelope>, dim3((unsigned)ceil_div((size_t)c.n_trials, kFoldThreads)), dim3(kFoldThreads), 0,
                (const double *)A.part, (unsigned)g.tiles, c.n_trials, (double)c.y_t * (double)c.x_t, c.score);
    return TSDR_OK;
  }
};

}  // namespace
}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_fold_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, int n_frames, int y_t, int x_t,
                   float alpha, float *state) {
  return fold_entry<Envelope>(ctx, "fold_iq", __func__,
                              {iq, iq_fmt, scale, n, t0, T, 0.0, 0.0, 0.0, 1, n_frames, y_t, x_t, alpha, state, nullptr, false}, true);
}

int tsdr_fold_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, int n_frames, int y_t, int x_t,
                 float alpha, float *state) {
  return fold_entry<Envelope>(ctx, "fold_iq", __func__,
                              {iq, iq_fmt, scale, n, t0, T, 0.0, 0.0, 0.0, 1, n_frames, y_t, x_t, alpha, state, nullptr, false}, false);
}

int tsdr_fold_scan_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T0, double dT, int n_trials,
                        int n_frames, int y_t, int x_t, double *score) {
  return fold_entry<Envelope>(ctx, "fold_scan_iq", __func__,
                              {iq, iq_fmt, scale, n, t0, T0, dT, 0.0, 0.0, n_trials, n_frames, y_t, x_t, 0.f, nullptr, score, true}, true);
}

int tsdr_fold_scan_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T0, double dT, int n_trials,
                      int n_frames, int y_t, int x_t, double *score, int *best) {
  return fold_entry<Envelope>(ctx, "fold_scan_iq", __func__,
                              {iq, iq_fmt, scale, n, t0, T0, dT, 0.0, 0.0, n_trials, n_frames, y_t, x_t, 0.f, nullptr, score, true}, false, best);
}

}  // extern "C"
