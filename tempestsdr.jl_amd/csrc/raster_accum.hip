// raster_accum.hip -- frame averaging at the monitor's own resolution (include/tempest_hip_hires.h):
//
//   k_raster_accum          A = alpha*A + (1-alpha)*circshift(R_f, -r_f) over the y_t x x_t rasters of n frames, frames in order;
//                           one launch, one lane per output pixel, n*4P + 8P bytes
//   tsdr_frames_hires_iq_d  the frame loop in chunks of k frames: tsdr_frames_iq_d with the chunk's rasters in context
//                           workspace, then one k_raster_accum over them with the loop's own sync indices -- or, under the option
//                           "hires_refine", with those indices refined to the raster pixel (raster_register.hip)
//
// It cannot be part of the raster launch: a frame's shift is known only after vsync has seen its whole 600x800 image, and the
// IIR is a recurrence across frames.  So it is a second stage over rasters the first stage has written.
#include <algorithm>

#include "common.h"
#include "raster_shift.h"

using namespace tsdr;

namespace {

// Frames whose raster loads one lane has in flight before the recurrence runs over them in frame order (the addresses do not
// depend on the accumulator).  sync.hip:k_shift_iir, the same recurrence at 600x800, was latency-bound with one.
// Measured at 30 rasters of 2576x1125 with a random shift per frame, us per launch (371 MB): 2 frames 77.1, 4 frames 68.3
// (5.43 TB/s), 8 frames 71.1, 16 frames 88.7; non-temporal loads 75.5 with 4 frames (68.7 / 71.8 with 8: no gain); 512-thread
// workgroups 69.9.  tests/test_hires_gpu.py reads this constant and walks n around its multiples.
constexpr int kRasterAccumU = 4;
constexpr int kThreads = 256;
// frames whose shifts a workgroup resolves per pass (one frame per thread, into LDS); a multiple of kRasterAccumU
constexpr int kShiftTile = kThreads;
static_assert(kShiftTile % kRasterAccumU == 0, "a tile of resolved shifts holds whole batches of loads");

struct AccumArgs {
  const float *rasters;   // n frames, P floats apart
  const int *shifts;      // 2*n ints ([2f] = s_y, [2f+1] = s_x) or null
  float *state;
  int n, y_t, x_t, units, img_h, img_w;
  float alpha;
};

// SHIFTED: shifts given.  The (r_y, r_x) of a frame are the same for every pixel, and the rule above costs a 64-bit division:
// each workgroup resolves them once per frame -- thread t the frame f0 + t of a tile of kShiftTile frames -- into LDS, and the
// pixel loop reads them from there (a broadcast read per frame) and wraps with one conditional subtraction per axis.
template <bool SHIFTED>
__global__ __launch_bounds__(kThreads) void k_raster_accum(AccumArgs A) {
  __shared__ int2 sh[SHIFTED ? kShiftTile : 1];
  const float *__restrict__ rasters = A.rasters;
  const int *__restrict__ shifts = A.shifts;
  float *__restrict__ state = A.state;
  const int n = A.n, y_t = A.y_t, x_t = A.x_t;
  const unsigned P = (unsigned)y_t * (unsigned)x_t;                     // < 2^31 (checked on the host)
  const unsigned idx = blockIdx.x * (unsigned)kThreads + threadIdx.x;   // < P + kThreads: no wrap
  const bool live = idx < P;
  const int i = (int)(idx % (unsigned)y_t), j = (int)(idx / (unsigned)y_t);   // the lanes of a wave run along i (down a column)
  const float alpha = A.alpha, oma = __fsub_rn(1.0f, alpha);
  float acc = live ? state[idx] : 0.0f;
  auto src_of = [&](int u) -> unsigned {   // pixel offset inside its frame of what frame (tile start + u) contributes to (i, j)
    if (!SHIFTED) return idx;
    const int2 r = sh[u];
    int si = i + r.x; if (si >= y_t) si -= y_t;   // 0 <= r < size: one conditional subtraction
    int sj = j + r.y; if (sj >= x_t) sj -= x_t;
    return (unsigned)sj * (unsigned)y_t + (unsigned)si;
  };
  for (int f0 = 0; f0 < n; f0 += kShiftTile) {
    const int cnt = n - f0 < kShiftTile ? n - f0 : kShiftTile;
    if (SHIFTED) {
      if (f0) __syncthreads();   // the previous tile's shifts are still being read
      const int t = (int)threadIdx.x;
      if (t < cnt) {
        const size_t f = (size_t)f0 + (size_t)t;
        sh[t] = make_int2(resolve_shift(shifts[2 * f], y_t, A.units, A.img_h), resolve_shift(shifts[2 * f + 1], x_t, A.units, A.img_w));
      }
      __syncthreads();
    }
    if (!live) continue;   // (after the barriers: every thread of the workgroup reaches them)
    const float *__restrict__ base = rasters + (size_t)f0 * (size_t)P;
    int f = 0;
    for (; f + kRasterAccumU <= cnt; f += kRasterAccumU) {
      float v[kRasterAccumU];
#pragma unroll
      for (int u = 0; u < kRasterAccumU; ++u) v[u] = base[(size_t)(f + u) * (size_t)P + src_of(f + u)];
#pragma unroll
      for (int u = 0; u < kRasterAccumU; ++u) acc = __fadd_rn(__fmul_rn(alpha, acc), __fmul_rn(oma, v[u]));
    }
    for (; f < cnt; ++f) {
      const float v = base[(size_t)f * (size_t)P + src_of(f)];
      acc = __fadd_rn(__fmul_rn(alpha, acc), __fmul_rn(oma, v));
    }
  }
  if (live) state[idx] = acc;
}

// everything tempest_hip_hires.h (EDGE CASES) refuses, before anything is enqueued or staged
int accum_check(tsdr_ctx *ctx, const char *fn, const float *rasters, int n_frames, int y_t, int x_t, const int *shifts, int shift_units,
                int img_h, int img_w, const float *state) {
  if (int rc = raster_args_check(ctx, fn, rasters, n_frames, y_t, x_t, shifts, shift_units, img_h, img_w)) return rc;
  if (!state) return set_err(ctx, TSDR_EINVAL, "%s: state is NULL", fn);
  TSDR_PTR_ALIGNED(ctx, fn, state, 4);
  return TSDR_OK;
}

// checked arguments, n_frames > 0: the launch (exact grid: one lane per pixel)
int accum_launch(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const int *shifts, int shift_units, int img_h,
                 int img_w, float alpha, float *state) {
  const AccumArgs A{rasters, shifts, state, n_frames, y_t, x_t, shift_units, img_h, img_w, alpha};
  const unsigned grid = (unsigned)ceil_div((size_t)y_t * (size_t)x_t, (size_t)kThreads);
  if (shifts) TSDR_LAUNCH(ctx, "raster_accum", k_raster_accum<true>, dim3(grid), dim3(kThreads), 0, A);
  else TSDR_LAUNCH(ctx, "raster_accum", k_raster_accum<false>, dim3(grid), dim3(kThreads), 0, A);
  return TSDR_OK;
}

}  // namespace

int tsdr::raster_args_check(tsdr_ctx *ctx, const char *fn, const float *rasters, int n_frames, int y_t, int x_t, const int *shifts,
                            int shift_units, int img_h, int img_w) {
  if (!ctx) return TSDR_EINVAL;
  if (y_t <= 0 || x_t <= 0) return set_err(ctx, TSDR_EINVAL, "%s: y_t and x_t must be positive (got %d, %d)", fn, y_t, x_t);
  if (n_frames < 0) return set_err(ctx, TSDR_EINVAL, "%s: n_frames is negative (%d)", fn, n_frames);
  if ((size_t)y_t * (size_t)x_t >= (size_t)1 << 31) return set_err(ctx, TSDR_EINVAL, "%s: y_t * x_t must be below 2^31", fn);
  if (n_frames > 0 && !rasters) return set_err(ctx, TSDR_EINVAL, "%s: rasters is NULL", fn);
  if (shift_units != TSDR_SHIFT_RASTER && shift_units != TSDR_SHIFT_IMAGE)
    return set_err(ctx, TSDR_EINVAL, "%s: unknown shift_units %d", fn, shift_units);
  if (shift_units == TSDR_SHIFT_IMAGE && (img_h <= 0 || img_w <= 0))
    return set_err(ctx, TSDR_EINVAL, "%s: TSDR_SHIFT_IMAGE needs a positive img_h x img_w (got %d x %d)", fn, img_h, img_w);
  TSDR_PTR_ALIGNED(ctx, fn, rasters, 4);
  TSDR_PTR_ALIGNED(ctx, fn, shifts, 4);
  return TSDR_OK;
}

extern "C" {

int tsdr_raster_accum_d(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const int *shifts, int shift_units,
                        int img_h, int img_w, float alpha, float *state) {
  if (int rc = accum_check(ctx, "raster_accum", rasters, n_frames, y_t, x_t, shifts, shift_units, img_h, img_w, state)) return rc;
  if (n_frames == 0) return TSDR_OK;
  return accum_launch(ctx, rasters, n_frames, y_t, x_t, shifts, shift_units, img_h, img_w, alpha, state);
}

int tsdr_raster_accum(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const int *shifts, int shift_units,
                      int img_h, int img_w, float alpha, float *state) {
  if (int rc = accum_check(ctx, "raster_accum", rasters, n_frames, y_t, x_t, shifts, shift_units, img_h, img_w, state)) return rc;
  if (n_frames == 0) return TSDR_OK;
  const size_t P = (size_t)y_t * (size_t)x_t, n = (size_t)n_frames;
  HostStage st(ctx);
  const float *d_r = (const float *)st.in(WS_IN, rasters, n * P * 4);
  float *d_state = (float *)st.inout(WS_AUX, state, P * 4, true);
  const int *d_shifts = (const int *)st.in(WS_MISC, shifts, n * 8);
  return st.run(__func__, [&] { return accum_launch(ctx, d_r, n_frames, y_t, x_t, d_shifts, shift_units, img_h, img_w, alpha, d_state); });
}

int tsdr_frames_hires_iq_d(tsdr_ctx *ctx, tsdr_sync *sync, const void *iq, int iq_fmt, float scale, size_t nEch, size_t S, int y_t,
                           int x_t, float alpha, int do_align, float *imageOut_state, float *frames_out, float alpha_hires,
                           float *hires_state, int *sync_idx, int *n_frames) {
  // what the second stage refuses is refused before the first chunk runs (tsdr_frames_iq_d checks the rest, chunk by chunk)
  if (int rc = accum_check(ctx, "frames_hires", nullptr, 0, y_t, x_t, sync_idx, TSDR_SHIFT_IMAGE, TSDR_RENDER_H, TSDR_RENDER_W, hires_state))
    return rc;
  IqFmt fmt;
  TSDR_IQ_ARG(ctx, "frames_hires", iq, iq_fmt, scale, fmt);
  if (S == 0 || !imageOut_state || (nEch && !iq)) return TSDR_EINVAL;
  const size_t nb = nEch / S, P = (size_t)y_t * (size_t)x_t, npx = (size_t)TSDR_RENDER_H * TSDR_RENDER_W;
  ctx->hires_shifts_n = 0;   // (tsdr_frames_hires_shifts: nothing applied yet)
  if (nb == 0 || nb > (size_t)1 << 20)   // nothing to average: tsdr_frames_iq_d's own answer (pending submissions, n_frames = 0, refusals)
    return tsdr_frames_iq_d(ctx, sync, iq, iq_fmt, scale, nEch, S, y_t, x_t, alpha, do_align, imageOut_state, frames_out, nullptr,
                            sync_idx, n_frames);
  // Frames per chunk.  The default is the whole buffer in one chunk, because that is what was measured to be fastest: chunks
  // whose rasters stay at or under 192 MiB -- meant to let the second stage read from the 256 MiB Infinity Cache what the first
  // wrote -- cost 254.3 against 243.2 us per buffer at C2 (17 + 13 frames) and 932 against 696 us at C5 (six chunks of 5):
  // smaller image launches fill the machine worse and the state is re-read and re-written per chunk, and nothing came back
  // from the cache (profiles/hires_c2.json).  "hires_chunk_frames" = k bounds the workspace (k * 4P bytes) at that price.
  size_t k = ctx->opt_hires_chunk_frames > 0 ? (size_t)ctx->opt_hires_chunk_frames : nb;
  if (k > nb) k = nb;
  float *rasters = (float *)ctx->scratch(WS_HIRES, k * P * 4);
  int *idx = sync_idx;
  if (do_align && !idx) idx = (int *)ctx->scratch(WS_HIRES_IDX, nb * 8);
  // the shifts each frame is averaged with, in raster units, kept for tsdr_frames_hires_shifts; with "hires_refine" they are the
  // registration's (raster_register.hip) and what the accumulator consumes
  int *applied = do_align ? (int *)ctx->scratch(WS_HIRES_SHIFTS, nb * 8) : nullptr;
  if (!rasters || (do_align && (!idx || !applied))) return TSDR_ENOMEM;
  const int refine = do_align ? ctx->opt_hires_refine : 0;
  const int d_y = (int)std::min<long long>(((long long)refine * y_t + TSDR_RENDER_H - 1) / TSDR_RENDER_H, (y_t - 1) / 2);
  const int d_x = (int)std::min<long long>(((long long)refine * x_t + TSDR_RENDER_W - 1) / TSDR_RENDER_W, (x_t - 1) / 2);
  if (n_frames) *n_frames = 0;
  for (size_t f0 = 0; f0 < nb; f0 += k) {
    const size_t cnt = nb - f0 < k ? nb - f0 : k;
    int nf = 0;
    int rc = tsdr_frames_iq_d(ctx, sync, (const char *)iq + f0 * S * iq_bytes(fmt), iq_fmt, scale, cnt * S, S, y_t, x_t, alpha, do_align,
                              imageOut_state, frames_out ? frames_out + f0 * npx : nullptr, rasters, do_align ? idx + 2 * f0 : nullptr,
                              &nf);
    if (rc) return rc;
    if ((size_t)nf != cnt) return set_err(ctx, TSDR_EHIP, "frames_hires: a chunk of %zu frames produced %d", cnt, nf);
    if (refine) {   // registered to the pixel against the state as this chunk finds it, then averaged with those shifts
      rc = register_launch(ctx, rasters, nf, y_t, x_t, hires_state, idx + 2 * f0, TSDR_SHIFT_IMAGE, TSDR_RENDER_H, TSDR_RENDER_W, d_y, d_x,
                           applied + 2 * f0, nullptr);
      if (rc) return rc;
      rc = accum_launch(ctx, rasters, nf, y_t, x_t, applied + 2 * f0, TSDR_SHIFT_RASTER, 0, 0, alpha_hires, hires_state);
    } else {
      rc = accum_launch(ctx, rasters, nf, y_t, x_t, do_align ? idx + 2 * f0 : nullptr, TSDR_SHIFT_IMAGE, TSDR_RENDER_H, TSDR_RENDER_W,
                        alpha_hires, hires_state);
      if (!rc && do_align)
        rc = resolve_launch(ctx, nf, y_t, x_t, idx + 2 * f0, TSDR_SHIFT_IMAGE, TSDR_RENDER_H, TSDR_RENDER_W, applied + 2 * f0);
    }
    if (rc) return rc;
    if (do_align) ctx->hires_shifts_n += nf;
    if (n_frames) *n_frames += nf;
  }
  return TSDR_OK;
}

}  // extern "C"
