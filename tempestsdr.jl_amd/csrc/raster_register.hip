// raster_register.hip -- registration of full-size rasters to the raster pixel (include/tempest_hip_register.h):
//
//   k_profiles         column and row sums of n rasters (and of the reference picture) in f64: the one bandwidth-bound pass,
//                      n*4P bytes read; per-tile partial sums out
//   k_profile_finish   adds the partials in tile order: the profiles
//   k_register_pick    one workgroup per (frame, axis): flat test of the reference profile, the 2D+1 dot products in f64, the
//                      ordered choice, the refined shift
//   k_resolve_shifts   the coarse shifts alone, in raster units (what tsdr_frames_hires_shifts reports without the option)
//
// No floating-point atomics anywhere: a sum's order is fixed by the tiling, so a call repeats its bits (the contract's PROFILES
// and SCORES).  Every grid is exact (ceil_div): one workgroup per tile, one lane per element.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "raster_shift.h"

using namespace tsdr;

namespace {

constexpr int kThreads = 256;
// A workgroup of k_profiles owns one frame x one strip of kStripCols columns x one block of kThreads * V rows (V = 4 with 16-byte
// loads, 1 with dword loads); lanes run down a column.  The strip goes through LDS kSubCols columns at a time; a lane has up to that
// many loads in flight.  A wider strip means fewer row partials (P / kStripCols doubles per frame are written) and fewer workgroups.
constexpr int kStripCols = 64, kSubCols = 16;
constexpr int kLd = kThreads + 16;   // elements between the columns of the LDS tile: 16 mod 32, see the second phase
static_assert(kStripCols % kSubCols == 0 && kSubCols * 16 == kThreads, "the second phase's thread map");

struct ProfArgs {
  const float *rasters;   // frames 0 .. n-1, P floats apart
  const float *extra;     // frame n (the reference picture) or null
  double *colpart;        // [frame][row block][x_t]
  double *rowpart;        // [frame][strip][y_t]
  int n, f0;              // f0: the first frame of this launch
  int y_t, x_t;
  unsigned nrb, nstrips;
};

template <int V>
__global__ __launch_bounds__(kThreads) void k_profiles(ProfArgs A) {
  using Share = std::conditional_t<V == 1, float, double>;   // one row per lane: its share of a column is the f32 value itself
  __shared__ Share sh[kSubCols * kLd];
  const unsigned y_t = (unsigned)A.y_t, x_t = (unsigned)A.x_t;
  const unsigned per = A.nrb * A.nstrips;            // workgroups per frame (< 2^31, checked on the host)
  const unsigned rem = blockIdx.x % per;
  const unsigned strip = rem / A.nrb, rb = rem % A.nrb;
  const size_t f = (size_t)A.f0 + blockIdx.x / per;
  const size_t P = (size_t)y_t * x_t;
  const float *__restrict__ base = f < (size_t)A.n ? A.rasters + f * P : A.extra;
  const unsigned t = threadIdx.x;
  const unsigned i = rb * (unsigned)(kThreads * V) + t * V;   // < y_t + kThreads * V: no wrap
  const bool live = i < y_t;                                  // (V == 4: y_t is a multiple of 4, so rows i .. i+3 are all live)
  const unsigned j0 = strip * kStripCols;
  double racc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) racc[v] = 0.0;
  // columns a lane loads at a time: all of a pass with one row per lane -- they are then issued AHEAD, before the previous pass's
  // second phase -- and half a pass with four (16 float4 per lane and their f64 sums cost 216 VGPRs, two waves per SIMD; 8 cost 164, three)
  constexpr int kFlight = V == 1 ? kSubCols : kSubCols / 2;
  constexpr bool kAhead = kFlight == kSubCols;
  float val[kFlight][V];
  auto load = [&](unsigned c) {   // the lane's rows of columns j0 + c .. + kFlight - 1, zeros outside the raster
#pragma unroll
    for (int u = 0; u < kFlight; ++u) {
      const unsigned j = j0 + c + u;
      const bool in = live && j < x_t;
      if constexpr (V == 4) {
        const float4 q = in ? *reinterpret_cast<const float4 *>(base + (size_t)j * y_t + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        val[u][0] = q.x; val[u][1] = q.y; val[u][2] = q.z; val[u][3] = q.w;
      } else {
        val[u][0] = in ? base[(size_t)j * y_t + i] : 0.f;
      }
    }
  };
  if (kAhead) load(0);
  for (unsigned c0 = 0;;) {
    // first phase: lane t adds its rows' values to its row sums and leaves its share of each column in the tile
#pragma unroll
    for (int h = 0; h < kSubCols; h += kFlight) {
      if (!kAhead) load(c0 + h);
#pragma unroll
      for (int u = 0; u < kFlight; ++u) {
        double q = (double)val[u][0];
        racc[0] = __dadd_rn(racc[0], q);
#pragma unroll
        for (int v = 1; v < V; ++v) {
          const double d = (double)val[u][v];
          racc[v] = __dadd_rn(racc[v], d);
          q = __dadd_rn(q, d);
        }
        if constexpr (V == 1) sh[(h + u) * kLd + t] = val[u][0];
        else sh[(h + u) * kLd + t] = q;
      }
    }
    // the next columns' loads are in flight under the second phase and its barriers (the same decision in every lane)
    const unsigned next = c0 + kSubCols;
    const bool more = next < (unsigned)kStripCols && j0 + next < x_t;
    if (kAhead && more) load(next);
    __syncthreads();
    // second phase: 16 lanes per column, lane `seg` of them adds the shares of lanes seg, seg + 16, ... in that order; the 16
    // results are added pairwise across the lanes.  A half-wave reads two columns, kLd = 16 mod 32 elements apart: 32 distinct
    // banks (f32) or 8-byte bank pairs (f64).
    const unsigned cc = t >> 4, seg = t & 15;
    double p = 0.0;
#pragma unroll
    for (int k = 0; k < kThreads / 16; ++k) p = __dadd_rn(p, (double)sh[cc * kLd + k * 16 + seg]);
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) p = __dadd_rn(p, __shfl_xor(p, m));
    const unsigned j = j0 + c0 + cc;
    if (seg == 0 && j < x_t) A.colpart[(f * A.nrb + rb) * x_t + j] = p;
    if (!more) break;
    __syncthreads();   // the tile is rewritten
    c0 = next;
  }
  if (live) {
#pragma unroll
    for (int v = 0; v < V; ++v) A.rowpart[(f * A.nstrips + strip) * y_t + i + v] = racc[v];
  }
}

struct FinArgs {
  const double *colpart, *rowpart;
  double *col, *row;      // [frame][x_t], [frame][y_t]; either may be null
  size_t ncol, nrow;      // frames * x_t, frames * y_t
  int y_t, x_t;
  unsigned nrb, nstrips;
};

// one lane per profile element: its partials in tile order
__global__ __launch_bounds__(kThreads) void k_profile_finish(FinArgs A) {
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx < A.ncol) {
    if (!A.col) return;
    const size_t f = idx / (size_t)A.x_t, j = idx % (size_t)A.x_t;
    double s = 0.0;
#pragma unroll 8
    for (unsigned rb = 0; rb < A.nrb; ++rb) s = __dadd_rn(s, A.colpart[(f * A.nrb + rb) * (size_t)A.x_t + j]);
    A.col[idx] = s;
  } else if (idx - A.ncol < A.nrow) {
    if (!A.row) return;
    const size_t k = idx - A.ncol, f = k / (size_t)A.y_t, i = k % (size_t)A.y_t;
    double s = 0.0;
#pragma unroll 8
    for (unsigned st = 0; st < A.nstrips; ++st) s = __dadd_rn(s, A.rowpart[(f * A.nstrips + st) * (size_t)A.y_t + i]);
    A.row[k] = s;
  }
}

struct PickArgs {
  const double *colprof, *rowprof;   // [n (+1: the reference's)][x_t], [..][y_t]
  const int *shifts;                 // coarse shifts or null
  int *shifts_out;
  double *scores;                    // per frame: 2*d_y+1 then 2*d_x+1
  int n, has_ref, y_t, x_t, units, img_h, img_w, d_y, d_x;
};

// Workgroup (frame f, axis): a wave scores kCand candidates at a time (their loads are independent: four times the loads in flight
// of one), wave w the groups w, w + 4, ...: lane l the terms j = l, l + 64, ... in that order, the 64 partial sums pairwise across
// the lanes; then thread 0 makes the ordered choice.
constexpr int kCand = 4;
__global__ __launch_bounds__(kThreads) void k_register_pick(PickArgs A) {
  const size_t f = blockIdx.x >> 1;
  const int axis = (int)(blockIdx.x & 1);   // 0: y (row profile), 1: x (column profile)
  const int size = axis ? A.x_t : A.y_t, D = axis ? A.d_x : A.d_y, img = axis ? A.img_w : A.img_h;
  const double *prof = axis ? A.colprof : A.rowprof;
  const double *pf = prof + f * (size_t)size, *pr = prof + (size_t)A.n * (size_t)size;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  // flat: every element of the reference profile compares equal to element 0 (a NaN compares unequal: not flat)
  int self = 1;
  if (A.has_ref) {
    const double e0 = pr[0];
    int differs = 0;
    for (long long j = t; j < size; j += kThreads) differs |= !(pr[j] == e0);
    self = !__syncthreads_or(differs);
  }
  const int r0 = A.shifts ? resolve_shift(A.shifts[2 * f + axis], size, A.units, img) : 0;
  const int r00 = A.shifts ? resolve_shift(A.shifts[axis], size, A.units, img) : 0;   // frame 0's
  const long long ncand = 2ll * D + 1;
  double *sc = A.scores + f * (size_t)(2ll * A.d_y + 1 + 2ll * A.d_x + 1) + (axis ? (size_t)(2ll * A.d_y + 1) : 0);
  for (long long c0 = (long long)wave * kCand; c0 < ncand; c0 += (kThreads / 64) * kCand) {
    int off[kCand];   // (a candidate past the last one is computed like the others -- every index stays inside the profile -- and dropped)
    double s[kCand];
#pragma unroll
    for (int q = 0; q < kCand; ++q) {
      off[q] = mod_floor((long long)r0 + (c0 + q - D), size);
      s[q] = 0.0;
    }
#pragma unroll 8
    for (long long j = lane; j < size; j += 64) {
      long long m = j + r00;
      if (m >= size) m -= size;
      const double a = self ? prof[m] : pr[j];
#pragma unroll
      for (int q = 0; q < kCand; ++q) {
        long long k = j + off[q];
        if (k >= size) k -= size;
        s[q] = __dadd_rn(s[q], __dmul_rn(a, pf[k]));
      }
    }
#pragma unroll
    for (int q = 0; q < kCand; ++q) {
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) s[q] = __dadd_rn(s[q], __shfl_xor(s[q], m));
      if (lane == 0 && c0 + q < ncand) sc[c0 + q] = s[q];
    }
  }
  __syncthreads();   // (the scores are in global memory: written and read by this workgroup only)
  if (t == 0) {
    const volatile double *v = sc;
    double best = v[D];
    int bd = 0;
    for (int m = 1; m <= D; ++m) {   // 0, -1, +1, -2, +2, ...: replaced on a strict > only
      const double lo = v[D - m], hi = v[D + m];
      if (lo > best) { best = lo; bd = -m; }
      if (hi > best) { best = hi; bd = m; }
    }
    A.shifts_out[2 * f + axis] = mod_floor((long long)r0 + bd, size);
  }
}

__global__ __launch_bounds__(kThreads) void k_resolve_shifts(const int *shifts, int *out, int n, int y_t, int x_t, int units, int img_h,
                                                             int img_w) {
  const size_t f = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (f >= (size_t)n) return;
  out[2 * f] = resolve_shift(shifts[2 * f], y_t, units, img_h);
  out[2 * f + 1] = resolve_shift(shifts[2 * f + 1], x_t, units, img_w);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// rows per lane of k_profiles: 16-byte loads when every column of every frame starts on a 16-byte boundary
int rows_per_lane(const float *rasters, const float *extra, int y_t) { return y_t % 4 == 0 && aligned16(rasters) && aligned16(extra) ? 4 : 1; }

struct ProfPlan {
  int V;
  unsigned nrb, nstrips;
  size_t colpart, rowpart;   // doubles
};

ProfPlan prof_plan(const float *rasters, const float *extra, size_t frames, int y_t, int x_t) {
  ProfPlan p;
  p.V = rows_per_lane(rasters, extra, y_t);
  p.nrb = (unsigned)ceil_div((size_t)y_t, (size_t)kThreads * p.V);
  p.nstrips = (unsigned)ceil_div((size_t)x_t, (size_t)kStripCols);
  p.colpart = frames * p.nrb * (size_t)x_t;
  p.rowpart = frames * p.nstrips * (size_t)y_t;
  return p;
}

// the profiles of frames 0 .. n-1 of `rasters` and, when extra != null, of `extra` as frame n: col = [frames][x_t], row =
// [frames][y_t] (either may be null); checked arguments, n + (extra != null) > 0
int profiles_launch(tsdr_ctx *ctx, const float *rasters, int n, const float *extra, int y_t, int x_t, double *col, double *row) {
  const size_t frames = (size_t)n + (extra ? 1 : 0);
  const ProfPlan p = prof_plan(rasters, extra, frames, y_t, x_t);
  double *part = (double *)ctx->scratch(WS_REG_PART, (p.colpart + p.rowpart) * sizeof(double));
  if (!part) return TSDR_ENOMEM;
  const size_t per = (size_t)p.nrb * p.nstrips;   // <= ceil(P / 256) * ... < 2^31: nrb * nstrips <= (y_t/256 + 1) * (x_t/64 + 1)
  if (per > 0x7fffffffull) return set_err(ctx, TSDR_EINVAL, "raster profiles: %zu tiles per frame", per);
  const size_t fmax = std::max<size_t>(1, 0x7fffffffull / per);   // frames per launch: the grid stays below 2^31 workgroups
  for (size_t f0 = 0; f0 < frames; f0 += fmax) {
    const size_t cnt = std::min(fmax, frames - f0);
    const ProfArgs A{rasters, extra, part, part + p.colpart, n, (int)f0, y_t, x_t, p.nrb, p.nstrips};
    const unsigned grid = (unsigned)(per * cnt);
    if (p.V == 4) TSDR_LAUNCH(ctx, "raster_profiles", k_profiles<4>, dim3(grid), dim3(kThreads), 0, A);
    else TSDR_LAUNCH(ctx, "raster_profiles", k_profiles<1>, dim3(grid), dim3(kThreads), 0, A);
  }
  const FinArgs F{part, part + p.colpart, col, row, frames * (size_t)x_t, frames * (size_t)y_t, y_t, x_t, p.nrb, p.nstrips};
  const size_t fgrid = ceil_div(F.ncol + F.nrow, (size_t)kThreads);
  if (fgrid > 0x7fffffffull) return set_err(ctx, TSDR_EINVAL, "raster profiles: %zu profile elements", F.ncol + F.nrow);
  TSDR_LAUNCH(ctx, "raster_profile_sum", k_profile_finish, dim3((unsigned)fgrid), dim3(kThreads), 0, F);
  return TSDR_OK;
}

// everything tempest_hip_register.h (REFUSALS) refuses, before anything is enqueued or staged
int register_check(tsdr_ctx *ctx, const char *fn, const float *rasters, int n_frames, int y_t, int x_t, const float *ref, const int *shifts,
                   int shift_units, int img_h, int img_w, int d_y, int d_x, const int *shifts_out, const double *scores) {
  if (int rc = raster_args_check(ctx, fn, rasters, n_frames, y_t, x_t, shifts, shift_units, img_h, img_w)) return rc;
  if (d_y < 0 || d_x < 0) return set_err(ctx, TSDR_EINVAL, "%s: d_y and d_x must not be negative (got %d, %d)", fn, d_y, d_x);
  if (2ll * d_y + 1 > y_t || 2ll * d_x + 1 > x_t)
    return set_err(ctx, TSDR_EINVAL, "%s: 2*d + 1 candidates must be distinct shifts (d_y %d of %d lines, d_x %d of %d pixels)", fn, d_y, y_t,
                   d_x, x_t);
  if (n_frames > 0 && !shifts_out) return set_err(ctx, TSDR_EINVAL, "%s: shifts_out is NULL", fn);
  TSDR_PTR_ALIGNED(ctx, fn, ref, 4);
  TSDR_PTR_ALIGNED(ctx, fn, shifts_out, 4);
  TSDR_PTR_ALIGNED(ctx, fn, scores, 8);
  return TSDR_OK;
}

size_t scores_per_frame(int d_y, int d_x) { return (size_t)(2ll * d_y + 1) + (size_t)(2ll * d_x + 1); }

}  // namespace

int tsdr::register_launch(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const float *ref, const int *shifts,
                          int shift_units, int img_h, int img_w, int d_y, int d_x, int *shifts_out, double *scores) {
  const size_t frames = (size_t)n_frames + (ref ? 1 : 0);
  double *prof = (double *)ctx->scratch(WS_REG_PROF, frames * ((size_t)x_t + (size_t)y_t) * sizeof(double));
  if (!prof) return TSDR_ENOMEM;
  if (!scores) scores = (double *)ctx->scratch(WS_REG_SCORES, (size_t)n_frames * scores_per_frame(d_y, d_x) * sizeof(double));
  if (!scores) return TSDR_ENOMEM;
  double *colprof = prof, *rowprof = prof + frames * (size_t)x_t;
  if (int rc = profiles_launch(ctx, rasters, n_frames, ref, y_t, x_t, colprof, rowprof)) return rc;
  const PickArgs A{colprof, rowprof, shifts, shifts_out, scores, n_frames, ref ? 1 : 0, y_t, x_t, shift_units, img_h, img_w, d_y, d_x};
  TSDR_LAUNCH(ctx, "raster_register", k_register_pick, dim3(2u * (unsigned)n_frames), dim3(kThreads), 0, A);
  return TSDR_OK;
}

int tsdr::resolve_launch(tsdr_ctx *ctx, int n_frames, int y_t, int x_t, const int *shifts, int shift_units, int img_h, int img_w,
                         int *shifts_out) {
  const unsigned grid = (unsigned)ceil_div((size_t)n_frames, (size_t)kThreads);
  TSDR_LAUNCH(ctx, "raster_shifts", k_resolve_shifts, dim3(grid), dim3(kThreads), 0, shifts, shifts_out, n_frames, y_t, x_t, shift_units,
              img_h, img_w);
  return TSDR_OK;
}

extern "C" {

int tsdr_raster_profiles_d(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, double *col, double *row) {
  if (int rc = raster_args_check(ctx, "raster_profiles", rasters, n_frames, y_t, x_t, nullptr, TSDR_SHIFT_RASTER, 0, 0)) return rc;
  TSDR_PTR_ALIGNED(ctx, "raster_profiles", col, 8);
  TSDR_PTR_ALIGNED(ctx, "raster_profiles", row, 8);
  if (n_frames == 0 || (!col && !row)) return TSDR_OK;
  return profiles_launch(ctx, rasters, n_frames, nullptr, y_t, x_t, col, row);
}

int tsdr_raster_register_d(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const float *ref, const int *shifts,
                           int shift_units, int img_h, int img_w, int d_y, int d_x, int *shifts_out, double *scores) {
  if (int rc = register_check(ctx, "raster_register", rasters, n_frames, y_t, x_t, ref, shifts, shift_units, img_h, img_w, d_y, d_x,
                              shifts_out, scores))
    return rc;
  if (n_frames == 0) return TSDR_OK;
  if (n_frames > 0x3fffffff) return set_err(ctx, TSDR_EINVAL, "raster_register: n_frames must be below 2^30");
  return register_launch(ctx, rasters, n_frames, y_t, x_t, ref, shifts, shift_units, img_h, img_w, d_y, d_x, shifts_out, scores);
}

int tsdr_raster_register(tsdr_ctx *ctx, const float *rasters, int n_frames, int y_t, int x_t, const float *ref, const int *shifts,
                         int shift_units, int img_h, int img_w, int d_y, int d_x, int *shifts_out, double *scores) {
  if (int rc = register_check(ctx, "raster_register", rasters, n_frames, y_t, x_t, ref, shifts, shift_units, img_h, img_w, d_y, d_x,
                              shifts_out, scores))
    return rc;
  if (n_frames == 0) return TSDR_OK;
  if (n_frames > 0x3fffffff) return set_err(ctx, TSDR_EINVAL, "raster_register: n_frames must be below 2^30");
  const size_t P = (size_t)y_t * (size_t)x_t, n = (size_t)n_frames, sbytes = n * scores_per_frame(d_y, d_x) * sizeof(double);
  HostStage st(ctx);
  const float *d_r = (const float *)st.in(WS_IN, rasters, n * P * 4);
  const float *d_ref = (const float *)st.in(WS_AUX, ref, P * 4);
  const int *d_shifts = (const int *)st.in(WS_MISC, shifts, n * 8);
  char *d_out = (char *)st.reserve(WS_OUT, n * 8 + sbytes);   // shifts_out (n * 8 bytes), then the scores: the device form
  (void)st.out(WS_OUT, shifts_out, n * 8);                    // always writes both
  (void)st.out(WS_OUT, scores, sbytes);
  return st.run(__func__, [&] {
    return register_launch(ctx, d_r, n_frames, y_t, x_t, d_ref, d_shifts, shift_units, img_h, img_w, d_y, d_x, (int *)d_out, (double *)(d_out + n * 8));
  });
}

int tsdr_frames_hires_shifts(tsdr_ctx *ctx, int max_frames, int *shifts, int *n_frames) {
  if (!ctx || max_frames < 0 || (max_frames && !shifts)) return TSDR_EINVAL;
  const tsdr_ctx::Buf &b = ctx->ws[WS_HIRES_SHIFTS];
  const int F = b.p && (size_t)ctx->hires_shifts_n * 8 <= b.cap ? ctx->hires_shifts_n : 0;
  if (n_frames) *n_frames = F;
  const int nf = F < max_frames ? F : max_frames;
  return read_back(ctx, true, shifts, b.p, (size_t)nf * 8, __func__);   // (no frames: the drain and the wait alone)
}

}  // extern "C"
