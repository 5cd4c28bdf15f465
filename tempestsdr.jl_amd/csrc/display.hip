// display.hip -- display export (include/tempest_hip_display.h): the ROI of n f32 pictures as bytes, stretched over a range that is
// given (FIXED), the ROI's finite minimum and maximum (MINMAX), or two percentiles of a 4096-bin histogram between them (PERCENTILE).
//
//   k_display_stats   one pass over the ROI: finite minimum and maximum per lane, per wave (shuffles), per workgroup (LDS), then
//                     at most two integer atomics per workgroup on the group's words (minimum and maximum as order-preserving
//                     integer keys: the result does not depend on the order of arrival).  A workgroup first READS the words and
//                     skips an atomic that cannot change them: atomics on one cache line take 25 - 40 ns each on this part, one
//                     after the other, and with three per 4096 pixels they were 80 of the pass's 92 us at 2250x4400.
//   k_display_hist    PERCENTILE only: a 4096-counter histogram per workgroup in LDS (16 KiB), its non-zero counters added to the
//                     group's 64-bit counters with integer atomics
//   k_display_pick    one workgroup per group: the range of the mode (prefix counts of the 4096 counters -- their total is N --,
//                     the two bins, their edges), kept in the scratch for the mapping pass and written to ranges_out
//   k_display_map     reads the ROI, writes bytes: a lane owns four consecutive rows of one column, chosen so that their four
//                     bytes are one aligned dword of `out` (any byte alignment, rh not a multiple of 4: a column of `out` starts
//                     anywhere); a column's head and tail are single byte stores
//
// A work item everywhere is a QUAD: four consecutive rows r .. r+3 of one ROI column, r = 4q - phase, rows outside [0, rh) masked.
// The statistics and histogram passes choose the phase that puts quads on 16-byte boundaries of the INPUT, the mapping pass the
// phase (per column) that puts them on 4-byte boundaries of the OUTPUT.  A whole quad whose address is 16-byte aligned is one
// 16-byte load, anything else up to four dword loads.  Every grid is exact (ceil_div); no floating-point atomics anywhere.
#include <algorithm>

#include "common.h"

using namespace tsdr;

namespace {

constexpr int kThreads = 256;
constexpr int kBins = TSDR_DISPLAY_BINS;
constexpr int kStatQuads = 16;   // quads per lane of k_display_stats (four at a time in flight): fewer workgroups, fewer atomics
constexpr int kHistQuads = 32;   // quads per lane of k_display_hist: a workgroup's 16 KiB of counters are cleared and flushed per 32768 pixels
constexpr int kMapQuads = 2;
static_assert(kBins % kThreads == 0, "k_display_pick: a lane owns kBins / kThreads consecutive counters");

// per group, cleared on the stream by every call
struct GroupStat {
  unsigned nmin_key;   // ~key of the finite minimum (0: no finite pixel yet), see fkey
  unsigned max_key;    // key of the finite maximum (0: none)
  float lo, hi;        // the range the mapping pass uses (k_display_pick)
  unsigned pad[4];
};
static_assert(sizeof(GroupStat) == 32, "scratch layout");

// order-preserving map of the finite floats onto unsigned integers (the two zeros are neighbours: -0 below +0); no finite value
// maps to 0 or to 0xffffffff
__device__ inline unsigned fkey(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float fkey_inv(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ inline bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct Roi {
  const float *images;
  size_t P;            // floats between pictures
  int h, i0, j0, rh, rw;
  int n, f0;           // pictures of the call; the first picture of this launch
  unsigned nq;         // quads per column
  unsigned bpi;        // workgroups per picture
  int shared;
};

// rows r .. r+3 of the column at `col` (its ROI row 0): ok[k] says whether row r+k is inside [0, rh); v[k] is loaded only then
__device__ inline void load_quad(const float *__restrict__ col, int r, int rh, float v[4], bool ok[4]) {
  if (r >= 0 && r + 3 < rh) {
    const float *p = col + r;
    if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
      const float4 q = *reinterpret_cast<const float4 *>(p);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
    ok[0] = ok[1] = ok[2] = ok[3] = true;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ok[k] = r + k >= 0 && r + k < rh;
      v[k] = ok[k] ? col[r + k] : 0.f;
    }
  }
}

// the workgroup's picture and its first item
__device__ inline void where(const Roi &A, int per_lane, size_t &f, unsigned &item0) {
  f = (size_t)A.f0 + blockIdx.x / A.bpi;
  item0 = (blockIdx.x % A.bpi) * (unsigned)(kThreads * per_lane);
}

__global__ __launch_bounds__(kThreads) void k_display_stats(Roi A, int phase, GroupStat *gs) {
  __shared__ unsigned s_min[kThreads / 64], s_max[kThreads / 64];
  size_t f;
  unsigned item0;
  where(A, kStatQuads, f, item0);
  const float *__restrict__ pic = A.images + f * A.P + (size_t)A.j0 * A.h + A.i0;
  const unsigned items = A.nq * (unsigned)A.rw;
  unsigned kmin = 0xffffffffu, kmax = 0;
  constexpr int kFlight = 4;
  for (int u0 = 0; u0 < kStatQuads; u0 += kFlight) {
    if (item0 + (unsigned)u0 * kThreads >= items) break;   // workgroup-uniform
    float v[kFlight][4];
    bool ok[kFlight][4];
#pragma unroll
    for (int u = 0; u < kFlight; ++u) {
      const unsigned t = item0 + (unsigned)(u0 + u) * kThreads + threadIdx.x;
      if (t < items) {
        const unsigned c = t / A.nq, q = t % A.nq;
        load_quad(pic + (size_t)c * A.h, (int)(4 * q) - phase, A.rh, v[u], ok[u]);
      } else {
        ok[u][0] = ok[u][1] = ok[u][2] = ok[u][3] = false;
      }
    }
#pragma unroll
    for (int u = 0; u < kFlight; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (ok[u][k] && finite_f(v[u][k])) {
          const unsigned key = fkey(v[u][k]);
          kmin = min(kmin, key);
          kmax = max(kmax, key);
        }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, m));
    kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, m));
  }
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_min[wave] = kmin; s_max[wave] = kmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) { kmin = min(kmin, s_min[w]); kmax = max(kmax, s_max[w]); }
    if (kmax) {   // a finite pixel: the words only ever grow, so one that already holds as much needs no atomic
      GroupStat *g = gs + (A.shared ? 0 : f);
      if (__hip_atomic_load(&g->nmin_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < ~kmin) atomicMax(&g->nmin_key, ~kmin);
      if (__hip_atomic_load(&g->max_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < kmax) atomicMax(&g->max_key, kmax);
    }
  }
}

// the histogram's frame of a group: mn and invw, or use == false when the contract falls back to (mn, mx)
struct HistFrame { float mn, mx, d, invw; bool use; };
__device__ inline HistFrame hist_frame(const GroupStat &g) {
  HistFrame F;
  const bool any = g.max_key != 0;
  F.mn = any ? fkey_inv(~g.nmin_key) : 0.f;
  F.mx = any ? fkey_inv(g.max_key) : 0.f;
  F.d = __fsub_rn(F.mx, F.mn);
  F.invw = __fdiv_rn((float)kBins, F.d);
  F.use = F.d > 0.f && finite_f(F.d) && finite_f(F.invw);
  return F;
}

// AGG: a wave whose active lanes all hold the same bin adds their number once (a near-constant picture otherwise puts every
// lane of every wave on one LDS address)
template <bool AGG>
__global__ __launch_bounds__(kThreads) void k_display_hist(Roi A, int phase, const GroupStat *gs, unsigned long long *hist) {
  __shared__ unsigned cnt[kBins];
  size_t f;
  unsigned item0;
  where(A, kHistQuads, f, item0);
  const size_t g = A.shared ? 0 : f;
  const HistFrame F = hist_frame(gs[g]);
  if (!F.use) return;   // (the same decision in every lane of the grid's workgroups of this group)
  for (int b = threadIdx.x; b < kBins; b += kThreads) cnt[b] = 0;
  __syncthreads();
  const float *__restrict__ pic = A.images + f * A.P + (size_t)A.j0 * A.h + A.i0;
  const unsigned items = A.nq * (unsigned)A.rw;
  constexpr int kFlight = 4;
  for (int u0 = 0; u0 < kHistQuads; u0 += kFlight) {
    if (item0 + (unsigned)u0 * kThreads >= items) break;   // workgroup-uniform
    float v[kFlight][4];
    bool ok[kFlight][4];
#pragma unroll
    for (int u = 0; u < kFlight; ++u) {
      const unsigned t = item0 + (unsigned)(u0 + u) * kThreads + threadIdx.x;
      if (t < items) {
        const unsigned c = t / A.nq, q = t % A.nq;
        load_quad(pic + (size_t)c * A.h, (int)(4 * q) - phase, A.rh, v[u], ok[u]);
      } else {
        ok[u][0] = ok[u][1] = ok[u][2] = ok[u][3] = false;
      }
    }
#pragma unroll
    for (int u = 0; u < kFlight; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = ok[u][k] && finite_f(v[u][k]);
        const int b = in ? min(kBins - 1, (int)floorf(__fmul_rn(__fsub_rn(v[u][k], F.mn), F.invw))) : 0;
        if (AGG) {
          const unsigned long long mask = __ballot(in);
          if (mask) {
            const int lead = __ffsll((long long)mask) - 1;
            const int b0 = __shfl(b, lead);
            if (__ballot(in && b != b0) == 0) {
              if ((int)(threadIdx.x & 63) == lead) atomicAdd(&cnt[b0], (unsigned)__popcll(mask));
            } else if (in) {
              atomicAdd(&cnt[b], 1u);
            }
          }
        } else if (in) {
          atomicAdd(&cnt[b], 1u);
        }
      }
  }
  __syncthreads();
  unsigned long long *hg = hist + g * (size_t)kBins;
  for (int b = threadIdx.x; b < kBins; b += kThreads) {
    const unsigned c = cnt[b];
    if (c) atomicAdd(&hg[b], (unsigned long long)c);
  }
}

struct PickArgs {
  GroupStat *gs;
  const unsigned long long *hist;
  float *ranges_out;
  int n, shared, mode;
  float lo, hi;
  double p_lo, p_hi;
};

// one workgroup per group
__global__ __launch_bounds__(kThreads) void k_display_pick(PickArgs A) {
  __shared__ unsigned long long s_wave[kThreads / 64];
  __shared__ int s_b[2];
  __shared__ float s_rng[2];
  const size_t g = blockIdx.x;
  const int t = (int)threadIdx.x;
  GroupStat &G = A.gs[g];
  float lo = A.lo, hi = A.hi;
  if (A.mode != TSDR_RANGE_FIXED) {
    const HistFrame F = hist_frame(G);
    lo = F.mn;
    hi = F.mx;
    if (A.mode == TSDR_RANGE_PERCENTILE && F.use) {   // (workgroup-uniform)
      constexpr int kPer = kBins / kThreads;
      const unsigned long long *hg = A.hist + g * (size_t)kBins;
      unsigned long long c[kPer], mine = 0;
#pragma unroll
      for (int k = 0; k < kPer; ++k) { c[k] = hg[t * kPer + k]; mine += c[k]; }
      // inclusive prefix of the lane totals: shuffles inside a wave, the four wave totals through LDS
      const int lane = t & 63, wave = t >> 6;
      unsigned long long incl = mine;
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        const unsigned long long o = __shfl_up(incl, m);
        if (lane >= m) incl += o;
      }
      if (lane == 63) s_wave[wave] = incl;
      if (t < 2) s_b[t] = kBins - 1;
      __syncthreads();
      unsigned long long before = 0, N = 0;   // N: the finite ROI pixels of the group, every one of them in a bin
#pragma unroll
      for (int w = 0; w < kThreads / 64; ++w) {
        if (w < wave) before += s_wave[w];
        N += s_wave[w];
      }
      const double nm1 = (double)(N - 1);
      const unsigned long long k_lo = (unsigned long long)floor(__dmul_rn(A.p_lo, nm1));
      const unsigned long long k_hi = (unsigned long long)ceil(__dmul_rn(A.p_hi, nm1));
      unsigned long long cum = before + incl - mine;
      int b_lo = kBins, b_hi = kBins;
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        cum += c[k];
        if (cum > k_lo && b_lo == kBins) b_lo = t * kPer + k;
        if (cum > k_hi && b_hi == kBins) b_hi = t * kPer + k;
      }
      if (b_lo < kBins) atomicMin(&s_b[0], b_lo);
      if (b_hi < kBins) atomicMin(&s_b[1], b_hi);
      __syncthreads();
      if (t == 0) {
        const float wd = __fdiv_rn(F.d, (float)kBins);
        const int e_lo = s_b[0], e_hi = s_b[1] + 1;
        s_rng[0] = e_lo == kBins ? F.mx : __fadd_rn(F.mn, __fmul_rn((float)e_lo, wd));
        s_rng[1] = e_hi == kBins ? F.mx : __fadd_rn(F.mn, __fmul_rn((float)e_hi, wd));
      }
      __syncthreads();
      lo = s_rng[0];
      hi = s_rng[1];
    }
  }
  if (t == 0) { G.lo = lo; G.hi = hi; }
  if (A.ranges_out) {
    if (A.shared) {
      for (size_t i = (size_t)t; i < (size_t)A.n; i += kThreads) { A.ranges_out[2 * i] = lo; A.ranges_out[2 * i + 1] = hi; }
    } else if (t == 0) {
      A.ranges_out[2 * g] = lo;
      A.ranges_out[2 * g + 1] = hi;
    }
  }
}

__device__ inline unsigned to_byte(float v, float lo, float s, bool zero, bool invert) {
  if (zero || v != v) return 0u;
  float q = __fmul_rn(__fsub_rn(v, lo), s);
  q = fminf(fmaxf(q, 0.f), 255.f);
  const unsigned b = (unsigned)rintf(q);
  return invert ? 255u - b : b;
}

// gs == null: the range is (lo, hi) of the arguments (FIXED without ranges_out: no other launch ran)
__global__ __launch_bounds__(kThreads) void k_display_map(Roi A, const GroupStat *gs, float lo, float hi, int invert, uint8_t *out) {
  size_t f;
  unsigned item0;
  where(A, kMapQuads, f, item0);
  if (gs) {
    const GroupStat &G = gs[A.shared ? 0 : f];
    lo = G.lo;
    hi = G.hi;
  }
  const float dd = __fsub_rn(hi, lo);
  const float s = __fdiv_rn(255.0f, dd);
  const bool zero = !(dd > 0.f) || !finite_f(dd) || !finite_f(s);
  const float *__restrict__ pic = A.images + f * A.P + (size_t)A.j0 * A.h + A.i0;
  const size_t R = (size_t)A.rh * (size_t)A.rw;
  uint8_t *__restrict__ opic = out + f * R;
  const unsigned ophase = (unsigned)(reinterpret_cast<uintptr_t>(opic) & 3u);
  const unsigned items = A.nq * (unsigned)A.rw;
  float v[kMapQuads][4];
  bool ok[kMapQuads][4];
  unsigned c[kMapQuads];
  int r[kMapQuads];
#pragma unroll
  for (int u = 0; u < kMapQuads; ++u) {
    const unsigned t = item0 + u * kThreads + threadIdx.x;
    ok[u][0] = ok[u][1] = ok[u][2] = ok[u][3] = false;
    c[u] = 0;
    r[u] = 0;
    if (t < items) {
      c[u] = t / A.nq;
      const unsigned q = t % A.nq;
      // the column's first byte sits at opic + c*rh: rows 4q - phase .. + 3 are one aligned dword of out
      const unsigned phase = (ophase + (unsigned)(((size_t)c[u] * (size_t)A.rh) & 3u)) & 3u;
      r[u] = (int)(4 * q) - (int)phase;
      load_quad(pic + (size_t)c[u] * A.h, r[u], A.rh, v[u], ok[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < kMapQuads; ++u) {
    unsigned b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = ok[u][k] ? to_byte(v[u][k], lo, s, zero, invert != 0) : 0u;
    uint8_t *o = opic + (size_t)c[u] * (size_t)A.rh + (ptrdiff_t)r[u];   // (formed only; dereferenced where ok)
    if (ok[u][0] && ok[u][3]) {
      *reinterpret_cast<unsigned *>(o) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (ok[u][k]) o[k] = (uint8_t)b[k];
    }
  }
}

struct Call {
  const float *images;
  int n, h, w, i0, j0, rh, rw, mode;
  float lo, hi;
  double p_lo, p_hi;
  int flags;
  uint8_t *out;
  float *ranges_out;
};

// everything tempest_hip_display.h (REFUSALS) refuses, before anything is enqueued or staged
int display_check(tsdr_ctx *ctx, const char *fn, const Call &c) {
  if (!ctx) return TSDR_EINVAL;
  if (c.n < 0) return set_err(ctx, TSDR_EINVAL, "%s: n_images must not be negative (got %d)", fn, c.n);
  if (c.n == 0) return TSDR_OK;
  if (!c.images) return set_err(ctx, TSDR_EINVAL, "%s: images is NULL", fn);
  if (!c.out && !c.ranges_out) return set_err(ctx, TSDR_EINVAL, "%s: out and ranges_out are both NULL", fn);
  if (c.h <= 0 || c.w <= 0 || c.rh <= 0 || c.rw <= 0)
    return set_err(ctx, TSDR_EINVAL, "%s: h, w, rh and rw must be positive (got %d, %d, %d, %d)", fn, c.h, c.w, c.rh, c.rw);
  if (c.i0 < 0 || c.j0 < 0 || (long long)c.i0 + c.rh > c.h || (long long)c.j0 + c.rw > c.w)
    return set_err(ctx, TSDR_EINVAL, "%s: the ROI (%d, %d, %d, %d) does not lie inside the %d x %d picture", fn, c.i0, c.j0, c.rh, c.rw, c.h, c.w);
  if ((long long)c.h * c.w >= (1ll << 31)) return set_err(ctx, TSDR_EINVAL, "%s: h*w must be below 2^31", fn);
  if (c.mode != TSDR_RANGE_FIXED && c.mode != TSDR_RANGE_MINMAX && c.mode != TSDR_RANGE_PERCENTILE)
    return set_err(ctx, TSDR_EINVAL, "%s: range_mode %d is not a TSDR_RANGE_* mode", fn, c.mode);
  if (c.flags & ~(TSDR_DISPLAY_INVERT | TSDR_DISPLAY_SHARED)) return set_err(ctx, TSDR_EINVAL, "%s: unknown flag bits in %d", fn, c.flags);
  if (c.mode == TSDR_RANGE_PERCENTILE && !(0.0 <= c.p_lo && c.p_lo <= c.p_hi && c.p_hi <= 1.0))
    return set_err(ctx, TSDR_EINVAL, "%s: the fractions must satisfy 0 <= p_lo <= p_hi <= 1 (got %g, %g)", fn, c.p_lo, c.p_hi);
  if (c.mode == TSDR_RANGE_FIXED && (c.lo != c.lo || c.hi != c.hi)) return set_err(ctx, TSDR_EINVAL, "%s: a FIXED bound is NaN", fn);
  TSDR_PTR_ALIGNED(ctx, fn, c.images, 4);
  TSDR_PTR_ALIGNED(ctx, fn, c.ranges_out, 4);
  return TSDR_OK;
}

// launches `body(roi)` over all pictures, as many per launch as keep the grid below 2^31 workgroups
template <typename F>
int for_launches(const Call &c, unsigned nq, int per_lane, int shared, F body) {
  Roi A{c.images, (size_t)c.h * (size_t)c.w, c.h, c.i0, c.j0, c.rh, c.rw, c.n, 0, nq, 0, shared};
  A.bpi = (unsigned)ceil_div((size_t)nq * (size_t)c.rw, (size_t)kThreads * per_lane);
  const size_t fmax = std::max<size_t>(1, 0x7fffffffull / A.bpi);
  for (size_t f0 = 0; f0 < (size_t)c.n; f0 += fmax) {
    A.f0 = (int)f0;
    const unsigned grid = (unsigned)(std::min(fmax, (size_t)c.n - f0) * A.bpi);
    if (int rc = body(A, grid)) return rc;
  }
  return TSDR_OK;
}

// the device form: checked arguments, n > 0
int display_launch(tsdr_ctx *ctx, const Call &c) {
  const int shared = (c.flags & TSDR_DISPLAY_SHARED) != 0;
  const size_t groups = shared ? 1 : (size_t)c.n;
  const bool stats = c.mode != TSDR_RANGE_FIXED, hist = c.mode == TSDR_RANGE_PERCENTILE;
  const bool pick = stats || c.ranges_out;
  GroupStat *gs = nullptr;
  unsigned long long *hg = nullptr;
  if (pick) {
    const size_t bytes = groups * sizeof(GroupStat) + (hist ? groups * (size_t)kBins * 8 : 0);
    gs = (GroupStat *)ctx->scratch(WS_DISPLAY, bytes);
    if (!gs) return TSDR_ENOMEM;
    hg = reinterpret_cast<unsigned long long *>(gs + groups);
    TSDR_HIP(ctx, hipMemsetAsync(gs, 0, bytes, ctx->launch_stream));
  }
  if (stats) {
    // the phase that puts quads on the input's 16-byte boundaries: the same for every column of every picture when h is a
    // multiple of 4 (then h*w is one too), none otherwise
    const uintptr_t first = reinterpret_cast<uintptr_t>(c.images + (size_t)c.j0 * c.h + c.i0);
    const int phase = c.h % 4 == 0 ? (int)((first >> 2) & 3u) : 0;
    const unsigned nq = (unsigned)ceil_div((size_t)c.rh + phase, 4);
    if (int rc = for_launches(c, nq, kStatQuads, shared, [&](const Roi &A, unsigned grid) {
          TSDR_LAUNCH(ctx, "display_stats", k_display_stats, dim3(grid), dim3(kThreads), 0, A, phase, gs);
          return (int)TSDR_OK;
        }))
      return rc;
    if (hist) {
      const bool agg = ctx->opt_display_hist_agg != 0;
      if (int rc = for_launches(c, nq, kHistQuads, shared, [&](const Roi &A, unsigned grid) {
            if (agg) TSDR_LAUNCH(ctx, "display_hist", k_display_hist<true>, dim3(grid), dim3(kThreads), 0, A, phase, gs, hg);
            else TSDR_LAUNCH(ctx, "display_hist", k_display_hist<false>, dim3(grid), dim3(kThreads), 0, A, phase, gs, hg);
            return (int)TSDR_OK;
          }))
        return rc;
    }
  }
  if (pick) {
    const PickArgs P{gs, hg, c.ranges_out, c.n, shared, c.mode, c.lo, c.hi, c.p_lo, c.p_hi};
    TSDR_LAUNCH(ctx, "display_pick", k_display_pick, dim3((unsigned)groups), dim3(kThreads), 0, P);
  }
  if (c.out) {
    const unsigned nq = (unsigned)ceil_div((size_t)c.rh + 3, 4);
    const int invert = (c.flags & TSDR_DISPLAY_INVERT) != 0;
    if (int rc = for_launches(c, nq, kMapQuads, shared, [&](const Roi &A, unsigned grid) {
          TSDR_LAUNCH(ctx, "display_map", k_display_map, dim3(grid), dim3(kThreads), 0, A, (const GroupStat *)(pick ? gs : nullptr), c.lo, c.hi,
                      invert, c.out);
          return (int)TSDR_OK;
        }))
      return rc;
  }
  return TSDR_OK;
}

}  // namespace

extern "C" {

int tsdr_display_u8_d(tsdr_ctx *ctx, const float *images, int n_images, int h, int w, int i0, int j0, int rh, int rw, int range_mode,
                      float lo, float hi, double p_lo, double p_hi, int flags, uint8_t *out, float *ranges_out) {
  const Call c{images, n_images, h, w, i0, j0, rh, rw, range_mode, lo, hi, p_lo, p_hi, flags, out, ranges_out};
  if (int rc = display_check(ctx, "display_u8", c)) return rc;
  if (n_images == 0) return TSDR_OK;
  return display_launch(ctx, c);
}

int tsdr_display_u8(tsdr_ctx *ctx, const float *images, int n_images, int h, int w, int i0, int j0, int rh, int rw, int range_mode, float lo,
                    float hi, double p_lo, double p_hi, int flags, uint8_t *out, float *ranges_out) {
  Call c{images, n_images, h, w, i0, j0, rh, rw, range_mode, lo, hi, p_lo, p_hi, flags, out, ranges_out};
  if (int rc = display_check(ctx, "display_u8", c)) return rc;
  if (n_images == 0) return TSDR_OK;
  const size_t n = (size_t)n_images, in_bytes = n * (size_t)h * (size_t)w * 4, R = (size_t)rh * (size_t)rw;
  HostStage st(ctx);
  c.images = (const float *)st.in(WS_IN, images, in_bytes);
  c.out = (uint8_t *)st.out(WS_OUT, out, n * R);
  c.ranges_out = (float *)st.out(WS_AUX, ranges_out, n * 8);
  return st.run(__func__, [&] { return display_launch(ctx, c); });
}

}  // extern "C"
