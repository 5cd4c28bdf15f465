// raster_tune.hip -- the tuner of include/tempest_hip_tune.h: frequency shift by a 64-bit phase accumulator, real FIR low-pass,
// decimation.  y[j] = sum_i h[i] u[j D + i], u[m] = x[m] w[m].
//   k_tune       one workgroup per tile of `lanes * 4` outputs.  Phase 1: all 256 lanes mix the (nt - 1) D + L samples the tile's nt
//                outputs need (tune_u: from iq through ld_iq and the oscillator, or from hist in front of iq[0]) into LDS, sample s of
//                the tile at float2 index s + s / S, S = 4 D: a row of S samples per lane, padded by one, so that lane t's window
//                starts at t (S + 1) and the lanes of a wavefront, S samples apart, read 32 different banks (ds_read_b64: 64 banks
//                of 4 bytes, 32 lanes per cycle; S + 1 is odd).  Phase 2: lane t < lanes runs the chains of outputs 4 t .. 4 t + 3:
//                it reads sample k = 0 .. 3 D + L - 1 of its window ONCE and feeds it to chain r with tap i = k - r D where 0 <= i < L
//                -- every chain sees its taps in ascending order, whatever the tile.  k in [3 D, L) feeds all four chains with no
//                test; the head and the tail test per chain (uniform branches).  k is uniform, so the taps are scalar loads.
//   k_tune_hist  one workgroup behind it on the stream: entry q of the new history is a mixed sample of this call or an entry of the
//                old history further right; every lane reads, barrier, every lane writes: hist is updated in place.
// Both form u[m] through tune_u alone: the bits of a mixed sample do not depend on which kernel, tile or call made it.
#include "common.h"

namespace tsdr {
namespace {

constexpr int kTuneThreads = 256, kTuneR = 4, kTuneU = 8, kTuneHistThreads = 1024;
constexpr int kTuneLdsCap = 6144;   // float2 per workgroup (48 KiB): three workgroups per CU

struct TuneArgs {
  const float *iq;
  IqFmt fmt;
  long long n;                       // samples of iq
  unsigned long long m0, nu, phi;
  const float *taps;
  int L, D;
  long long r0;                      // j0 * D - m0: where the first output's window starts, relative to iq[0] (>= -n_hist)
  float *hist;                       // L - 1 float2, float-aligned; entry L - 1 + r is u[m0 + r], -n_hist <= r < 0
  float *out;
  unsigned long long n_out;
  int lanes;                         // lanes of a workgroup that make outputs: tune_lanes(L, D)
};

// lanes per workgroup: the tile's padded samples, lanes * (S + 1) + the L - D of the last window + its pads, fit kTuneLdsCap
inline int tune_lanes(int L, int D) {
  const int S = kTuneR * D, ext = L > D ? L - D : 0;
  const int lanes = (kTuneLdsCap - 2 - (ext * (S + 1) + S - 1) / S) / (S + 1);   // >= 20 over the accepted domain
  return lanes > kTuneThreads ? kTuneThreads : lanes;
}

// w = exp(2 pi i p / 2^64): the phase as a signed number of half turns in f64 (one rounding, 2^-53 relative), the f64 sincospi, each
// of the two rounded to f32.  p == 0: (1, 0) exactly.
__device__ inline float2 tune_w(unsigned long long p) {
  double s, c;
  sincospi((double)(long long)p * 0x1p-63, &s, &c);
  return make_float2((float)c, (float)s);
}

// u[m0 + r], -n_hist <= r < n: a sample of this call mixed, or the history's entry
__device__ inline float2 tune_u(const TuneArgs &A, long long r) {
  if (r < 0) {
    const float *h = A.hist + 2 * ((long long)(A.L - 1) + r);
    return make_float2(h[0], h[1]);
  }
  const float2 x = ld_iq(A.iq, (unsigned)r, A.fmt);
  const float2 w = tune_w(A.phi + A.nu * (A.m0 + (unsigned long long)r));
  return make_float2(__fsub_rn(__fmul_rn(x.x, w.x), __fmul_rn(x.y, w.y)), __fadd_rn(__fmul_rn(x.x, w.y), __fmul_rn(x.y, w.x)));
}

__global__ __launch_bounds__(kTuneThreads) void k_tune(TuneArgs A) {
  extern __shared__ float2 tune_lds[];
  const int L = A.L, D = A.D, S = kTuneR * D, TO = A.lanes * kTuneR;
  const unsigned long long jt = (unsigned long long)blockIdx.x * (unsigned)TO;   // the tile's first output, counted from j0
  const unsigned long long left = A.n_out - jt;
  const int nt = left < (unsigned long long)TO ? (int)left : TO;                  // outputs of this tile
  const long long base = A.r0 + (long long)(jt * (unsigned)D);                    // its first sample, relative to iq[0]
  const int NS = (nt - 1) * D + L;   // every one of them exists: the last output's window is complete
  {
    const int a = kTuneThreads / S, b = kTuneThreads % S;
    int q = (int)threadIdx.x / S, rem = (int)threadIdx.x % S;   // q = s / S, carried along
    for (int s = threadIdx.x; s < NS; s += kTuneThreads) {
      tune_lds[s + q] = tune_u(A, base + s);
      q += a;
      rem += b;
      if (rem >= S) { rem -= S; ++q; }
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t * kTuneR >= nt) return;   // (nt <= lanes * 4)
  const float2 *row = tune_lds + t * (S + 1);
  const float *__restrict__ taps = A.taps;
  float2 acc[kTuneR];
#pragma unroll
  for (int r = 0; r < kTuneR; ++r) acc[r] = make_float2(0.f, 0.f);
  const int span = (kTuneR - 1) * D + L;
  int k = 0, o = 0, nx = S;   // o = k + k / S: where sample k of the window lies in the row
  // one sample into the chains it belongs to, tested per chain: the head (k < 3 D) and the tail (k >= L)
  auto edge = [&](int k_end) {
    for (; k < k_end; ++k) {
      const float2 v = row[o];
#pragma unroll
      for (int r = 0; r < kTuneR; ++r) {
        const int i = k - r * D;
        if (i >= 0 && i < L) {
          const float h = taps[i];
          acc[r].x = __fmaf_rn(h, v.x, acc[r].x);
          acc[r].y = __fmaf_rn(h, v.y, acc[r].y);
        }
      }
      ++o;
      if (k + 1 == nx) { ++o; nx += S; }
    }
  };
  edge((kTuneR - 1) * D);
  // (kTuneR - 1) D <= k < L: all four chains, no test.  Batches of kTuneU samples: their LDS reads and tap loads are issued together,
  // one wait per batch; each chain still takes its samples in ascending order
  for (; k + kTuneU <= L; k += kTuneU) {
    float2 v[kTuneU];
    float h[kTuneU][kTuneR];
#pragma unroll
    for (int u = 0; u < kTuneU; ++u) {
      v[u] = row[o];
      ++o;
      if (k + u + 1 == nx) { ++o; nx += S; }
#pragma unroll
      for (int r = 0; r < kTuneR; ++r) h[u][r] = taps[k + u - r * D];
    }
#pragma unroll
    for (int u = 0; u < kTuneU; ++u)
#pragma unroll
      for (int r = 0; r < kTuneR; ++r) {
        acc[r].x = __fmaf_rn(h[u][r], v[u].x, acc[r].x);
        acc[r].y = __fmaf_rn(h[u][r], v[u].y, acc[r].y);
      }
  }
  for (; k < L; ++k) {   // the rest of them, one by one
    const float2 v = row[o];
#pragma unroll
    for (int r = 0; r < kTuneR; ++r) {
      const float h = taps[k - r * D];
      acc[r].x = __fmaf_rn(h, v.x, acc[r].x);
      acc[r].y = __fmaf_rn(h, v.y, acc[r].y);
    }
    ++o;
    if (k + 1 == nx) { ++o; nx += S; }
  }
  edge(span);
#pragma unroll
  for (int r = 0; r < kTuneR; ++r) {
    const int j = t * kTuneR + r;
    if (j < nt) {
      float *y = A.out + 2 * (jt + (unsigned)j);   // (float-aligned, no more)
      y[0] = acc[r].x;
      y[1] = acc[r].y;
    }
  }
}

// hist[q], H - keep <= q < H, <- u[m0 + n - (H - q)]: this call's sample, or the old entry n places to the right
__global__ __launch_bounds__(kTuneHistThreads) void k_tune_hist(TuneArgs A, int keep) {
  const int H = A.L - 1, q = threadIdx.x;
  const bool on = q >= H - keep && q < H;
  float2 v = make_float2(0.f, 0.f);
  if (on) v = tune_u(A, A.n - (long long)(H - q));
  __syncthreads();
  if (on) {
    A.hist[2 * q] = v.x;
    A.hist[2 * q + 1] = v.y;
  }
}

int tune_launch(tsdr_ctx *ctx, const TuneArgs &A, int n_hist) {
  if (A.n == 0) return TSDR_OK;   // nothing new: the history is what it was
  if (A.n_out) {
    const int S = kTuneR * A.D, TO = A.lanes * kTuneR;
    const size_t tiles = ceil_div((size_t)A.n_out, (size_t)TO);   // < 2^31: n_out <= n + L < 2^31 + 2^10
    const size_t ns = (size_t)(TO - 1) * A.D + A.L, lds = (ns + ns / S + 1) * sizeof(float2);
    TSDR_LAUNCH(ctx, "tune", k_tune, dim3((unsigned)tiles), dim3(kTuneThreads), lds, A);
  }
  const int H = A.L - 1;
  if (A.hist && H > 0) {
    const long long have = (long long)n_hist + A.n;
    TSDR_LAUNCH(ctx, "tune_hist", k_tune_hist, dim3(1), dim3(kTuneHistThreads), 0, A, have < H ? (int)have : H);
  }
  return TSDR_OK;
}

// an entry point: the refusals and *n_out, then the device form, or the host form around it
int tune_entry(tsdr_ctx *ctx, const char *fn, const char *what, const void *iq, int iq_fmt, float scale, size_t n, uint64_t m0,
               uint64_t nu_fix, uint64_t phi_fix, const float *taps, int n_taps, int decim, uint64_t j0, float *hist, int n_hist,
               float *out, size_t out_cap, size_t *n_out, bool device) {
  if (!ctx) return TSDR_EINVAL;
  if (!n_out) return set_err(ctx, TSDR_EINVAL, "%s: n_out is NULL", fn);
  if (!iq) return set_err(ctx, TSDR_EINVAL, "%s: iq is NULL", fn);
  if (!taps) return set_err(ctx, TSDR_EINVAL, "%s: taps is NULL", fn);
  if (!out) return set_err(ctx, TSDR_EINVAL, "%s: out is NULL", fn);
  if (n_taps < 1 || n_taps > TSDR_TUNE_TAPS_MAX)
    return set_err(ctx, TSDR_EINVAL, "%s: n_taps must be in [1, %d] (got %d)", fn, TSDR_TUNE_TAPS_MAX, n_taps);
  if (decim < 1 || decim > TSDR_TUNE_DECIM_MAX)
    return set_err(ctx, TSDR_EINVAL, "%s: decim must be in [1, %d] (got %d)", fn, TSDR_TUNE_DECIM_MAX, decim);
  if (n >= ((size_t)1 << 31)) return set_err(ctx, TSDR_EINVAL, "%s: n must be below 2^31 (got %zu)", fn, n);
  IqFmt f;
  if (device) {
    TSDR_IQ_ARG(ctx, fn, iq, iq_fmt, scale, f);
    TSDR_PTR_ALIGNED(ctx, fn, taps, 4);
    TSDR_PTR_ALIGNED(ctx, fn, hist, 4);
    TSDR_PTR_ALIGNED(ctx, fn, out, 4);
  } else {
    TSDR_IQ_FMT_ARG(ctx, fn, iq_fmt);
    f = IqFmt{iq_fmt, iq_fmt == TSDR_IQ_CF32 ? 1.0f : scale};
  }
  const uint64_t end = m0 + (uint64_t)n;
  if (end < m0) return set_err(ctx, TSDR_EINVAL, "%s: m0 + n must be below 2^64 (m0 %llu)", fn, (unsigned long long)m0);
  const int H = n_taps - 1;
  if (n_hist < 0 || n_hist > H || (uint64_t)n_hist > m0)
    return set_err(ctx, TSDR_EINVAL, "%s: n_hist must be in [0, n_taps - 1] and at most m0 (got %d)", fn, n_hist);
  if (n_hist > 0 && !hist) return set_err(ctx, TSDR_EINVAL, "%s: hist is NULL with n_hist %d", fn, n_hist);
  if ((unsigned __int128)j0 * (unsigned)decim < (unsigned __int128)(m0 - (uint64_t)n_hist))
    return set_err(ctx, TSDR_EINVAL, "%s: the window of j0 = %llu starts before the history (m0 %llu, n_hist %d)", fn,
                   (unsigned long long)j0, (unsigned long long)m0, n_hist);
  size_t cnt = 0;
  if (end >= (uint64_t)n_taps) {
    const uint64_t j1 = (end - (uint64_t)n_taps) / (uint64_t)decim;
    if (j1 >= j0) cnt = (size_t)(j1 - j0 + 1);
  }
  if (out_cap < cnt) return set_err(ctx, TSDR_EINVAL, "%s: out_cap %zu is below the %zu outputs of this call", fn, out_cap, cnt);
  *n_out = cnt;
  TuneArgs A;
  A.iq = (const float *)iq; A.fmt = f; A.n = (long long)n; A.m0 = m0; A.nu = nu_fix; A.phi = phi_fix;
  A.taps = taps; A.L = n_taps; A.D = decim;
  A.r0 = cnt ? (long long)(j0 * (uint64_t)decim - m0) : 0;   // (j0 D <= m0 + n here; the difference is in [-n_hist, n])
  A.hist = hist; A.out = out; A.n_out = cnt; A.lanes = tune_lanes(n_taps, decim);
  if (device) return tune_launch(ctx, A, n_hist);
  // host form.  WS_IN: iq; WS_OUT: out[0 .. n_out); WS_AUX: taps, then hist (up and down: entries the call leaves alone go round)
  HostStage st(ctx);
  const size_t tb = (size_t)n_taps * 4, hb = (size_t)H * 8;
  A.iq = (const float *)st.in(WS_IN, iq, n * iq_bytes(f));
  A.out = (float *)st.out(WS_OUT, out, cnt * 8);
  st.reserve(WS_AUX, ((tb + 7) & ~(size_t)7) + hb);
  A.taps = (const float *)st.in(WS_AUX, taps, tb);
  A.hist = (float *)st.inout(WS_AUX, hist, hb, true);   // absent or present
  return st.run(what, [&] { return tune_launch(ctx, A, n_hist); });
}

}  // namespace
}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_tune_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, uint64_t m0, uint64_t nu_fix, uint64_t phi_fix,
                   const float *taps, int n_taps, int decim, uint64_t j0, float *hist, int n_hist, float *out, size_t out_cap,
                   size_t *n_out) {
  return tune_entry(ctx, "tune_iq", __func__, iq, iq_fmt, scale, n, m0, nu_fix, phi_fix, taps, n_taps, decim, j0, hist, n_hist, out,
                    out_cap, n_out, true);
}

int tsdr_tune_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, uint64_t m0, uint64_t nu_fix, uint64_t phi_fix,
                 const float *taps, int n_taps, int decim, uint64_t j0, float *hist, int n_hist, float *out, size_t out_cap,
                 size_t *n_out) {
  return tune_entry(ctx, "tune_iq", __func__, iq, iq_fmt, scale, n, m0, nu_fix, phi_fix, taps, n_taps, decim, j0, hist, n_hist, out,
                    out_cap, n_out, false);
}

int tsdr_tune_tile(int n_taps, int decim) {
  if (n_taps < 1 || n_taps > TSDR_TUNE_TAPS_MAX || decim < 1 || decim > TSDR_TUNE_DECIM_MAX) return TSDR_EINVAL;
  return tune_lanes(n_taps, decim) * kTuneR;
}

}  // extern "C"
