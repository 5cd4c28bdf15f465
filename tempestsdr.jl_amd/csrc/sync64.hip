// sync64.hip -- FrameSynchronisation.jl's SyncXY{Float64} / vsync / fill_beta! (:25-112) on a Float64 image.
// The same operation ORDER as the f32 kernels and the oracle's "summation orders" comment, in double:
//   * column sums  sum(image;dims=1): 64-row blocks, each accumulated top to bottom from 0.0, block sums added in order;
//   * row sums     sum(image;dims=2): strictly left to right, starting from 0.0 + 0.0;
//   * the 5-tap FIR: DSP.jl's transposed-direct-form muladd chain, written as explicit fma() (the build is -ffp-contract=off;
//     this is the one place of the f64 path that fuses);
//   * Sigma = sum(c_v): lane m accumulates c_v[m], c_v[m+64], ... from 0.0, the 64 partials folded by the tree 32, 16, .., 1;
//   * beta = ((S - s)/(2(n-w)) + s/(2w))^2 with correctly rounded divisions, the running blank sum s as the reference's
//     sequential recurrence over w;
//   * findmax: the first maximum in column-major order, NaN maximal; only its column is used (:66, :76).  With the option
//     "vsync_blank_dark" findmin instead (:51-53): the first minimum, NaN minimal -- the DARK instantiations below.
// As in tsdr_vsync, s_y is read from beta_y BEFORE this call refills it (:66): the first call after create / reset returns 1.
// The taps exp(-2k^2/25)/sum are computed on the host in f64 and kept in f64 (:124-129).
// Not a streaming path: one projection launch per axis, one FIR launch, one beta launch for both axes (a thread per centre
// walks its widths), one launch that picks the two columns.
#include <cmath>

#include "common.h"
#include "sync_state.h"

namespace tsdr {

struct Best64 { double v; int c; int pad; };  // a workgroup's first maximum (DARK: minimum): value, 1-based column

// a beats b: NaN before everything, then the larger (DARK: smaller) value, ties (and two NaNs) to the smaller column
template <bool DARK>
__device__ inline bool beats64(double av, int ac, double bv, int bc) {
  const bool an = isnan(av), bn = isnan(bv);
  if (an != bn) return an;
  if (!an && av != bv) return DARK ? av < bv : av > bv;
  return ac < bc;
}

// c_v: one workgroup of 64 lanes per 64 columns; each 64 x 64 block is staged through LDS with coalesced column reads and
// summed by its column's lane in row order
__global__ __launch_bounds__(64) void k_colsum64(const double *__restrict__ img, int y_t, int x_t, double *__restrict__ cv) {
  __shared__ double tile[64][65];  // [column][row]
  const int t = threadIdx.x, c0 = blockIdx.x * 64;
  double tot = 0.0;
  for (int r0 = 0; r0 < y_t; r0 += 64) {
    for (int j = 0; j < 64; ++j)
      if (c0 + j < x_t && r0 + t < y_t) tile[j][t] = img[(size_t)(c0 + j) * y_t + r0 + t];
    __syncthreads();
    double a = 0.0;
    const int rn = min(64, y_t - r0);
    for (int k = 0; k < rn; ++k) a = __dadd_rn(a, tile[t][k]);
    tot = r0 == 0 ? a : __dadd_rn(tot, a);
    __syncthreads();
  }
  if (c0 + t < x_t) cv[c0 + t] = tot;
}

// c_h: a lane per row, the columns strictly left to right (the loads run ahead of the add chain)
__global__ __launch_bounds__(64) void k_rowsum64(const double *__restrict__ img, int y_t, int x_t, double *__restrict__ ch) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= y_t) return;
  double acc = __dadd_rn(0.0, 0.0);
  int c = 0;
  for (; c + 8 <= x_t; c += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = img[(size_t)(c + u) * y_t + r];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = __dadd_rn(acc, v[u]);
  }
  for (; c < x_t; ++c) acc = __dadd_rn(acc, img[(size_t)c * y_t + r]);
  ch[r] = acc;
}

struct Taps64 { double h[5]; };

// y[i] = fma(x[i],h0, fma(x[i-1],h1, fma(x[i-2],h2, fma(x[i-3],h3, h4*x[i-4]))))  (x[<0] = 0): the transposed-direct-form
// chain of DSP.jl's filt with zero initial state, unrolled per output.  Both axes in one launch: [0, nx) then [nx, nx+ny).
__device__ inline double fir64_at(const double *x, int i, const Taps64 &T) {
  const double x4 = i >= 4 ? x[i - 4] : 0.0, x3 = i >= 3 ? x[i - 3] : 0.0, x2 = i >= 2 ? x[i - 2] : 0.0, x1 = i >= 1 ? x[i - 1] : 0.0;
  double s = __dmul_rn(T.h[4], x4);
  s = fma(x3, T.h[3], s);
  s = fma(x2, T.h[2], s);
  s = fma(x1, T.h[1], s);
  return fma(x[i], T.h[0], s);
}
__global__ __launch_bounds__(256) void k_fir64(const double *__restrict__ xa, int na, double *__restrict__ ya, const double *__restrict__ xb,
                                               int nb, double *__restrict__ yb, Taps64 T) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < na) ya[g] = fir64_at(xa, g, T);
  else if (g < na + nb) yb[g - na] = fir64_at(xb, g - na, T);
}

struct Beta64Axis {
  const double *cv;  // filtered projection, n values
  int n, w_min, w_max;
  double *beta;      // (w_max - w_min + 1) x n, column-major
  Best64 *blk;       // one record per workgroup
};
struct Beta64Args { Beta64Axis ax[2]; };

__device__ inline int mod_idx64(int k1, int n) { int m = (k1 - 1) % n; if (m < 0) m += n; return m; }

// fill_beta! for one axis per blockIdx.y: a lane per centre c; every wavefront forms Sigma in sum64 order itself
template <bool DARK>
__global__ __launch_bounds__(256) void k_beta64(Beta64Args A) {
  const Beta64Axis &X = A.ax[blockIdx.y];
  const int n = X.n, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if ((int)(blockIdx.x * blockDim.x) >= n) return;   // (the other axis needs more workgroups)
  double p = 0.0;
  for (int i = lane; i < n; i += 64) p = __dadd_rn(p, X.cv[i]);
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(p, off, 64);
    if (lane < off) p = __dadd_rn(p, o);
  }
  const double S = __shfl(p, 0, 64);
  const int c = blockIdx.x * blockDim.x + threadIdx.x + 1;  // 1-based centre
  const int W = X.w_max - X.w_min + 1;
  double bv = 0.0;
  int bc = 0x7fffffff;
  if (c <= n) {
    double acc = 0.0;  // averagePixel(c_v, c, w_min - 1, n)
    for (int k = c - (X.w_min - 1); k <= c + (X.w_min - 1); ++k) acc = __dadd_rn(acc, X.cv[mod_idx64(k, n)]);
    double s = __dmul_rn(2.0, acc);
    double *col = X.beta + (size_t)(c - 1) * W;
    bool have = false;
    for (int w = X.w_min, cnt = 0; w <= X.w_max; ++w, ++cnt) {
      s = __dadd_rn(s, __dmul_rn(2.0, X.cv[mod_idx64(c - w, n)]));
      s = __dadd_rn(s, __dmul_rn(2.0, X.cv[mod_idx64(c + w, n)]));
      const double v = __dadd_rn(__ddiv_rn(__dsub_rn(S, s), (double)(2 * (n - w))), __ddiv_rn(s, (double)(2 * w)));
      const double b = __dmul_rn(v, v);
      col[cnt] = b;
      if (!have || (!isnan(bv) && (isnan(b) || (DARK ? b < bv : b > bv)))) { bv = b; have = true; }
    }
    bc = c;
  }
  // first maximum (DARK: minimum) of the workgroup: wavefront shuffles, then the four wavefronts in order through LDS
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(bv, off, 64);
    const int oc = __shfl_xor(bc, off, 64);
    if (oc != 0x7fffffff && (bc == 0x7fffffff || beats64<DARK>(ov, oc, bv, bc))) { bv = ov; bc = oc; }
  }
  __shared__ double sv[4];
  __shared__ int sc[4];
  if (lane == 0) { sv[wv] = bv; sc[wv] = bc; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k)
      if (sc[k] != 0x7fffffff && beats64<DARK>(sv[k], sc[k], bv, bc)) { bv = sv[k]; bc = sc[k]; }
    X.blk[blockIdx.x].v = bv; X.blk[blockIdx.x].c = bc;
  }
}

// the two columns: s_x = argmax of the new beta_x; s_y = the PENDING argmax of beta_y (the previous call's, :66), and the new
// one becomes pending.  current_sy: the option "vsync_current_sy" (s_y of this image).  DARK: argmin on both axes.
template <bool DARK>
__global__ void k_pick64(const Best64 *__restrict__ bx, int nbx, const Best64 *__restrict__ by, int nby, int *__restrict__ pending,
                         int *__restrict__ out, int current_sy) {
  if (threadIdx.x != 0) return;
  double v = bx[0].v; int c = bx[0].c;
  for (int k = 1; k < nbx; ++k) if (beats64<DARK>(bx[k].v, bx[k].c, v, c)) { v = bx[k].v; c = bx[k].c; }
  const int sx = c;
  v = by[0].v; c = by[0].c;
  for (int k = 1; k < nby; ++k) if (beats64<DARK>(by[k].v, by[k].c, v, c)) { v = by[k].v; c = by[k].c; }
  const int old_sy = pending[0];
  pending[0] = c;
  if (out) { out[0] = current_sy ? c : old_sy; out[1] = sx; }
}

static int beta_blocks(int n) { return (int)ceil_div((size_t)n, 256); }

static int sync64_argmax_check(tsdr_ctx *ctx, const tsdr_sync *s, const char *what) {
  if (!s->f64) return set_err(ctx, TSDR_EINVAL, "%s: SyncXY{Float32} state (use the f32 entry point)", what);
  return TSDR_OK;
}

}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_sync_create_f64(tsdr_ctx *ctx, int y_t, int x_t, tsdr_sync **out) {
  if (!ctx || !out) return TSDR_EINVAL;
  *out = nullptr;
  if (y_t < 8 || x_t < 20) return set_err(ctx, TSDR_EINVAL, "SyncXY needs an image of at least 8x20");
  if (y_t > 6000 || x_t > 6000) return set_err(ctx, TSDR_EINVAL, "SyncXY supports images up to 6000x6000 (got %dx%d)", y_t, x_t);
  tsdr_sync *s = new tsdr_sync();
  s->ctx = ctx; s->y_t = y_t; s->x_t = x_t; s->f64 = true;
  // init_gaussian_filter(5): exp(-2k^2/25), k=-2..2, normalised -- Float64 throughout
  double t[5], sum = 0.0;
  for (int k = -2; k <= 2; ++k) { t[k + 2] = exp(-2.0 * (double)(k * k) / 25.0); sum += t[k + 2]; }
  for (int i = 0; i < 5; ++i) { s->h64[i] = t[i] / sum; s->h[i] = (float)s->h64[i]; }
  s->wmin_y = (int)ceil(1.0 / 100.0 * (double)y_t);
  s->wmax_y = (int)floor((double)y_t / 4.0);
  s->wmin_x = (int)ceil(5.0 / 100.0 * (double)x_t);
  s->wmax_x = (int)floor((double)x_t / 4.0);
  const size_t nbx = (size_t)(1 + s->wmax_x - s->wmin_x) * x_t, nby = (size_t)(1 + s->wmax_y - s->wmin_y) * y_t;
  s->blk64_cap = (size_t)beta_blocks(x_t) + beta_blocks(y_t);
  if (hipMalloc((void **)&s->beta64_x, nbx * 8) != hipSuccess || hipMalloc((void **)&s->beta64_y, nby * 8) != hipSuccess ||
      hipMalloc((void **)&s->blk64, s->blk64_cap * sizeof(Best64)) != hipSuccess || hipMalloc((void **)&s->pending, 16) != hipSuccess) {
    tsdr_sync_free(s);
    return set_err(ctx, TSDR_ENOMEM, "sync state allocation failed");
  }
  int rc = tsdr_sync_reset(s);
  if (rc) { tsdr_sync_free(s); return rc; }
  *out = s;
  return TSDR_OK;
}

int tsdr_vsync_f64_d(tsdr_sync *s, const double *img, int *s_yx_dev) {
  if (!s || !img) return TSDR_EINVAL;
  tsdr_ctx *ctx = s->ctx;
  if (int rc = sync64_argmax_check(ctx, s, "tsdr_vsync_f64_d")) return rc;
  const int y = s->y_t, x = s->x_t;
  double *proj = (double *)ctx->scratch(WS_F64_C, (size_t)2 * (x + y) * 8);
  if (!proj) return TSDR_ENOMEM;
  double *cv = proj, *ch = cv + x, *cvf = ch + y, *chf = cvf + x;
  TSDR_LAUNCH(ctx, "vsync_f64_colsum", k_colsum64, dim3((unsigned)ceil_div((size_t)x, 64)), dim3(64), 0, img, y, x, cv);
  TSDR_LAUNCH(ctx, "vsync_f64_rowsum", k_rowsum64, dim3((unsigned)ceil_div((size_t)y, 64)), dim3(64), 0, img, y, x, ch);
  Taps64 T;
  for (int i = 0; i < 5; ++i) T.h[i] = s->h64[i];
  TSDR_LAUNCH(ctx, "vsync_f64_fir", k_fir64, dim3((unsigned)ceil_div((size_t)x + y, 256)), dim3(256), 0, (const double *)cv, x, cvf,
              (const double *)ch, y, chf, T);
  Beta64Args A;
  const int nbx = beta_blocks(x), nby = beta_blocks(y);
  A.ax[0] = Beta64Axis{cvf, x, s->wmin_x, s->wmax_x, s->beta64_x, reinterpret_cast<Best64 *>(s->blk64)};
  A.ax[1] = Beta64Axis{chf, y, s->wmin_y, s->wmax_y, s->beta64_y, reinterpret_cast<Best64 *>(s->blk64) + nbx};
  const bool dark = ctx->opt_vsync_blank_dark != 0;
  void (*const kbeta)(Beta64Args) = dark ? k_beta64<true> : k_beta64<false>;
  void (*const kpick)(const Best64 *, int, const Best64 *, int, int *, int *, int) = dark ? k_pick64<true> : k_pick64<false>;
  TSDR_LAUNCH(ctx, "vsync_f64_beta", kbeta, dim3((unsigned)std::max(nbx, nby), 2), dim3(256), 0, A);
  TSDR_LAUNCH(ctx, "vsync_f64_pick", kpick, dim3(1), dim3(64), 0, (const Best64 *)A.ax[0].blk, nbx, (const Best64 *)A.ax[1].blk, nby,
              s->pending, s_yx_dev, ctx->opt_vsync_current_sy);
  return TSDR_OK;
}

int tsdr_vsync_f64(tsdr_sync *s, const double *img, int *s_y, int *s_x) {
  if (!s || !img || !s_y || !s_x) return TSDR_EINVAL;
  tsdr_ctx *ctx = s->ctx;
  if (int rc = sync64_argmax_check(ctx, s, "tsdr_vsync_f64")) return rc;
  const size_t bytes = (size_t)s->y_t * s->x_t * 8;
  HostStage st(ctx);
  const int *hidx = (const int *)st.small(8);
  const double *d = (const double *)st.in(WS_F64_A, img, bytes);
  int *didx = (int *)st.out(WS_F64_B, (void *)hidx, 8);
  if (int rc = st.run(__func__, [&] { return tsdr_vsync_f64_d(s, d, didx); })) return rc;
  *s_y = hidx[0]; *s_x = hidx[1];
  return TSDR_OK;
}

int tsdr_sync_beta_f64(tsdr_sync *s, int which, double *beta_host) {
  if (!s || !beta_host || (which != 0 && which != 1)) return TSDR_EINVAL;
  tsdr_ctx *ctx = s->ctx;
  if (int rc = sync64_argmax_check(ctx, s, "tsdr_sync_beta_f64")) return rc;
  const size_t n = which == 0 ? (size_t)(1 + s->wmax_x - s->wmin_x) * s->x_t : (size_t)(1 + s->wmax_y - s->wmin_y) * s->y_t;
  return read_back(ctx, false, beta_host, which == 0 ? s->beta64_x : s->beta64_y, n * 8, __func__);
}

int tsdr_fill_beta_f64(tsdr_ctx *ctx, const double *cv, int n, int w_min, int w_max, double *beta) {
  if (!ctx || !cv || !beta || n < 2 || w_min < 1 || w_max < w_min || w_max >= n) return TSDR_EINVAL;
  const size_t W = (size_t)(w_max - w_min + 1);
  Best64 *blk = (Best64 *)ctx->scratch(WS_F64_C, (size_t)beta_blocks(n) * sizeof(Best64));
  if (!blk) return TSDR_ENOMEM;
  return host_map(ctx, cv, (size_t)n * 8, beta, W * n * 8, [&](void *i, void *o) {
    Beta64Args A;
    A.ax[0] = Beta64Axis{(const double *)i, n, w_min, w_max, (double *)o, blk};
    A.ax[1] = A.ax[0];
    TSDR_LAUNCH(ctx, "fill_beta_f64", k_beta64<false>, dim3((unsigned)beta_blocks(n), 1), dim3(256), 0, A);
    return (int)TSDR_OK;
  });
}

}  // extern "C"
