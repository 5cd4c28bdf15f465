// resample64.hip -- Resampler.jl's imresize / sig_to_image / downgradeImage / naiveResampler on Float64 input
// (Resampler.jl:103-126 run on whatever element type comes in; a :double capture hands them Float64).
// The coordinate, clamp and blend sequence is the one the f32 EXACT kernels and oracle/tempest_oracle.c (resize_axis /
// resize_coord / lin_pos) follow -- f64 sf*i + off in two roundings, clamp to [1, n_in], floor stepped back at the upper
// edge, (1-d)*a + d*b in two products and a sum, the first dimension outermost in 2-D -- with the result KEPT in f64.
// On f32-representable input, rounding these results to f32 therefore gives the f32 entry points' values bit for bit.
// imresize's same-size short-circuit copies the input unchanged.
#include "common.h"

namespace tsdr {

// 0-based left sample index and right-sample weight of 1-based destination index i1 (64-bit indices: 1-D inputs may be long)
__device__ inline size_t rs_pos64(const RsAxis &a, double i1, double &delta) {
  double x = __dadd_rn(__dmul_rn(a.sf, i1), a.off);
  x = fmax(x, 1.0);
  x = fmin(x, a.n_in);
  double xf = floor(x);
  if (xf > a.n_in - 1.0) xf -= 1.0;
  delta = x - xf;
  return (size_t)xf - 1;
}
__device__ inline double rs_blend64(double a, double b, double d) { return __dadd_rn(__dmul_rn(1.0 - d, a), __dmul_rn(d, b)); }

__global__ __launch_bounds__(256) void k_resize1d64(const double *__restrict__ in, size_t n_in, size_t n_out, double *__restrict__ out) {
  const RsAxis ax = rs_axis(n_in, n_out);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (size_t)gridDim.x * blockDim.x) {
    double d;
    const size_t k = rs_pos64(ax, (double)(i + 1), d);
    out[i] = rs_blend64(in[k], in[k + 1], d);
  }
}

// sig_to_image: img(l, p) = imresize(sig, y_t*x_t)[l*x_t + p], column-major (y_t, x_t).  One workgroup per 64 x 64 tile:
// pixels are formed along p (consecutive flat indices: contiguous input), parked in LDS, and stored along l (contiguous
// output columns), so both the reads and the 8-byte stores of the transpose are coalesced.
constexpr int kT64 = 64;
__global__ __launch_bounds__(256) void k_s2i64(const double *__restrict__ sig, size_t S, int y_t, int x_t, double *__restrict__ img) {
  __shared__ double tile[kT64][kT64 + 1];  // [p][l]
  const size_t P = (size_t)y_t * x_t;
  const RsAxis ax = rs_axis(S, P);
  const int l0 = blockIdx.y * kT64, p0 = blockIdx.x * kT64, t = threadIdx.x;
  const bool same = S == P;
#pragma unroll 4
  for (int m = 0; m < kT64 / 4; ++m) {
    const int pc = t & 63, lr = m * 4 + (t >> 6);
    const int l = l0 + lr, p = p0 + pc;
    if (l < y_t && p < x_t) {
      const size_t i = (size_t)l * x_t + p;
      double v;
      if (same) {
        v = sig[i];
      } else {
        double d;
        const size_t k = rs_pos64(ax, (double)(i + 1), d);
        v = rs_blend64(sig[k], sig[k + 1], d);
      }
      tile[pc][lr] = v;
    }
  }
  __syncthreads();
#pragma unroll 4
  for (int m = 0; m < kT64 / 4; ++m) {
    const int lr = t & 63, pc = m * 4 + (t >> 6);
    const int l = l0 + lr, p = p0 + pc;
    if (l < y_t && p < x_t) img[(size_t)p * y_t + l] = tile[pc][lr];
  }
}

// imresize(image, (h_out, w_out)) on a column-major matrix: wy0*(wx0*a00 + wx1*a01) + wy1*(wx0*a10 + wx1*a11)
__global__ __launch_bounds__(256) void k_resize2d64(const double *__restrict__ in, int h_in, int w_in, int h_out, int w_out,
                                                    double *__restrict__ out) {
  const RsAxis ay = rs_axis((size_t)h_in, (size_t)h_out), ax = rs_axis((size_t)w_in, (size_t)w_out);
  const size_t n = (size_t)h_out * w_out;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) {
    const size_t c = j / (size_t)h_out, r = j - c * (size_t)h_out;
    double dx, dy;
    const size_t kx = rs_pos64(ax, (double)(c + 1), dx);
    const size_t ky = rs_pos64(ay, (double)(r + 1), dy);
    const double a00 = in[kx * h_in + ky], a10 = in[kx * h_in + ky + 1];
    const double a01 = in[(kx + 1) * h_in + ky], a11 = in[(kx + 1) * h_in + ky + 1];
    const double top = rs_blend64(a00, a01, dx), bot = rs_blend64(a10, a11, dx);
    out[j] = rs_blend64(top, bot, dy);
  }
}

__global__ __launch_bounds__(256) void k_naive64(const double *__restrict__ in, size_t n_out, unsigned up, double *__restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (size_t)gridDim.x * blockDim.x) out[i] = in[i / up];
}

}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_resize1d_f64_d(tsdr_ctx *ctx, const double *sig, size_t n_in, size_t n_out, double *out) {
  if (!ctx || (n_out && (!sig || !out))) return TSDR_EINVAL;
  if (n_out == 0) return TSDR_OK;
  if (n_in == n_out) {
    if (int rf = run_fence(ctx)) return rf;   // (a copy, not a launch)
    TSDR_HIP(ctx, hipMemcpyAsync(out, sig, n_in * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return TSDR_OK;
  }
  if (n_in < 2) return set_err(ctx, TSDR_EINVAL, "imresize needs at least 2 input samples");
  TSDR_LAUNCH(ctx, "resize1d_f64", k_resize1d64, dim3(stream_grid(ctx, n_out)), dim3(256), 0, sig, n_in, n_out, out);
  return TSDR_OK;
}

int tsdr_sig_to_image_f64_d(tsdr_ctx *ctx, const double *sig, size_t S, int y_t, int x_t, double *img) {
  if (!ctx || !sig || !img) return TSDR_EINVAL;
  if (y_t <= 0 || x_t <= 0) return set_err(ctx, TSDR_EINVAL, "y_t and x_t must be positive");
  const size_t P = (size_t)y_t * (size_t)x_t;
  if (S >= (size_t(1) << 31) || P >= (size_t(1) << 31)) return set_err(ctx, TSDR_EINVAL, "frame larger than 2^31 samples/pixels");
  if (S != P && S < 2) return set_err(ctx, TSDR_EINVAL, "imresize needs at least 2 input samples");
  const dim3 grid((unsigned)ceil_div((size_t)x_t, kT64), (unsigned)ceil_div((size_t)y_t, kT64));
  TSDR_LAUNCH(ctx, "sig_to_image_f64", k_s2i64, grid, dim3(256), 0, sig, S, y_t, x_t, img);
  return TSDR_OK;
}

int tsdr_resize2d_f64_d(tsdr_ctx *ctx, const double *img, int h_in, int w_in, int h_out, int w_out, double *out) {
  if (!ctx || !img || !out) return TSDR_EINVAL;
  if (h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0) return set_err(ctx, TSDR_EINVAL, "resize2d: sizes must be positive");
  if (h_in == h_out && w_in == w_out) {
    if (int rf = run_fence(ctx)) return rf;   // (a copy, not a launch)
    TSDR_HIP(ctx, hipMemcpyAsync(out, img, (size_t)h_in * w_in * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return TSDR_OK;
  }
  if (h_in < 2 || w_in < 2) return set_err(ctx, TSDR_EINVAL, "resize2d: needs at least 2x2 input");
  TSDR_LAUNCH(ctx, "resize2d_f64", k_resize2d64, dim3(stream_grid(ctx, (size_t)h_out * w_out)), dim3(256), 0, img, h_in, w_in, h_out,
              w_out, out);
  return TSDR_OK;
}

int tsdr_downgrade_f64_d(tsdr_ctx *ctx, const double *img, int y_t, int x_t, double *out) {
  return tsdr_resize2d_f64_d(ctx, img, y_t, x_t, TSDR_RENDER_H, TSDR_RENDER_W, out);
}

int tsdr_naive_resample_f64_d(tsdr_ctx *ctx, const double *in, size_t n, int up, double *out) {
  if (!ctx || up < 1 || (n && (!in || !out))) return TSDR_EINVAL;
  if (n == 0) return TSDR_OK;
  TSDR_LAUNCH(ctx, "naive_resample_f64", k_naive64, dim3(stream_grid(ctx, n * (size_t)up)), dim3(256), 0, in, n * (size_t)up,
              (unsigned)up, out);
  return TSDR_OK;
}

int tsdr_resize1d_f64(tsdr_ctx *ctx, const double *sig, size_t n_in, size_t n_out, double *out) {
  return host_map(ctx, sig, n_in * 8, out, n_out * 8,
                  [&](void *i, void *o) { return tsdr_resize1d_f64_d(ctx, (const double *)i, n_in, n_out, (double *)o); });
}
int tsdr_sig_to_image_f64(tsdr_ctx *ctx, const double *sig, size_t S, int y_t, int x_t, double *img) {
  if (y_t <= 0 || x_t <= 0) return TSDR_EINVAL;
  return host_map(ctx, sig, S * 8, img, (size_t)y_t * x_t * 8,
                  [&](void *i, void *o) { return tsdr_sig_to_image_f64_d(ctx, (const double *)i, S, y_t, x_t, (double *)o); });
}
int tsdr_resize2d_f64(tsdr_ctx *ctx, const double *img, int h_in, int w_in, int h_out, int w_out, double *out) {
  if (h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0) return TSDR_EINVAL;
  return host_map(ctx, img, (size_t)h_in * w_in * 8, out, (size_t)h_out * w_out * 8,
                  [&](void *i, void *o) { return tsdr_resize2d_f64_d(ctx, (const double *)i, h_in, w_in, h_out, w_out, (double *)o); });
}
int tsdr_downgrade_f64(tsdr_ctx *ctx, const double *img, int y_t, int x_t, double *out) {
  return tsdr_resize2d_f64(ctx, img, y_t, x_t, TSDR_RENDER_H, TSDR_RENDER_W, out);
}
int tsdr_naive_resample_f64(tsdr_ctx *ctx, const double *in, size_t n, int up, double *out) {
  if (up < 1) return TSDR_EINVAL;
  return host_map(ctx, in, n * 8, out, n * (size_t)up * 8,
                  [&](void *i, void *o) { return tsdr_naive_resample_f64_d(ctx, (const double *)i, n, up, (double *)o); });
}

}  // extern "C"
