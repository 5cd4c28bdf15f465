// demod64.hip -- Demodulation.jl for Complex{Float64} input (amDemod / invert_amDemod / fmDemod / abs2 on the Float64
// capture readComplexBinary(file, :double) returns, DatBinaryFiles.jl:53-64).  Streaming grid-stride kernels over double2:
// 16 B in / 8 B out per sample.  Julia's arithmetic on ComplexF64, operation for operation:
//   abs(z)   = hypot(re, im)                 device hypot: no overflow at 1e300, no flush of 1e-310, hypot(Inf, NaN) = Inf
//   abs2(z)  = re*re + im*im                 two products and a sum, no FMA (-ffp-contract=off)
//   fmDemod  = angle(s[n+1] * conj(s[n]))    the product in plain mul / add, atan2, out[1] = 0
//   invert   = 1 - a / maximum(a)            the maximum reduced on the device; NaN propagates as in Julia's maximum
#include "common.h"

namespace tsdr {

enum { DM64_ABS = 0, DM64_ABS2 = 1 };

template <int MODE>
__device__ inline double demod64(double2 z) {
  if (MODE == DM64_ABS) {
    if (isinf(z.x) || isinf(z.y)) return INFINITY;  // hypot(+-Inf, NaN) = Inf (IEEE 754 / Julia)
    return hypot(z.x, z.y);
  }
  return __dadd_rn(__dmul_rn(z.x, z.x), __dmul_rn(z.y, z.y));
}

// out[i] = f(iq[i]); TRACK_MAX: max(out) through ordered 64-bit atomics (values >= +0, so their bit patterns order like the
// values; a NaN -- any sign -- is mapped to the quiet +NaN pattern, which sorts above +Inf: Julia's maximum returns NaN)
template <int MODE, bool TRACK_MAX>
__global__ __launch_bounds__(256) void k_demod64(const double2 *__restrict__ iq, size_t n, double *__restrict__ out,
                                                 unsigned long long *__restrict__ maxbits) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  unsigned long long local = 0ull;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double v = demod64<MODE>(iq[i]);
    out[i] = v;
    if (TRACK_MAX) local = max(local, isnan(v) ? 0x7ff8000000000000ull : (unsigned long long)__double_as_longlong(v));
  }
  if (TRACK_MAX) {
    for (int off = 32; off > 0; off >>= 1) local = max(local, (unsigned long long)__shfl_xor((long long)local, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(maxbits, local);
  }
}

// out = 1 - out / max   (correctly rounded f64 division and subtraction)
__global__ __launch_bounds__(256) void k_invert64(double *__restrict__ out, size_t n, const unsigned long long *__restrict__ maxbits) {
  const double mx = __longlong_as_double((long long)*maxbits);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = __dsub_rn(1.0, __ddiv_rn(out[i], mx));
}

__global__ __launch_bounds__(256) void k_fm64(const double2 *__restrict__ iq, size_t n, double *__restrict__ out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (i == 0) { out[0] = 0.0; continue; }
    const double2 s1 = iq[i], s0 = iq[i - 1];
    const double c = s0.x, d = -s0.y;  // conj(sig[n])
    const double re = __dsub_rn(__dmul_rn(s1.x, c), __dmul_rn(s1.y, d));
    const double im = __dadd_rn(__dmul_rn(s1.x, d), __dmul_rn(s1.y, c));
    out[i] = atan2(im, re);
  }
}

static int demod64_args(tsdr_ctx *ctx, const char *kname, const double *iq, size_t n, const double *out) {
  if (!ctx || (n && (!iq || !out))) return TSDR_EINVAL;
  if (((uintptr_t)iq & 15) || ((uintptr_t)out & 7)) return set_err(ctx, TSDR_EINVAL, "%s: iq must be 16-byte, out 8-byte aligned", kname);
  return TSDR_OK;
}

template <int MODE>
static int demod64_d(tsdr_ctx *ctx, const char *kname, const double *iq, size_t n, double *out) {
  if (int rc = demod64_args(ctx, kname, iq, n, out)) return rc;
  if (n == 0) return TSDR_OK;
  TSDR_LAUNCH(ctx, kname, (k_demod64<MODE, false>), dim3(stream_grid(ctx, n)), dim3(256), 0, reinterpret_cast<const double2 *>(iq), n,
              out, (unsigned long long *)nullptr);
  return TSDR_OK;
}

}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_am_demod_f64_d(tsdr_ctx *ctx, const double *iq, size_t n, double *out) { return demod64_d<DM64_ABS>(ctx, "am_demod_f64", iq, n, out); }
int tsdr_abs2_f64_d(tsdr_ctx *ctx, const double *iq, size_t n, double *out) { return demod64_d<DM64_ABS2>(ctx, "abs2_f64", iq, n, out); }

int tsdr_invert_am_f64_d(tsdr_ctx *ctx, const double *iq, size_t n, double *out) {
  if (!ctx || n == 0) return TSDR_EINVAL;  // maximum() of an empty collection throws
  if (int rc = demod64_args(ctx, "invert_am_f64", iq, n, out)) return rc;
  unsigned long long *mx = (unsigned long long *)ctx->scratch(WS_F64_C, 16);
  if (!mx) return TSDR_ENOMEM;
  TSDR_HIP(ctx, hipMemsetAsync(mx, 0, 8, ctx->stream));
  const int grid = stream_grid(ctx, n);
  TSDR_LAUNCH(ctx, "invert_am_f64_abs", (k_demod64<DM64_ABS, true>), dim3(grid), dim3(256), 0, reinterpret_cast<const double2 *>(iq), n,
              out, mx);
  TSDR_LAUNCH(ctx, "invert_am_f64_scale", k_invert64, dim3(grid), dim3(256), 0, out, n, (const unsigned long long *)mx);
  return TSDR_OK;
}

int tsdr_fm_demod_f64_d(tsdr_ctx *ctx, const double *iq, size_t n, double *out) {
  if (int rc = demod64_args(ctx, "fm_demod_f64", iq, n, out)) return rc;
  if (n == 0) return TSDR_OK;
  TSDR_LAUNCH(ctx, "fm_demod_f64", k_fm64, dim3(stream_grid(ctx, n)), dim3(256), 0, reinterpret_cast<const double2 *>(iq), n, out);
  return TSDR_OK;
}

int tsdr_am_demod_f64(tsdr_ctx *ctx, const double *iq, size_t n, double *out) {
  return host_map(ctx, iq, n * 16, out, n * 8, [&](void *i, void *o) { return tsdr_am_demod_f64_d(ctx, (const double *)i, n, (double *)o); });
}
int tsdr_abs2_f64(tsdr_ctx *ctx, const double *iq, size_t n, double *out) {
  return host_map(ctx, iq, n * 16, out, n * 8, [&](void *i, void *o) { return tsdr_abs2_f64_d(ctx, (const double *)i, n, (double *)o); });
}
int tsdr_invert_am_f64(tsdr_ctx *ctx, const double *iq, size_t n, double *out) {
  if (n == 0) return TSDR_EINVAL;
  return host_map(ctx, iq, n * 16, out, n * 8, [&](void *i, void *o) { return tsdr_invert_am_f64_d(ctx, (const double *)i, n, (double *)o); });
}
int tsdr_fm_demod_f64(tsdr_ctx *ctx, const double *iq, size_t n, double *out) {
  return host_map(ctx, iq, n * 16, out, n * 8, [&](void *i, void *o) { return tsdr_fm_demod_f64_d(ctx, (const double *)i, n, (double *)o); });
}

}  // extern "C"
