// spectrum64.hip -- calculate_autocorrelation (Autocorrelations.jl:23-37) and getSpectrum (GetSpectrum.jl:21-30) on Float64 /
// ComplexF64 input, through the complex f64 transform of fft64.hip (Stockham passes for lengths whose prime factors are <= 13,
// Bluestein for the rest).  What the f64 path adds around it:
//   autocorr : a widening loader of x[1:n], n = min(2 indexMax, len), as (x, 0); fft; |X|^2 in place (re*re + im*im, no
//              FMA); ifft (1/n); the lags [indexMin, indexMax] as 10log10(abs2(c)) (or abs2) into Float64.
//   spectrum : a loader of N real or complex samples; fft; fftshift + abs2 (+ 10log10) into Float64.
// Both transform in the context's own f64 workspaces (WS_F64_A / _B), grown on first use and released by tsdr_destroy.
#include "common.h"

namespace tsdr {

int fft64_d(tsdr_ctx *ctx, double2 *data, double2 *scratch, size_t N, int dir);
int autocorr_args(tsdr_ctx *ctx, size_t len, double Fs, double minDelay, double maxDelay, size_t *n, size_t *k0, size_t *cnt);

__device__ inline double abs2_64(double2 c) { return __dadd_rn(__dmul_rn(c.x, c.x), __dmul_rn(c.y, c.y)); }
__device__ inline double db_or_lin64(double p, int log_scale) { return log_scale ? __dmul_rn(10.0, log10(p)) : p; }

// X[i] = sig[i] as a complex value: real input widened with a zero imaginary part, complex input copied
__global__ __launch_bounds__(256) void k_load64(const double *__restrict__ sig, int is_complex, size_t n, double2 *__restrict__ X) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    X[i] = is_complex ? reinterpret_cast<const double2 *>(sig)[i] : make_double2(sig[i], 0.0);
}

__global__ __launch_bounds__(256) void k_pow64(double2 *__restrict__ X, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    X[i] = make_double2(abs2_64(X[i]), 0.0);
}

// out[k] = 10log10(abs2(c[k0 + k])) (or abs2), k < cnt
__global__ __launch_bounds__(256) void k_ac_out64(const double2 *__restrict__ c, size_t k0, size_t cnt, int log_scale,
                                                  double *__restrict__ out) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += (size_t)gridDim.x * blockDim.x)
    out[k] = db_or_lin64(abs2_64(c[k0 + k]), log_scale);
}

// fftshift: y[j] takes X[(j + N - N/2) mod N]
__global__ __launch_bounds__(256) void k_spec_out64(const double2 *__restrict__ X, size_t N, int log_scale, double *__restrict__ y) {
  const size_t h = N - N / 2;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (size_t)gridDim.x * blockDim.x) {
    size_t s = j + h;
    if (s >= N) s -= N;
    y[j] = db_or_lin64(abs2_64(X[s]), log_scale);
  }
}

static int ws64(tsdr_ctx *ctx, size_t n, double2 **X, double2 **T) {
  *X = (double2 *)ctx->scratch(WS_F64_A, n * sizeof(double2));
  *T = (double2 *)ctx->scratch(WS_F64_B, n * sizeof(double2));
  return (*X && *T) ? (int)TSDR_OK : (int)TSDR_ENOMEM;
}

// is_complex: x is ComplexF64 and the lags are those of the complex sequence itself (autocorr_cplx.hip) -- the loader copies
// instead of widening; everything behind it is complex already
int autocorr64_core(tsdr_ctx *ctx, const double *x, size_t n, size_t k0, size_t cnt, int log_scale, double *out, int is_complex = 0) {
  double2 *X, *T;
  if (int rc = ws64(ctx, n, &X, &T)) return rc;
  TSDR_LAUNCH(ctx, "autocorr_f64_load", k_load64, dim3(stream_grid(ctx, n)), dim3(256), 0, x, is_complex, n, X);
  if (int rc = fft64_d(ctx, X, T, n, -1)) return rc;
  TSDR_LAUNCH(ctx, "autocorr_f64_power", k_pow64, dim3(stream_grid(ctx, n)), dim3(256), 0, X, n);
  if (int rc = fft64_d(ctx, X, T, n, +1)) return rc;
  TSDR_LAUNCH(ctx, "autocorr_f64_out", k_ac_out64, dim3(stream_grid(ctx, cnt)), dim3(256), 0, (const double2 *)X, k0, cnt, log_scale, out);
  return TSDR_OK;
}

static int spectrum64_core(tsdr_ctx *ctx, const double *sig, int is_complex, size_t N, int lin, double *y) {
  if (N == 0) return TSDR_OK;
  double2 *X, *T;
  if (int rc = ws64(ctx, N, &X, &T)) return rc;
  TSDR_LAUNCH(ctx, "spectrum_f64_load", k_load64, dim3(stream_grid(ctx, N)), dim3(256), 0, sig, is_complex, N, X);
  if (int rc = fft64_d(ctx, X, T, N, -1)) return rc;
  TSDR_LAUNCH(ctx, "spectrum_f64_out", k_spec_out64, dim3(stream_grid(ctx, N)), dim3(256), 0, (const double2 *)X, N, !lin, y);
  return TSDR_OK;
}

}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_autocorr_f64_d(tsdr_ctx *ctx, const double *x, size_t len, double Fs, double minDelay, double maxDelay, int log_scale,
                        double *out, size_t *n_out) {
  if (!ctx || !x || !out) return TSDR_EINVAL;
  size_t n, k0, cnt;
  int rc = autocorr_args(ctx, len, Fs, minDelay, maxDelay, &n, &k0, &cnt);
  if (rc) return rc;
  if (n_out) *n_out = cnt;
  if (cnt == 0) return TSDR_OK;
  return autocorr64_core(ctx, x, n, k0, cnt, log_scale, out);
}

int tsdr_autocorr_f64(tsdr_ctx *ctx, const double *x, size_t len, double Fs, double minDelay, double maxDelay, int log_scale,
                      double *out, size_t *n_out) {
  if (!ctx || !x || !out) return TSDR_EINVAL;
  size_t n, k0, cnt;
  int rc = autocorr_args(ctx, len, Fs, minDelay, maxDelay, &n, &k0, &cnt);
  if (rc) return rc;
  if (n_out) *n_out = cnt;
  if (cnt == 0) return TSDR_OK;
  return host_map(ctx, x, n * 8, out, cnt * 8,
                  [&](void *i, void *o) { return autocorr64_core(ctx, (const double *)i, n, k0, cnt, log_scale, (double *)o); });
}

int tsdr_spectrum_f64_d(tsdr_ctx *ctx, const double *sig, int is_complex, size_t N, int lin, double *y) {
  if (!ctx || (N && (!sig || !y))) return TSDR_EINVAL;
  if (is_complex && ((uintptr_t)sig & 15)) return set_err(ctx, TSDR_EINVAL, "spectrum_f64: complex input must be 16-byte aligned");
  return spectrum64_core(ctx, sig, is_complex, N, lin, y);
}

int tsdr_spectrum_f64(tsdr_ctx *ctx, const double *sig, int is_complex, size_t N, int lin, double *y) {
  return host_map(ctx, sig, N * (is_complex ? 16 : 8), y, N * 8,
                  [&](void *i, void *o) { return spectrum64_core(ctx, (const double *)i, is_complex, N, lin, (double *)o); });
}

}  // extern "C"
