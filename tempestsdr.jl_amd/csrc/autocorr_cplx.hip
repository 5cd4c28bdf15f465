// autocorr_cplx.hip -- calculate_autocorrelation (Autocorrelations.jl:23-37) of COMPLEX input on gfx950: the circular
// autocorrelation r[k] = sum_m z[(m+k) mod n] conj(z[m]) = ifft(fft(z) .* conj(fft(z)))[k] of the first n IQ samples themselves
// (ComplexF32, ComplexF64, or integer IQ as the SDR stored it), then abs2 / 10log10 of the lags k0 .. k0+cnt.  The contract is
// include/tempest_hip_cplx.h's.
//
// Simpler than the real route of autocorr.hip: nothing is packed two-per-complex, so the power spectrum is pointwise and the last
// pass's output o IS lag o.  It moves a length-n transform where the real route moves n/2 points.
//   n = 2^a 3^b 5^c of two or more passes: two native transforms.  First forward pass: SRC_C2C / SRC_IQ_* (integer IQ is read as
//     stored); first inverse pass: SRC_ABS2, (|Z[g]|^2, 0) while loading; last inverse pass: EPI_CAC writes the wanted lags and
//     carries the findmax.  No pointwise kernel touches HBM in between.
//   every other n: fft_any (one-pass lengths, Bluestein) around k_cac_power / k_cac_finish, k_argmax for the search.
#include <cstdint>

#include "amax.h"
#include "fft_dev.h"

namespace tsdr {

int autocorr_args(tsdr_ctx *ctx, size_t len, double Fs, double minDelay, double maxDelay, size_t *n, size_t *k0, size_t *cnt);
int autocorr64_core(tsdr_ctx *ctx, const double *x, size_t n, size_t k0, size_t cnt, int log_scale, double *out, int is_complex);

// in place: Z[g] -> (|Z[g]|^2, 0)
__global__ __launch_bounds__(256) void k_cac_power(float2 *__restrict__ Z, size_t n) {
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (size_t)gridDim.x * blockDim.x) {
    const float2 a = Z[g];
    Z[g] = make_float2(a.x * a.x + a.y * a.y, 0.f);
  }
}

// out[i] = abs2(r[k0 + i]) or 10log10 of it, i < cnt
__global__ __launch_bounds__(256) void k_cac_finish(const float2 *__restrict__ r, size_t k0, size_t cnt, int log_scale,
                                                    float *__restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (size_t)gridDim.x * blockDim.x) {
    const float2 x = r[k0 + i];
    const float p = x.x * x.x + x.y * x.y;
    out[i] = log_scale ? 10.0f * log10f(p) : p;
  }
}

// the two-transform route: n = 2^a 3^b 5^c of two or more passes ("ac_mixed" = 0 keeps it to the powers of two)
static bool cac_native(tsdr_ctx *ctx, size_t n) {
  return fft_passes(n) >= 2 && (is_pow2(n) || ctx->opt_ac_mixed != 0);
}

// shared core: the first n samples of z, ComplexF32 or integer IQ (1 <= n < 2^31, cnt >= 1, k0 + cnt <= n)
static int autocorr_cplx_core(tsdr_ctx *ctx, const SigSrc &z, size_t n, size_t k0, size_t cnt, int log_scale, float *out,
                              AmaxReq *amax = nullptr) {
  float2 *X = (float2 *)ctx->scratch(WS_FFT_A, n * sizeof(float2));
  if (!X) return TSDR_ENOMEM;
  if (cac_native(ctx, n)) {
    FftReq f;
    f.out = X; f.n = n;
    int rc = fft_run(ctx, f.load(z, src_of(z.kind)));
    if (rc) return rc;
    FftEpilogue epi;
    epi.kind = EPI_CAC;
    epi.out = out;
    epi.k0 = k0;
    epi.cnt = cnt;
    epi.log_scale = log_scale;
    if (amax && amax->cnt) {
      epi.amax_keys = amax->slots; epi.amax_lo = amax->lo; epi.amax_cnt = amax->cnt;
      amax->fused = true;
    }
    // (nothing is stored through the `out` argument of a pass with an epilogue; lags past the window are not formed into outputs)
    FftReq b;
    b.in = X; b.out = X; b.n = n; b.dir = +1; b.scale = (float)(1.0 / (double)n); b.src_mode = SRC_ABS2; b.keep = k0 + cnt; b.epi = &epi;
    return fft_run(ctx, b);
  }
  // (one-launch and Bluestein lengths: integer samples are expanded into the workspace first, fft_any)
  int rc = fft_any(ctx, z, X, n, 1, -1);
  if (rc) return rc;
  TSDR_LAUNCH(ctx, "cac_power", k_cac_power, dim3(stream_grid(ctx, n)), dim3(256), 0, X, n);
  rc = fft_any(ctx, SigSrc{X, SIG_CF32, 1.0f}, X, n, 1, +1);
  if (rc) return rc;
  TSDR_LAUNCH(ctx, "cac_finish", k_cac_finish, dim3(stream_grid(ctx, cnt)), dim3(256), 0, (const float2 *)X, k0, cnt, log_scale, out);
  return TSDR_OK;
}

// the arguments every form shares; *n = 0 when there is nothing to do (cnt == 0)
static int cac_args(tsdr_ctx *ctx, size_t len, double Fs, double minDelay, double maxDelay, size_t *n, size_t *k0, size_t *cnt,
                    size_t *n_out) {
  int rc = autocorr_args(ctx, len, Fs, minDelay, maxDelay, n, k0, cnt);
  if (rc) return rc;
  if (n_out) *n_out = *cnt;
  if (*n >= (size_t(1) << 31)) return set_err(ctx, TSDR_EINVAL, "autocorr_cplx: window too long");
  return TSDR_OK;
}

}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_autocorr_cplx_search_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t len, double Fs, double minDelay,
                                   double maxDelay, int log_scale, float *out, size_t *n_out, size_t win_lo, size_t win_cnt,
                                   size_t *idx, float *val) {
  if (!ctx || !iq || !out || (win_cnt && !idx)) return TSDR_EINVAL;
  IqFmt f;
  TSDR_IQ_ARG(ctx, "autocorr_cplx", iq, iq_fmt, scale, f);
  TSDR_PTR_ALIGNED(ctx, "autocorr_cplx", out, 4);
  size_t n, k0, cnt;
  int rc = cac_args(ctx, len, Fs, minDelay, maxDelay, &n, &k0, &cnt, n_out);
  if (rc) return rc;
  if (win_cnt == 0) return cnt ? autocorr_cplx_core(ctx, sig_iq(iq, f), n, k0, cnt, log_scale, out) : (int)TSDR_OK;
  if (win_lo >= cnt || win_cnt > cnt - win_lo) return set_err(ctx, TSDR_EBOUNDS, "autocorr_cplx_search: window outside the lag vector");
  if (win_cnt >= (size_t(1) << 32)) return set_err(ctx, TSDR_EINVAL, "argmax: vector too long");
  AmaxReq r;
  rc = amax_begin(ctx, &r);
  if (rc) return rc;
  r.lo = win_lo;
  r.cnt = win_cnt;
  ctx->amax_dirty = true;   // until the publish launch (or the route without an epilogue) is known to have been enqueued
  rc = autocorr_cplx_core(ctx, sig_iq(iq, f), n, k0, cnt, log_scale, out, &r);
  if (rc) return rc;
  if (!r.fused) {  // the routes around fft_any: the separate kernel
    ctx->amax_dirty = false;
    rc = argmax_launch(ctx, out + win_lo, win_cnt, r);
    if (rc) return rc;
  } else {
    rc = amax_publish(ctx, r);
    if (rc) return rc;
    ctx->amax_dirty = false;
  }
  return amax_wait(ctx, r.seq, idx, val);
}

int tsdr_autocorr_cplx_d(tsdr_ctx *ctx, const float *z, size_t len, double Fs, double minDelay, double maxDelay, int log_scale,
                         float *out, size_t *n_out) {
  if (!ctx || !z || !out) return TSDR_EINVAL;
  TSDR_PTR_ALIGNED(ctx, "autocorr_cplx", z, 8);
  TSDR_PTR_ALIGNED(ctx, "autocorr_cplx", out, 4);
  size_t n, k0, cnt;
  int rc = cac_args(ctx, len, Fs, minDelay, maxDelay, &n, &k0, &cnt, n_out);
  if (rc || cnt == 0) return rc;
  return autocorr_cplx_core(ctx, sig_f32(z, 1), n, k0, cnt, log_scale, out);
}

int tsdr_autocorr_cplx_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t len, double Fs, double minDelay,
                          double maxDelay, int log_scale, float *out, size_t *n_out) {
  if (!ctx || !iq || !out) return TSDR_EINVAL;
  TSDR_IQ_FMT_ARG(ctx, "autocorr_cplx_iq", iq_fmt);
  SigSrc z = sig_iq(iq, IqFmt{iq_fmt, iq_fmt == TSDR_IQ_CF32 ? 1.0f : scale});
  size_t n, k0, cnt;
  int rc = cac_args(ctx, len, Fs, minDelay, maxDelay, &n, &k0, &cnt, n_out);
  if (rc || cnt == 0) return rc;
  return host_map(ctx, iq, n * z.bytes(), out, cnt * 4,   // the raw bytes go up, not expanded ones
                  [&](void *i, void *o) { z.p = i; return autocorr_cplx_core(ctx, z, n, k0, cnt, log_scale, (float *)o); });
}

int tsdr_autocorr_cplx(tsdr_ctx *ctx, const float *z, size_t len, double Fs, double minDelay, double maxDelay, int log_scale,
                       float *out, size_t *n_out) {
  return tsdr_autocorr_cplx_iq(ctx, z, TSDR_IQ_CF32, 1.0f, len, Fs, minDelay, maxDelay, log_scale, out, n_out);
}

int tsdr_autocorr_cplx_f64_d(tsdr_ctx *ctx, const double *z, size_t len, double Fs, double minDelay, double maxDelay,
                             int log_scale, double *out, size_t *n_out) {
  if (!ctx || !z || !out) return TSDR_EINVAL;
  TSDR_PTR_ALIGNED(ctx, "autocorr_cplx_f64", z, 16);
  TSDR_PTR_ALIGNED(ctx, "autocorr_cplx_f64", out, 8);
  size_t n, k0, cnt;
  int rc = cac_args(ctx, len, Fs, minDelay, maxDelay, &n, &k0, &cnt, n_out);
  if (rc || cnt == 0) return rc;
  return autocorr64_core(ctx, z, n, k0, cnt, log_scale, out, 1);
}

int tsdr_autocorr_cplx_f64(tsdr_ctx *ctx, const double *z, size_t len, double Fs, double minDelay, double maxDelay,
                           int log_scale, double *out, size_t *n_out) {
  if (!ctx || !z || !out) return TSDR_EINVAL;
  size_t n, k0, cnt;
  int rc = cac_args(ctx, len, Fs, minDelay, maxDelay, &n, &k0, &cnt, n_out);
  if (rc || cnt == 0) return rc;
  return host_map(ctx, z, n * 16, out, cnt * 8,
                  [&](void *i, void *o) { return autocorr64_core(ctx, (const double *)i, n, k0, cnt, log_scale, (double *)o, 1); });
}

}  // extern "C"
