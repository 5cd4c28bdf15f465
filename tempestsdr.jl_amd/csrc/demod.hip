// demod.hip -- Demodulation.jl on gfx950: streaming, HBM-bound kernels.
//   amDemod        Demodulation.jl:26-28   8 B in / 4 B out per sample
//   invert_amDemod Demodulation.jl:31-35   needs a global max first
//   fmDemod        Demodulation.jl:17-23
//   abs2           GUI.jl:70 (power fed to the configuration search)
// Each lane moves 16-byte vectors (4 complex samples = 2 x float4 in, 1 x float4 out);
// the grid is capped and grid-strided so a launch is a few thousand workgroups.
// The `_iq_d` forms read int16 / int8 / uint8 pairs as stored (4 or 2 B in per sample) and convert in the loader.
#include "common.h"

namespace tsdr {

enum { DM_ABS = 0, DM_ABS2 = 1 };

template <int MODE>
__device__ inline float demod1(float re, float im) {
  return MODE == DM_ABS ? abs_c(re, im) : abs2_c(re, im);
}

// out[i] = f(iq[i]); optionally tracks max(out) through ordered-uint atomics (values >= 0,
// NaN bit patterns sort above +Inf, so a NaN propagates like Julia's maximum()).
template <int MODE, bool TRACK_MAX>
__global__ __launch_bounds__(256) void k_demod(const float4 *__restrict__ iq, size_t n, float4 *__restrict__ out,
                                               unsigned *__restrict__ maxbits) {
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  unsigned local = 0u;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 a = iq[2 * i], b = iq[2 * i + 1];
    float4 r;
    r.x = demod1<MODE>(a.x, a.y);
    r.y = demod1<MODE>(a.z, a.w);
    r.z = demod1<MODE>(b.x, b.y);
    r.w = demod1<MODE>(b.z, b.w);
    out[i] = r;
    if (TRACK_MAX) {
      local = max(local, __float_as_uint(r.x));
      local = max(local, __float_as_uint(r.y));
      local = max(local, __float_as_uint(r.z));
      local = max(local, __float_as_uint(r.w));
    }
  }
  // tail (n not a multiple of 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    size_t i = (n4 << 2) + threadIdx.x;
    const float *s = reinterpret_cast<const float *>(iq);
    float v = demod1<MODE>(s[2 * i], s[2 * i + 1]);
    reinterpret_cast<float *>(out)[i] = v;
    if (TRACK_MAX) local = max(local, __float_as_uint(v));
  }
  if (TRACK_MAX) {
    for (int off = 32; off > 0; off >>= 1) local = max(local, (unsigned)__shfl_xor((int)local, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(maxbits, local);
  }
}

// The same, one sample per lane: for the pointers k_demod's 16-byte vectors cannot take (an IQ buffer that starts at an odd
// sample of a larger one, an output at any float of a larger one).  One 8-byte load and one 4-byte store per sample; the
// values -- and so the maximum -- are those of k_demod bit for bit.
template <int MODE, bool TRACK_MAX>
__global__ __launch_bounds__(256) void k_demod1(const float2 *__restrict__ iq, size_t n, float *__restrict__ out,
                                                unsigned *__restrict__ maxbits) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  unsigned local = 0u;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float2 s = iq[i];
    const float v = demod1<MODE>(s.x, s.y);
    out[i] = v;
    if (TRACK_MAX) local = max(local, __float_as_uint(v));
  }
  if (TRACK_MAX) {
    for (int off = 32; off > 0; off >>= 1) local = max(local, (unsigned)__shfl_xor((int)local, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(maxbits, local);
  }
}

// out = 1 - out/max   (f32, correctly rounded division, two roundings)
__global__ __launch_bounds__(256) void k_invert(float *__restrict__ out, size_t n, const unsigned *__restrict__ maxbits) {
  const float mx = __uint_as_float(*maxbits);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float d = __fdiv_rn(out[i], mx);
    out[i] = __fsub_rn(1.0f, d);
  }
}

__global__ __launch_bounds__(256) void k_fm(const float2 *__restrict__ iq, size_t n, float *__restrict__ out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (i == 0) { out[0] = 0.0f; continue; }
    float2 s1 = iq[i], s0 = iq[i - 1];
    float c = s0.x, d = -s0.y;  // conj(sig[n])
    float re = __fsub_rn(__fmul_rn(s1.x, c), __fmul_rn(s1.y, d));
    float im = __fadd_rn(__fmul_rn(s1.x, d), __fmul_rn(s1.y, c));
    out[i] = atan2f(im, re);
  }
}

// ---- the same from integer IQ storage (tsdr_*_iq_d: int16, int8 or uint8 pairs as the SDR stored them, TSDR_IQ_*) -------------
// A sample is converted by common.h's cvt_* (one product by `scale`), then goes through demod1 / the FM product exactly as a
// ComplexF32 sample does, so the outputs are those of the expanded buffer bit for bit.  One 16-byte load is 4 sc16 samples (one
// float4 out) or 8 eight-bit samples (two float4 out).
template <int MODE, bool TRACK_MAX, int IQF>
__global__ __launch_bounds__(256) void k_demod_iq(const uint4 *__restrict__ iq, size_t n, float scale, float4 *__restrict__ out,
                                                  unsigned *__restrict__ maxbits) {
  constexpr int SPV = IQF == IQF_SC16 ? 4 : 8;   // samples per 16-byte vector
  const size_t nv = n / SPV;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  unsigned local = 0u;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    const uint4 q = iq[i];
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    float r[SPV];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (SPV == 4) {
        const float2 a = cvt_iq<IQF>(w[k], scale);
        r[k] = demod1<MODE>(a.x, a.y);
      } else {
        const float2 a = cvt_iq<IQF>(w[k] & 0xFFFFu, scale), b = cvt_iq<IQF>(w[k] >> 16, scale);
        r[2 * k] = demod1<MODE>(a.x, a.y);
        r[2 * k + 1] = demod1<MODE>(b.x, b.y);
      }
    }
#pragma unroll
    for (int v = 0; v < SPV / 4; ++v) out[(SPV / 4) * i + v] = make_float4(r[4 * v], r[4 * v + 1], r[4 * v + 2], r[4 * v + 3]);
    if (TRACK_MAX) {
#pragma unroll
      for (int k = 0; k < SPV; ++k) local = max(local, __float_as_uint(r[k]));
    }
  }
  // tail (n not a multiple of the vector)
  if (blockIdx.x == 0 && threadIdx.x < n - nv * SPV) {
    const size_t i = nv * SPV + threadIdx.x;
    const float2 a = ld_iq_as<IQF>(iq_at(reinterpret_cast<const float *>(iq), i, iq_bytes_as<IQF>(IqFmt{})), 0u, IqFmt{IQK_CF32, scale});
    const float v = demod1<MODE>(a.x, a.y);
    reinterpret_cast<float *>(out)[i] = v;
    if (TRACK_MAX) local = max(local, __float_as_uint(v));
  }
  if (TRACK_MAX) {
    for (int off = 32; off > 0; off >>= 1) local = max(local, (unsigned)__shfl_xor((int)local, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(maxbits, local);
  }
}

// one sample per lane (a 4- or 2-byte load, a 4-byte store): any sample-aligned input, any float-aligned output
template <int MODE, bool TRACK_MAX, int IQF>
__global__ __launch_bounds__(256) void k_demod1_iq(const void *__restrict__ iq, size_t n, float scale, float *__restrict__ out,
                                                   unsigned *__restrict__ maxbits) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  unsigned local = 0u;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float2 a = ld_iq_as<IQF>(iq_at(reinterpret_cast<const float *>(iq), i, iq_bytes_as<IQF>(IqFmt{})), 0u, IqFmt{IQK_CF32, scale});
    const float v = demod1<MODE>(a.x, a.y);
    out[i] = v;
    if (TRACK_MAX) local = max(local, __float_as_uint(v));
  }
  if (TRACK_MAX) {
    for (int off = 32; off > 0; off >>= 1) local = max(local, (unsigned)__shfl_xor((int)local, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(maxbits, local);
  }
}

template <int IQF>
__global__ __launch_bounds__(256) void k_fm_iq(const void *__restrict__ iq, size_t n, float scale, float *__restrict__ out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const IqFmt f{IQK_CF32, scale};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (i == 0) { out[0] = 0.0f; continue; }
    const float *p = iq_at(reinterpret_cast<const float *>(iq), i - 1, iq_bytes_as<IQF>(f));
    const float2 s0 = ld_iq_as<IQF>(p, 0u, f), s1 = ld_iq_as<IQF>(p, 1u, f);
    float c = s0.x, d = -s0.y;  // conj(sig[n])
    float re = __fsub_rn(__fmul_rn(s1.x, c), __fmul_rn(s1.y, d));
    float im = __fadd_rn(__fmul_rn(s1.x, d), __fmul_rn(s1.y, c));
    out[i] = atan2f(im, re);
  }
}

// k_demod moves 16-byte vectors on both sides; any other element-aligned pair of pointers takes k_demod1
static inline bool vec16(const float *iq, const float *out) {
  return ((reinterpret_cast<uintptr_t>(iq) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
}

template <int MODE>
static int demod_d(tsdr_ctx *ctx, const char *kname, const float *iq, size_t n, float *out) {
  if (!ctx || (n && (!iq || !out))) return TSDR_EINVAL;
  TSDR_PTR_ALIGNED(ctx, kname, iq, 8);
  TSDR_PTR_ALIGNED(ctx, kname, out, 4);
  if (n == 0) return TSDR_OK;
  if (vec16(iq, out)) {
    TSDR_LAUNCH(ctx, MODE == DM_ABS ? "am_demod" : "abs2", (k_demod<MODE, false>), dim3(stream_grid(ctx, ceil_div(n, 4))), dim3(256), 0,
                reinterpret_cast<const float4 *>(iq), n, reinterpret_cast<float4 *>(out), (unsigned *)nullptr);
  } else {
    TSDR_LAUNCH(ctx, MODE == DM_ABS ? "am_demod1" : "abs2_1", (k_demod1<MODE, false>), dim3(stream_grid(ctx, n)), dim3(256), 0,
                reinterpret_cast<const float2 *>(iq), n, out, (unsigned *)nullptr);
  }
  return TSDR_OK;
}

// am_demod / abs2 / invert_am's first launch on integer IQ: 16-byte vectors where both pointers allow, one sample per lane else
template <int MODE, bool TRACK_MAX>
static int demod_iq_launch(tsdr_ctx *ctx, const void *iq, const IqFmt &f, size_t n, float *out, unsigned *mx) {
  static const char *const kVec[3] = {"demod_iq_sc16", "demod_iq_sc8", "demod_iq_uc8"}, *const kOne[3] = {"demod1_iq_sc16", "demod1_iq_sc8", "demod1_iq_uc8"};
  return with_int_iqf(iqf_of(f.kind), [&](auto iqf) -> int {
    if (vec16(reinterpret_cast<const float *>(iq), out)) {
      TSDR_LAUNCH(ctx, kVec[iqf_name(iqf)], (k_demod_iq<MODE, TRACK_MAX, iqf>), dim3(stream_grid(ctx, ceil_div(n, iqf == IQF_SC16 ? 4 : 8))), dim3(256), 0,
                  reinterpret_cast<const uint4 *>(iq), n, f.scale, reinterpret_cast<float4 *>(out), mx);
    } else {
      TSDR_LAUNCH(ctx, kOne[iqf_name(iqf)], (k_demod1_iq<MODE, TRACK_MAX, iqf>), dim3(stream_grid(ctx, n)), dim3(256), 0, iq, n, f.scale, out, mx);
    }
    return TSDR_OK;
  });
}

template <int MODE>
static int demod_iq_d(tsdr_ctx *ctx, const char *kname, const void *iq, int iq_fmt, float scale, size_t n, float *out) {
  if (!ctx || (n && (!iq || !out))) return TSDR_EINVAL;
  IqFmt f;
  TSDR_IQ_ARG(ctx, kname, iq, iq_fmt, scale, f);
  TSDR_PTR_ALIGNED(ctx, kname, out, 4);
  if (iq_fmt == TSDR_IQ_CF32) return demod_d<MODE>(ctx, MODE == DM_ABS ? "am_demod" : "abs2", reinterpret_cast<const float *>(iq), n, out);
  if (n == 0) return TSDR_OK;
  return demod_iq_launch<MODE, false>(ctx, iq, f, n, out, nullptr);
}

}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_am_demod_d(tsdr_ctx *ctx, const float *iq, size_t n, float *out) { return demod_d<DM_ABS>(ctx, "am_demod", iq, n, out); }
int tsdr_abs2_d(tsdr_ctx *ctx, const float *iq, size_t n, float *out) { return demod_d<DM_ABS2>(ctx, "abs2", iq, n, out); }

int tsdr_invert_am_d(tsdr_ctx *ctx, const float *iq, size_t n, float *out) {
  if (!ctx || n == 0 || !iq || !out) return TSDR_EINVAL;  // maximum() of an empty collection throws
  TSDR_PTR_ALIGNED(ctx, "invert_am", iq, 8);
  TSDR_PTR_ALIGNED(ctx, "invert_am", out, 4);
  unsigned *mx = (unsigned *)ctx->scratch(WS_MISC, 16);
  if (!mx) return TSDR_ENOMEM;
  TSDR_HIP(ctx, hipMemsetAsync(mx, 0, 4, ctx->stream));
  if (vec16(iq, out)) {
    TSDR_LAUNCH(ctx, "invert_am_abs", (k_demod<DM_ABS, true>), dim3(stream_grid(ctx, ceil_div(n, 4))), dim3(256), 0,
                reinterpret_cast<const float4 *>(iq), n, reinterpret_cast<float4 *>(out), mx);
  } else {
    TSDR_LAUNCH(ctx, "invert_am_abs1", (k_demod1<DM_ABS, true>), dim3(stream_grid(ctx, n)), dim3(256), 0,
                reinterpret_cast<const float2 *>(iq), n, out, mx);
  }
  TSDR_LAUNCH(ctx, "invert_am_scale", k_invert, dim3(stream_grid(ctx, n)), dim3(256), 0, out, n, (const unsigned *)mx);
  return TSDR_OK;
}

int tsdr_fm_demod_d(tsdr_ctx *ctx, const float *iq, size_t n, float *out) {
  if (!ctx || (n && (!iq || !out))) return TSDR_EINVAL;
  TSDR_PTR_ALIGNED(ctx, "fm_demod", iq, 8);
  TSDR_PTR_ALIGNED(ctx, "fm_demod", out, 4);
  if (n == 0) return TSDR_OK;
  TSDR_LAUNCH(ctx, "fm_demod", k_fm, dim3(stream_grid(ctx, n)), dim3(256), 0, reinterpret_cast<const float2 *>(iq), n, out);
  return TSDR_OK;
}

int tsdr_am_demod_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, float *out) {
  return demod_iq_d<DM_ABS>(ctx, "am_demod_iq", iq, iq_fmt, scale, n, out);
}
int tsdr_abs2_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, float *out) {
  return demod_iq_d<DM_ABS2>(ctx, "abs2_iq", iq, iq_fmt, scale, n, out);
}

int tsdr_invert_am_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, float *out) {
  if (!ctx || n == 0 || !iq || !out) return TSDR_EINVAL;  // as tsdr_invert_am_d: maximum() of an empty collection throws
  IqFmt f;
  TSDR_IQ_ARG(ctx, "invert_am_iq", iq, iq_fmt, scale, f);
  TSDR_PTR_ALIGNED(ctx, "invert_am_iq", out, 4);
  if (iq_fmt == TSDR_IQ_CF32) return tsdr_invert_am_d(ctx, reinterpret_cast<const float *>(iq), n, out);
  unsigned *mx = (unsigned *)ctx->scratch(WS_MISC, 16);
  if (!mx) return TSDR_ENOMEM;
  TSDR_HIP(ctx, hipMemsetAsync(mx, 0, 4, ctx->stream));
  if (int rc = demod_iq_launch<DM_ABS, true>(ctx, iq, f, n, out, mx)) return rc;
  TSDR_LAUNCH(ctx, "invert_am_scale", k_invert, dim3(stream_grid(ctx, n)), dim3(256), 0, out, n, (const unsigned *)mx);
  return TSDR_OK;
}

int tsdr_fm_demod_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, float *out) {
  if (!ctx || (n && (!iq || !out))) return TSDR_EINVAL;
  IqFmt f;
  TSDR_IQ_ARG(ctx, "fm_demod_iq", iq, iq_fmt, scale, f);
  TSDR_PTR_ALIGNED(ctx, "fm_demod_iq", out, 4);
  if (iq_fmt == TSDR_IQ_CF32) return tsdr_fm_demod_d(ctx, reinterpret_cast<const float *>(iq), n, out);
  if (n == 0) return TSDR_OK;
  static const char *const kName[3] = {"fm_demod_iq_sc16", "fm_demod_iq_sc8", "fm_demod_iq_uc8"};
  return with_int_iqf(iqf_of(f.kind), [&](auto iqf) -> int {
    TSDR_LAUNCH(ctx, kName[iqf_name(iqf)], (k_fm_iq<iqf>), dim3(stream_grid(ctx, n)), dim3(256), 0, iq, n, f.scale, out);
    return TSDR_OK;
  });
}

int tsdr_am_demod(tsdr_ctx *ctx, const float *iq, size_t n, float *out) {
  return host_map(ctx, iq, n * 8, out, n * 4, [&](void *i, void *o) { return tsdr_am_demod_d(ctx, (const float *)i, n, (float *)o); });
}
int tsdr_abs2(tsdr_ctx *ctx, const float *iq, size_t n, float *out) {
  return host_map(ctx, iq, n * 8, out, n * 4, [&](void *i, void *o) { return tsdr_abs2_d(ctx, (const float *)i, n, (float *)o); });
}
int tsdr_invert_am(tsdr_ctx *ctx, const float *iq, size_t n, float *out) {
  if (n == 0) return TSDR_EINVAL;
  return host_map(ctx, iq, n * 8, out, n * 4, [&](void *i, void *o) { return tsdr_invert_am_d(ctx, (const float *)i, n, (float *)o); });
}
int tsdr_fm_demod(tsdr_ctx *ctx, const float *iq, size_t n, float *out) {
  return host_map(ctx, iq, n * 8, out, n * 4, [&](void *i, void *o) { return tsdr_fm_demod_d(ctx, (const float *)i, n, (float *)o); });
}

}  // extern "C"
