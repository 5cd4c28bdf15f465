// fft_dev.h -- device helpers shared by the power-of-two (fft.hip) and mixed-radix (fft_mixed.hip) engines.
#pragma once
#include <utility>

#include "common.h"

namespace tsdr {

enum { FFT_STRIDED = 0, FFT_LAST = 1, FFT_ROWS = 2 };

// Complex arithmetic on the packed-f32 pipe (v_pk_*_f32: two f32 lanes per instruction at the rate of one): the FFT
// kernels issue VALU instructions 70 % of the time, and a complex product is two instructions this way instead of four
// (six without explicit FMAs -- the library is built with -ffp-contract=off for the bit-exact kernels).  The compiler
// finds the packed add on its own but not the product's source modifiers: t = (-a.y b.y, a.y b.x) takes the high half of
// a twice, b swapped with its new low half negated; r = (a.x, a.x) * b + t.  Same roundings as
// (fma(a.x, b.x, -(a.y b.y)), fma(a.x, b.y, a.y b.x)).
typedef float tsdr_v2f __attribute__((ext_vector_type(2)));
__device__ inline tsdr_v2f c2v(float2 a) { return tsdr_v2f{a.x, a.y}; }
__device__ inline float2 v2c(tsdr_v2f a) { return make_float2(a.x, a.y); }
__device__ inline float2 cmul(float2 a, float2 b) {
  const tsdr_v2f av = c2v(a), bv = c2v(b);
  tsdr_v2f t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(t) : "v"(av), "v"(bv));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "=v"(r) : "v"(av), "v"(bv), "v"(t));
  return v2c(r);
}
__device__ inline float2 cadd(float2 a, float2 b) { return v2c(c2v(a) + c2v(b)); }
__device__ inline float2 csub(float2 a, float2 b) { return v2c(c2v(a) - c2v(b)); }
__device__ inline float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
// p - i q = (p.x + q.y, p.y - q.x) and p + i q = (p.x - q.y, p.y + q.x): one packed add with q's halves swapped and one
// of them negated by source modifiers
__device__ inline float2 cadd_mi(float2 p, float2 q) {
  tsdr_v2f r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(c2v(p)), "v"(c2v(q)));
  return v2c(r);
}
__device__ inline float2 cadd_pi(float2 p, float2 q) {
  tsdr_v2f r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(c2v(p)), "v"(c2v(q)));
  return v2c(r);
}
// a * s and a * s + c for a real s (both halves by the same factor)
__device__ inline float2 cscale(float2 a, float s) { return v2c(c2v(a) * tsdr_v2f{s, s}); }
__device__ inline float2 cfma_s(float2 a, float s, float2 c) { return v2c(__builtin_elementwise_fma(c2v(a), tsdr_v2f{s, s}, c2v(c))); }
// a * (kr + i ki) for a compile-time constant: the constant sits in a scalar register pair (no VGPRs, no per-use moves)
__device__ inline float2 cmul_k(float2 a, float kr, float ki) {
  const tsdr_v2f av = c2v(a), kv = tsdr_v2f{kr, ki};
  tsdr_v2f t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(t) : "v"(av), "s"(kv));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "=v"(r) : "v"(av), "s"(kv), "v"(t));
  return v2c(r);
}

// Forward DFT of N = 2, 4, 8 or 16 points held in registers: radix-2 decimation in frequency with the
// twiddles as literals (trivial ones special-cased), result in bit-reversed order (X[k] at v[brev<N>(k)]).
__device__ constexpr float kCos16[8] = {1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f,
                                        0.0f, -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128674f};
__device__ constexpr float kSin16[8] = {0.0f, 0.38268343236508977f, 0.70710678118654752f, 0.92387953251128674f,
                                        1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f};

template <int N, int I>
__device__ inline float2 mul_w(float2 d) {  // d * exp(-2*pi*i*I/N), 0 <= I < N/2
  constexpr int E = I * (16 / N);
  if constexpr (E == 0) {
    return d;
  } else if constexpr (E == 4) {
    return make_float2(d.y, -d.x);
  } else if constexpr (E == 2) {
    return cscale(cadd_mi(d, d), kCos16[2]);    // ((d.x + d.y), (d.y - d.x)) / sqrt 2
  } else if constexpr (E == 6) {
    return cscale(cadd_pi(d, d), -kCos16[2]);   // ((d.y - d.x), -(d.x + d.y)) / sqrt 2
  } else {
    return cmul_k(d, kCos16[E], -kSin16[E]);
  }
}

template <int N, int I>
__device__ inline void bfly(float2 *v) {
  const float2 a = v[I], b = v[I + N / 2];
  v[I] = cadd(a, b);
  v[I + N / 2] = mul_w<N, I>(csub(a, b));
}

template <int N, int... I>
__device__ inline void dif_stage(float2 *v, std::integer_sequence<int, I...>) {
  (bfly<N, I>(v), ...);
}

template <int N>
__device__ inline void reg_dft(float2 *v) {
  if constexpr (N >= 2) {
    dif_stage<N>(v, std::make_integer_sequence<int, N / 2>{});
    reg_dft<N / 2>(v);
    reg_dft<N / 2>(v + N / 2);
  }
}

template <int N>
__device__ constexpr int brev(int k) {
  int r = 0;
  for (int b = 1; b < N; b <<= 1) { r = (r << 1) | (k & 1); k >>= 1; }
  return r;
}

// Twiddles without tables.  A gathered table read costs one L1 tag cycle per distinct line per lane and made
// the passes gather-bound, so the phase is reduced to an octant o (0..7) plus x in [0, 1] -- exactly, in
// integers, for power-of-two N -- and sin/cos(pi/4 * x) come from degree-7/8 polynomials (Chebyshev
// interpolants in x^2; measured error <= 8.6e-8 absolute over all f32 x, i.e. <= 1.5 ulp).
// tw_octant: exp(-i*pi/4*(o + x)) for even o, exp(-i*pi/4*(o + 1 - x)) for odd o (the caller mirrors x).
__device__ inline float2 tw_octant(unsigned o, float x) {
  const float u = x * x;
  const float sn = fmaf(fmaf(fmaf(-3.595429006963968e-05f, u, 0.0024900068528950214f), u, -0.08074543625116348f), u,
                        0.7853981852531433f) * x;
  const float cs = fmaf(fmaf(fmaf(fmaf(3.5297971407999285e-06f, u, -0.0003259385994169861f), u, 0.015854325145483017f), u,
                             -0.3084251284599304f), u, 1.0f);
  const bool swap = ((o + 1u) >> 1) & 1u;
  float cr = swap ? sn : cs, sr = swap ? cs : sn;
  if ((o + 2u) & 4u) cr = -cr;
  if (!(o & 4u)) sr = -sr;
  return make_float2(cr, sr);
}

// exp(-2*pi*i*e / 2^L) for 0 <= e < 2^L, 2 <= L <= 31
__device__ inline float2 tw_unit(unsigned e, int L) {
  const unsigned q = e << (32 - L);
  const unsigned o = q >> 29;
  unsigned r = q & 0x1FFFFFFFu;
  if (o & 1u) r = 0x20000000u - r;
  return tw_octant(o, (float)r * 0x1p-29f);
}

// exp(-2*pi*i*q/2^32), and the phase q = floor(2^32 * e/N) (within 2 units) from inv = floor(2^64/N) = hi:lo
__device__ inline float2 tw_q32(unsigned q) {
  const unsigned o = q >> 29;
  unsigned r = q & 0x1FFFFFFFu;
  if (o & 1u) r = 0x20000000u - r;
  return tw_octant(o, (float)r * 0x1p-29f);
}
__device__ inline unsigned phase_q32(unsigned e, unsigned inv_hi, unsigned inv_lo) {
  return e * inv_hi + __umulhi(e, inv_lo);
}

__device__ inline float2 conj_if(float2 v, unsigned smask) {  // smask = 0x80000000 for the inverse transform
  return make_float2(v.x, __uint_as_float(__float_as_uint(v.y) ^ smask));
}

// element g of the (single) transform for the fused loaders of the first pass:
//   SRC_C2C   in[g]
//   SRC_REAL  (x[2g], x[2g+1])            real f32 sequence of src_n samples packed two per complex, zero beyond
//   SRC_IQPOW (|iq[2g]|^2, |iq[2g+1]|^2)  the same with x = abs2.(iq) formed on the fly (GUI.jl:70)
//   SRC_IQPOW_SC16 / _SC8 / _UC8  the same from integer IQ storage (int16, int8, uint8 pairs): every sample is converted by
//             common.h's cvt_* (the one product by `scale`, which arrives in the loader-parameter slot), then abs2_c.
//             The two samples of g are one 8-byte (sc16) or 4-byte (8-bit) load: the base must be aligned to that.
//   SRC_IQ_SC16 / _SC8 / _UC8  in[g] read from integer IQ storage (one sample-aligned load, converted by common.h's cvt_* with
//             the scale in the loader-parameter slot): ComplexF32 input of getSpectrum / getWelch / getWaterfall as the SDR
//             stored it.  Element-wise like SRC_C2C, so these also serve batched transforms (g runs over the whole batch).
//   SRC_POWER Y[g] of the autocorrelation: `in` = Z, the length-src_n transform of a packed real
//             sequence; Y is the packed spectrum whose inverse transform (times 1/2) is the real sequence with
//             spectrum |X|^2 (see k_ac_power, which this loader replaces: one launch and a 2 x 8*Mc-byte round
//             trip less)
//   SRC_STUFF (x[g / up], 0) when up divides g, else 0: the zero-stuffed real input of the resampler (Resampler.jl:
//             upsampling by inserting up - 1 zeros), src_n = up -- k_stuff without its pass
//   SRC_RE0   (x[g], 0): a real f32 sequence as complex input (getSpectrum of a real signal) -- k_r2c without its pass
//   SRC_MULH  in[g] * aux[g], aux = ComplexF64 (double2 behind the float2 pointer): the resampler's frequency-domain filter
//             applied while the inverse transform loads -- evaluated in f64 and rounded to ComplexF32 (Resampler.jl:51-53)
//   SRC_ABS2  (|in[g]|^2, 0): the power spectrum of a COMPLEX sequence while the inverse transform of its autocorrelation
//             loads (autocorr_cplx.hip) -- pointwise, re*re + im*im, a zero imaginary part; SRC_POWER's place on that route
enum { SRC_C2C = 0, SRC_REAL = 1, SRC_IQPOW = 2, SRC_POWER = 3, SRC_STUFF = 4, SRC_MULH = 5, SRC_RE0 = 6, SRC_IQPOW_SC16 = 7, SRC_IQPOW_SC8 = 8, SRC_IQPOW_UC8 = 9,
       SRC_IQ_SC16 = 10, SRC_IQ_SC8 = 11, SRC_IQ_UC8 = 12, SRC_ABS2 = 13 };
inline bool src_is_int_iq(int src_mode) { return src_mode >= SRC_IQPOW_SC16 && src_mode <= SRC_IQ_UC8; }
inline bool src_is_cplx_int(int src_mode) { return src_mode >= SRC_IQ_SC16 && src_mode <= SRC_IQ_UC8; }

// What the per-function host paths (spectra, tsdr_fft_c2c, autocorrelations) are handed: a pointer, what kind of samples it points
// to and, for integer IQ, their factor.  The IQ kinds are 1 + TSDR_IQ_*; k_ac_pack / k_pc_pack (autocorr.hip) take the kind as a
// kernel argument.  Every other encoding of "which samples" -- loader modes, row-kernel modes, template arguments -- is a function
// of the kind, below and in common.h (iqf_of), each pinned value by value.
enum SigKind { SIG_REAL = 0, SIG_CF32 = 1, SIG_SC16 = 2, SIG_SC8 = 3, SIG_UC8 = 4 };
struct SigSrc {
  const void *p; int kind; float scale;
  bool is_int() const { return kind >= SIG_SC16; }
  size_t bytes() const { return kind == SIG_CF32 ? 8 : kind == SIG_SC8 || kind == SIG_UC8 ? 2 : 4; }   // per element
  IqFmt iq() const { return IqFmt{is_int() ? kind - SIG_CF32 : IQK_CF32, scale}; }
  const float *f32() const { return reinterpret_cast<const float *>(p); }
  const float2 *c32() const { return reinterpret_cast<const float2 *>(p); }
};
inline SigSrc sig_f32(const float *x, int is_complex) { return SigSrc{x, is_complex ? SIG_CF32 : SIG_REAL, 1.0f}; }
inline SigSrc sig_iq(const void *iq, const IqFmt &f) { return SigSrc{iq, SIG_CF32 + f.kind, f.scale}; }
static_assert(SIG_CF32 == 1 + IQK_CF32 && SIG_SC16 == 1 + IQK_SC16 && SIG_SC8 == 1 + IQK_SC8 && SIG_UC8 == 1 + IQK_UC8, "IQ kinds are 1 + TSDR_IQ_*");

// element-wise loader of a first pass: in[g] of that kind as a complex value
constexpr int src_of(int kind) { return kind == SIG_REAL ? SRC_RE0 : kind == SIG_CF32 ? SRC_C2C : SRC_IQ_SC16 + (kind - SIG_SC16); }
static_assert(src_of(SIG_REAL) == 6 && src_of(SIG_CF32) == 0 && src_of(SIG_SC16) == 10 && src_of(SIG_SC8) == 11 && src_of(SIG_UC8) == 12, "SRC_RE0 / SRC_C2C / SRC_IQ_*");
// packing loader of the real autocorrelation: two samples (or two abs2 of IQ samples) per complex value
constexpr int srcpow_of(int kind) { return kind == SIG_REAL ? SRC_REAL : kind == SIG_CF32 ? SRC_IQPOW : SRC_IQPOW_SC16 + (kind - SIG_SC16); }
static_assert(srcpow_of(SIG_REAL) == 1 && srcpow_of(SIG_CF32) == 2 && srcpow_of(SIG_SC16) == 7 && srcpow_of(SIG_SC8) == 8 && srcpow_of(SIG_UC8) == 9, "SRC_REAL / SRC_IQPOW*");
// MixDesc::rows_real of the whole-row kernels (fft_mixed.hip): the integer kinds keep their SigKind value
enum { ROWS_CF32 = 0, ROWS_REAL = 1, ROWS_SC16 = 2, ROWS_SC8 = 3, ROWS_UC8 = 4 };
constexpr int rows_of(int kind) { return kind == SIG_REAL ? ROWS_REAL : kind == SIG_CF32 ? ROWS_CF32 : kind; }
static_assert(rows_of(SIG_REAL) == 1 && rows_of(SIG_CF32) == 0 && rows_of(SIG_SC16) == 2 && rows_of(SIG_SC8) == 3 && rows_of(SIG_UC8) == 4, "ROWS_*");
static_assert(iqf_of(IQK_CF32) == 0 && iqf_of(IQK_SC16) == 1 && iqf_of(IQK_SC8) == 3 && iqf_of(IQK_UC8) == 4 && IQF_RT == 2, "IQF_*");

// inv_m8 is the loader's one f64 parameter: 8/M for SRC_POWER with M not a power of two, the f32 scale for integer IQ, else 0
// tw_frac below (needed by the SRC_POWER loader when M = 2*Mc is not a power of two)
__device__ inline float2 tw_frac(unsigned e, double inv_n8);

__device__ inline float2 fft_load(const float2 *__restrict__ in, int src_mode, unsigned long long src_n, size_t g,
                                  double inv_m8 = 0.0, const float2 *__restrict__ aux = nullptr) {
  if (src_mode == SRC_C2C) return in[g];
  if (src_mode == SRC_MULH) {
    const float2 x = in[g];
    const double2 h = reinterpret_cast<const double2 *>(aux)[g];
    return make_float2((float)((double)x.x * h.x - (double)x.y * h.y), (float)((double)x.x * h.y + (double)x.y * h.x));
  }
  if (src_mode == SRC_RE0) return make_float2(reinterpret_cast<const float *>(in)[g], 0.f);
  if (src_mode == SRC_STUFF) {
    const size_t q = g / (size_t)src_n;
    return q * (size_t)src_n == g ? make_float2(reinterpret_cast<const float *>(in)[q], 0.f) : make_float2(0.f, 0.f);
  }
  if (src_mode == SRC_POWER) {
    const size_t Mc = (size_t)src_n;
    const float2 a = in[g], b = in[g ? Mc - g : 0];
    const float2 E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
    const float2 D = make_float2(0.5f * (a.x - b.x), 0.5f * (a.y + b.y));  // (Z[g] - conj Z[Mc-g]) / 2
    const float2 O = make_float2(D.y, -D.x);                                // -i*D
    // W_M^g, M = 2*Mc: exact octant split for a power of two, f64 phase (inv_m8 = 8/M) otherwise
    const float2 W = inv_m8 == 0.0 ? tw_unit((unsigned)g, 64 - __clzll((unsigned long long)Mc)) : tw_frac((unsigned)g, inv_m8);
    const float2 WO = cmul(W, O);
    const float2 X0 = make_float2(E.x + WO.x, E.y + WO.y), X1 = make_float2(E.x - WO.x, E.y - WO.y);
    const float P0 = X0.x * X0.x + X0.y * X0.y, P1 = X1.x * X1.x + X1.y * X1.y;
    const float sum = P0 + P1, dif = P0 - P1;
    return make_float2(sum + dif * W.y, dif * W.x);  // (P + P') + i conj(W) (P - P')
  }
  if (src_mode == SRC_ABS2) {
    const float2 a = in[g];
    return make_float2(a.x * a.x + a.y * a.y, 0.f);
  }
  if (src_mode >= SRC_IQ_SC16) {
    if (src_mode == SRC_IQ_SC16) return cvt_sc16(reinterpret_cast<const short2 *>(in)[g], (float)inv_m8);
    const unsigned v = reinterpret_cast<const unsigned short *>(in)[g];
    return src_mode == SRC_IQ_SC8 ? cvt_sc8(v, (float)inv_m8) : cvt_uc8(v, (float)inv_m8);
  }
  const unsigned long long i0 = 2ull * g;
  if (i0 >= src_n) return make_float2(0.f, 0.f);  // zero padding is never read
  if (src_mode == SRC_REAL) {
    const float *x = reinterpret_cast<const float *>(in);
    return make_float2(x[i0], i0 + 1 < src_n ? x[i0 + 1] : 0.f);
  }
  if (src_mode == SRC_IQPOW) {
    const float4 z = reinterpret_cast<const float4 *>(in)[g];  // iq[2g], iq[2g+1]
    return make_float2(z.x * z.x + z.y * z.y, i0 + 1 < src_n ? z.z * z.z + z.w * z.w : 0.f);
  }
  const float sc = (float)inv_m8;
  float2 a, b;
  if (src_mode == SRC_IQPOW_SC16) {
    const short4 v = reinterpret_cast<const short4 *>(in)[g];
    a = cvt_sc16(make_short2(v.x, v.y), sc); b = cvt_sc16(make_short2(v.z, v.w), sc);
  } else {
    const unsigned v = reinterpret_cast<const unsigned *>(in)[g];
    if (src_mode == SRC_IQPOW_SC8) { a = cvt_sc8(v & 0xFFFFu, sc); b = cvt_sc8(v >> 16, sc); }
    else { a = cvt_uc8(v & 0xFFFFu, sc); b = cvt_uc8(v >> 16, sc); }
  }
  return make_float2(abs2_c(a.x, a.y), i0 + 1 < src_n ? abs2_c(b.x, b.y) : 0.f);
}

// one element of a whole-row kernel's integer IQ input (MixDesc::rows_real = ROWS_SC16 / _SC8 / _UC8, the scale in MixDesc::src_w8).
// `e` is the element's index from the buffer's start.  (The twin of fft_load's SRC_IQ_* branch: folded into one run-time loader
// the compiler emits other code for the pass kernels, so the two stay.)
__device__ inline float2 rows_load_int(const float2 *__restrict__ in, int rows_real, size_t e, float scale) {
  if (rows_real == ROWS_SC16) return cvt_sc16(reinterpret_cast<const short2 *>(in)[e], scale);
  const unsigned v = reinterpret_cast<const unsigned short *>(in)[e];
  return rows_real == ROWS_SC8 ? cvt_sc8(v, scale) : cvt_uc8(v, scale);
}

// exp(-2*pi*i*e/N) for any N: inv_n8 = 8/N in f64, 0 <= e < N.  The phase e/N is formed in f64 (relative error
// 2^-52), so the octant split is exact to ~1e-16 of a turn.
__device__ inline float2 tw_frac(unsigned e, double inv_n8) {
  const double ph = (double)e * inv_n8;
  const unsigned o = (unsigned)ph;
  const double f = ph - (double)o;
  const float x = (float)((o & 1u) ? 1.0 - f : f);
  return tw_octant(o & 7u, x);
}

// Epilogues of the last pass (o = index of the complex output x within its transform):
//   EPI_AC     autocorrelation (Autocorrelations.jl:33-36): x holds the real lags (2o, 2o+1); lags k0 <= k < k0+cnt leave
//              as abs2 (and 10log10) in f32 -- k_ac_finish without the round trip
//   EPI_REAL   out[o] = gain * real(x) for o < cnt: the resampler's `2*upCoeff*real.(ifft)` (Resampler.jl) without k_real_scale
//   EPI_SPEC   getSpectrum (GetSpectrum.jl:21-30): out[fftshift position of o] = abs2(x) or 10log10(abs2(x)); cnt = N, k0 = N div 2
//              With amax_keys set the same pass also finds findmax over out[amax_lo .. amax_lo + amax_cnt) (GUI.jl:79 on
//              the zoom window, Autocorrelations.jl:42-53): every thread keeps the best packed key of what it stores and a
//              workgroup contributes ONE relaxed atomicMax to one of kAmaxSlots words (epi_argmax_finish) -- no fence, no
//              arrival counter: a release fence per workgroup writes its freshly stored lags back through L2 and tripled
//              the pass (measured 12 -> 38 us at C2).  A one-wavefront launch behind the pass folds the slots and hands
//              the result to the host (k_amax_publish); the separate pass over the lags is gone.
//   EPI_CAC    autocorrelation of a COMPLEX sequence (autocorr_cplx.hip): x is the one complex lag o; lags k0 <= o < k0+cnt
//              leave as abs2 (and 10log10) at out[o - k0], order and rounding as EPI_SPEC; the fused findmax as EPI_AC
enum { EPI_NONE = 0, EPI_AC = 1, EPI_REAL = 2, EPI_SPEC = 3, EPI_CAC = 4 };
struct FftEpilogue {
  float *out = nullptr;
  unsigned long long k0 = 0, cnt = 0;
  int log_scale = 0;
  int kind = EPI_AC;
  float gain = 1.0f;
  // fused findmax (EPI_AC and EPI_CAC)
  unsigned long long *amax_keys = nullptr;  // kAmaxSlots device words, zero on entry
  unsigned long long amax_lo = 0, amax_cnt = 0;
};
constexpr int kAmaxSlots = 16;

// findmax: first maximum, NaN maximal -- value bits made order-preserving, index complemented so the smallest wins ties
__device__ inline unsigned long long argmax_key(float v, unsigned idx) {
  unsigned u = (v != v) ? 0x7FC00000u : __float_as_uint(v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}

__device__ inline void epilogue_store(const FftEpilogue &e, size_t o, float2 x, unsigned long long &best) {
  if (e.kind == EPI_REAL) {
    if (o < e.cnt) e.out[o] = e.gain * x.x;
    return;
  }
  if (e.kind == EPI_SPEC) {
    if (o < e.cnt) {
      size_t j = o + e.k0;
      if (j >= e.cnt) j -= e.cnt;
      const float p = x.x * x.x + x.y * x.y;
      e.out[j] = e.log_scale ? 10.0f * log10f(p) : p;
    }
    return;
  }
  if (e.kind == EPI_CAC) {
    const unsigned long long i = (unsigned long long)o - e.k0;  // (wraps to huge when below k0)
    if (i < e.cnt) {
      const float p = x.x * x.x + x.y * x.y, v = e.log_scale ? 10.0f * log10f(p) : p;
      e.out[i] = v;
      if (i - e.amax_lo < e.amax_cnt) { const unsigned long long k = argmax_key(v, (unsigned)(i - e.amax_lo)); best = k > best ? k : best; }
    }
    return;
  }
  const unsigned long long i0 = 2ull * o - e.k0, i1 = i0 + 1ull;  // (wraps to huge when below k0)
  if (i0 < e.cnt) {
    const float p = x.x * x.x, v = e.log_scale ? 10.0f * log10f(p) : p;
    e.out[i0] = v;
    if (i0 - e.amax_lo < e.amax_cnt) { const unsigned long long k = argmax_key(v, (unsigned)(i0 - e.amax_lo)); best = k > best ? k : best; }
  }
  if (i1 < e.cnt) {
    const float p = x.y * x.y, v = e.log_scale ? 10.0f * log10f(p) : p;
    e.out[i1] = v;
    if (i1 - e.amax_lo < e.amax_cnt) { const unsigned long long k = argmax_key(v, (unsigned)(i1 - e.amax_lo)); best = k > best ? k : best; }
  }
}
__device__ inline void epilogue_store(const FftEpilogue &e, size_t o, float2 x) {
  unsigned long long best = 0ull;
  epilogue_store(e, o, x, best);
}

// End of a last pass with a fused findmax: called by every thread of a workgroup (wkeys: one LDS word per wavefront).
__device__ inline void epi_argmax_finish(const FftEpilogue &e, unsigned long long best, unsigned long long *wkeys, int nwaves) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off, 64);
    best = o > best ? o : best;
  }
  if ((threadIdx.x & 63) == 0) wkeys[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long b = wkeys[0];
    for (int i = 1; i < nwaves; ++i) b = wkeys[i] > b ? wkeys[i] : b;
    if (b) __hip_atomic_fetch_max(e.amax_keys + (blockIdx.x & (kAmaxSlots - 1)), b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One transform request: `batch` contiguous transforms of n = 2^a 3^b 5^c points, in -> out (they may alias; neither may be a
// WS_FFT_B buffer).  The first pass can load through a fused loader (src_mode / src_n / src_aux / src_scale, see fft_load), the last
// pass can store only the first `keep` complex outputs per transform (0 = all) or leave through an epilogue.  Loaders and epilogues
// need one transform (batch == 1; the element-wise integer IQ loaders: any batch) of more than one pass.
struct FftReq {
  const float2 *in = nullptr;
  float2 *out = nullptr;
  size_t n = 0, batch = 1;
  int dir = -1;                        // -1 forward, +1 inverse
  float scale = 1.0f;
  int src_mode = SRC_C2C;
  size_t src_n = 0;
  const float2 *src_aux = nullptr;
  float src_scale = 1.0f;              // integer IQ loaders: the samples' factor
  size_t keep = 0;
  const FftEpilogue *epi = nullptr;
  // the first pass reads `s` through loader `mode` (src_of / srcpow_of of its kind)
  FftReq &load(const SigSrc &s, int mode) { in = s.c32(); src_mode = mode; src_scale = s.scale; return *this; }
};

// the options a plan depends on, by value: "fft_no_mix2", "fft_big", the device's CU count
struct FftOpts { int no_mix2 = 0, big = 1, cu_count = 0; };
inline FftOpts fft_opts(const tsdr_ctx *ctx) { FftOpts o; o.no_mix2 = ctx->opt_fft_no_mix2; o.big = ctx->opt_fft_big; o.cu_count = ctx->cu_count; return o; }

// host entry points of the engines (fft.hip, fft_mixed.hip; what each call launches is decided by fft_plan.h)
int fft_run(tsdr_ctx *ctx, const FftReq &q);   // one 2^a 3^b 5^c request, on the engine its length takes
// the circular autocorrelation of 2 * q.n real samples with the fused middle (fft_plan.h:plan_autocorr; Zbuf: q.n complex values);
// *done = false (nothing launched) when this length has none
int fft_run_autocorr(tsdr_ctx *ctx, const FftReq &q, float2 *Zbuf, bool *done);
unsigned fft_rows_welch_parts(tsdr_ctx *ctx);
// whole-row kernels (fft_mixed.hip): the rows are read as stored, whatever their kind (fft_rows_store: not real ones)
int fft_rows_welch(tsdr_ctx *ctx, const SigSrc &sig, size_t N, size_t nbSeg, float *part, unsigned *nparts, bool *did);
int fft_rows_store(tsdr_ctx *ctx, const SigSrc &in, float2 *out, size_t N, size_t batch, int dir, float scale, bool *did);
int fft_rows_waterfall(tsdr_ctx *ctx, const SigSrc &sig, size_t N, size_t nbSeg, double *wf, bool *did);
int fft_rows1024(tsdr_ctx *ctx, const float2 *in, float2 *out, size_t batch, int dir, float scale);   // spectrum.hip
// fft.hip: `batch` contiguous transforms of any length n from any kind of samples (integer IQ: forward only)
int fft_any(tsdr_ctx *ctx, SigSrc x, float2 *out, size_t n, size_t batch, int dir);
int fft64_d(tsdr_ctx *ctx, double2 *data, double2 *scratch, size_t N, int dir);   // fft64.hip
int resampler_init_kind(tsdr_ctx *ctx, size_t bufferSize, int upCoeff, bool f64, tsdr_resampler **out);   // spectrum.hip
int fft_mixed_passes(tsdr_ctx *ctx, size_t N, size_t batch);   // passes the mixed-radix engine takes for `batch` transforms of N points (0: not its length)
bool fft_mixed_ok(size_t N);
int fft_passes(size_t N);            // launches a length-N transform takes (0: not a 2^a 3^b 5^c length)
int ensure_tw_small(tsdr_ctx *ctx);  // builds ctx->tw_small: W_4096^e for e < 4096
int get_tw(tsdr_ctx *ctx, int logN, TwTable **out);   // fft.hip: the two-level table of W_N^e, N = 2^logN, built at first use

}  // namespace tsdr
