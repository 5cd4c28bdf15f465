// fft_mixed.hip -- complex f32 FFT for lengths N = 2^a * 3^b * 5^c (FFTW.jl fft/ifft semantics).
//
// Sample rates in this domain are decimal (20 MS/s, 200 MS/s ...), so the transform lengths the reference asks
// for -- two refresh periods of samples for the autocorrelation (Autocorrelations.jl:27), spectrum windows,
// resampler blocks -- are of the form 2^a * 5^b far more often than 2^a (4e6 = 2^8 * 5^6).  Padding such a length
// to a power of two doubles the bytes every pass moves; this engine transforms it natively.
//
// Same multi-pass structure as fft.hip: N = R_1 * ... * R_p with every R_i <= 256, one launch per factor, pass
// i < p a length-R_i DFT at stride B_i = R_{i+1}..R_p followed by the twiddle W_{P_i R_i R_{i+1}}^(n_{i+1} K),
// the last pass contiguous and written in natural order.  The differences:
//   * the radices are arbitrary, so tile coordinates come from integer divisions by launch constants instead of
//     shifts, tiles are ragged at the end of a row, and twiddle phases e/N are 32-bit fixed-point fractions from a
//     64-bit reciprocal (phase_q32);
//   * inside a tile the length-R DFT is an in-place decimation-in-frequency over LDS with stage radices
//     from {2, 3, 4, 5, 8, 9, 10, 16, 25} (register DFTs), and the mixed-radix digit reversal is undone through a
//     position -> frequency map while storing.
// The factors are ordered so that the last one carries the factors of two: every stride B_i is then a multiple
// of 16 elements and the T-wide runs of a tile stay 128-byte aligned.
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "fft_plan.h"

namespace tsdr {

// a = k_1*(R_2..R_m) + ... + k_m  ->  k_1*W_1 + ... + k_m*W_m  (uniform per workgroup: scalar code)
__device__ inline unsigned digit_swap_g(unsigned a, int m, const unsigned *R, const unsigned *W) {
  unsigned K = 0;
  for (int j = m - 1; j >= 0; --j) {
    const unsigned q = a / R[j];
    K += (a - q * R[j]) * W[j];
    a = q;
  }
  return K;
}

// x * exp(-2*pi*i*K/N) with the constant taken from a literal table
__device__ constexpr float kCos25[17] = {1.f, 0.96858316112863108f, 0.87630668004386358f, 0.72896862742141155f, 0.53582679497899655f,
    0.30901699437494745f, 0.062790519529313527f, -0.1873813145857246f, -0.42577929156507272f, -0.63742398974868975f,
    -0.80901699437494734f, -0.92977648588825135f, -0.99211470131447776f, -0.99211470131447788f, -0.92977648588825146f,
    -0.80901699437494778f, -0.63742398974868952f};
__device__ constexpr float kSin25[17] = {0.f, 0.24868988716485479f, 0.48175367410171532f, 0.68454710592868862f, 0.84432792550201508f,
    0.95105651629515353f, 0.99802672842827156f, 0.98228725072868872f, 0.90482705246601947f, 0.77051324277578925f,
    0.58778525229247325f, 0.36812455268467814f, 0.12533323356430454f, -0.12533323356430429f, -0.36812455268467792f,
    -0.58778525229247269f, -0.77051324277578936f};
__device__ constexpr float kCos10[5] = {1.f, 0.80901699437494745f, 0.30901699437494745f, -0.30901699437494734f, -0.80901699437494734f};
__device__ constexpr float kSin10[5] = {0.f, 0.58778525229247314f, 0.95105651629515353f, 0.95105651629515364f, 0.58778525229247325f};
__device__ constexpr float kCos20[13] = {1.0f, 0.9510565162951535f, 0.8090169943749475f, 0.5877852522924731f, 0.30901699437494745f, 6.123233995736766e-17f, -0.30901699437494734f, -0.587785252292473f, -0.8090169943749473f, -0.9510565162951535f, -1.0f, -0.9510565162951538f, -0.8090169943749476f};
__device__ constexpr float kSin20[13] = {0.0f, 0.3090169943749474f, 0.5877852522924731f, 0.8090169943749475f, 0.9510565162951535f, 1.0f, 0.9510565162951536f, 0.8090169943749475f, 0.5877852522924732f, 0.3090169943749475f, 1.2246467991473532e-16f, -0.3090169943749469f, -0.587785252292473f};
__device__ constexpr float kCos9[5] = {1.f, 0.76604444311897801f, 0.17364817766693041f, -0.5f, -0.93969262078590832f};
__device__ constexpr float kSin9[5] = {0.f, 0.64278760968653925f, 0.98480775301220802f, 0.86602540378443871f, 0.34202014332566888f};

template <int N, int K>
__device__ inline float2 mul_c(float2 x) {
  if constexpr (K == 0) {
    return x;
  } else {
    constexpr float c = N == 25 ? kCos25[K] : N == 20 ? kCos20[K] : N == 10 ? kCos10[K] : kCos9[K];
    constexpr float sn = N == 25 ? kSin25[K] : N == 20 ? kSin20[K] : N == 10 ? kSin10[K] : kSin9[K];
    return cmul_k(x, c, -sn);
  }
}

// forward DFT of r points, natural order, in place
template <int r>
__device__ inline void dft_nat(float2 *x);

// r = P*Q as two register steps: n = Q'*a + b ... X[c + P*d] = sum_b W_Q^(b d) W_r^(b c) sum_a W_P^(a c) x[Q*a + b]
template <int P, int Q, int B, int... C>
__device__ inline void two_step_col(const float2 *x, float2 *y, std::integer_sequence<int, C...>) {
  float2 t[P];
#pragma unroll
  for (int a = 0; a < P; ++a) t[a] = x[Q * a + B];
  dft_nat<P>(t);
  ((y[Q * C + B] = mul_c<P * Q, B * C>(t[C])), ...);
}
template <int P, int Q, int... B>
__device__ inline void two_step_cols(const float2 *x, float2 *y, std::integer_sequence<int, B...>) {
  (two_step_col<P, Q, B>(x, y, std::make_integer_sequence<int, P>{}), ...);
}
template <int P, int Q>
__device__ inline void dft_two_step(float2 *x) {
  float2 y[P * Q];
  two_step_cols<P, Q>(x, y, std::make_integer_sequence<int, Q>{});  // y[Q*c + b]
#pragma unroll
  for (int c = 0; c < P; ++c) {
    float2 t[Q];
#pragma unroll
    for (int b = 0; b < Q; ++b) t[b] = y[Q * c + b];
    dft_nat<Q>(t);
#pragma unroll
    for (int d = 0; d < Q; ++d) x[c + P * d] = t[d];
  }
}

template <int r>
__device__ inline void dft_nat(float2 *x) {
  if constexpr (r == 3) {
    const float s = 0.86602540378443865f;
    const float2 t = cadd(x[1], x[2]), d = csub(x[1], x[2]);
    const float2 m = cfma_s(t, -0.5f, x[0]);
    const float2 q = cscale(d, s);
    x[0] = cadd(x[0], t);
    x[1] = cadd_mi(m, q);  // m - i s d
    x[2] = cadd_pi(m, q);
  } else if constexpr (r == 5) {
    const float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;
    const float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;
    const float2 a1 = cadd(x[1], x[4]), a2 = cadd(x[2], x[3]), b1 = csub(x[1], x[4]), b2 = csub(x[2], x[3]);
    // (packed: every line below is one instruction per complex value)
    const float2 p1 = cadd(x[0], cfma_s(a1, c1, cscale(a2, c2)));
    const float2 p2 = cadd(x[0], cfma_s(a1, c2, cscale(a2, c1)));
    const float2 q1 = cfma_s(b1, s1, cscale(b2, s2));
    const float2 q2 = cfma_s(b1, s2, cscale(b2, -s1));
    x[0] = cadd(x[0], cadd(a1, a2));
    x[1] = cadd_mi(p1, q1);  // p1 - i q1
    x[4] = cadd_pi(p1, q1);
    x[2] = cadd_mi(p2, q2);
    x[3] = cadd_pi(p2, q2);
  } else if constexpr (r == 25) {
    dft_two_step<5, 5>(x);
  } else if constexpr (r == 20) {
    dft_two_step<5, 4>(x);
  } else if constexpr (r == 10) {
    dft_two_step<5, 2>(x);
  } else if constexpr (r == 9) {
    dft_two_step<3, 3>(x);
  } else {
    reg_dft<r>(x);
    float2 y[r];
#pragma unroll
    for (int c = 0; c < r; ++c) y[c] = x[brev<r>(c)];
#pragma unroll
    for (int c = 0; c < r; ++c) x[c] = y[c];
  }
}

// One DIF stage of radix r on sub-transforms of length L: for every group g and j < Q = L/r
//   y_c = sum_m x[g*L + j + m*Q] W_r^(m c),   x[g*L + j + c*Q] <- y_c * W_L^(j c)
template <int r>
__device__ inline void mix_stage(float2 *buf, const float2 *twR, unsigned R, unsigned L, int logT, int TP, int tid) {
  const unsigned Q = L / r, step = R / L;
  const unsigned nb = (R / r) << logT;
  const unsigned T = 1u << logT;
  const float invQ = 1.0f / (float)Q;
  for (unsigned w = tid; w < nb; w += 256) {
    const unsigned t = w & (T - 1u), u = w >> logT;
    const unsigned g = (unsigned)(((float)u + 0.5f) * invQ), j = u - g * Q;  // u < 4096: exact
    float2 *p = buf + (g * L + j) * TP + t;
    float2 x[r];
#pragma unroll
    for (int m = 0; m < r; ++m) x[m] = p[m * Q * TP];
    dft_nat<r>(x);
    p[0] = x[0];
    if (Q > 1) {
#pragma unroll
      for (int c = 1; c < r; ++c) p[c * Q * TP] = cmul(x[c], twR[j * c * step]);
    } else {
#pragma unroll
      for (int c = 1; c < r; ++c) p[c * TP] = x[c];
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(256, 4) void k_fft_mix(const float2 *__restrict__ in, float2 *__restrict__ out, MixDesc d) {
  extern __shared__ float2 sm[];
  const unsigned R = d.R;
  const int logT = d.logT, TP = (1 << logT) + 1;
  const unsigned T = 1u << logT;
  float2 *buf = sm;
  float2 *twR = sm + R * TP;
  unsigned short *kmap = reinterpret_cast<unsigned short *>(twR + R);  // position after the stages -> frequency
  const int tid = threadIdx.x;
  const unsigned smask = d.dir > 0 ? 0x80000000u : 0u;
  for (unsigned e = tid; e < R; e += 256) {
    twR[e] = tw_q32(phase_q32(e, d.r_hi, d.r_lo));
    unsigned rem = e, k = 0, mult = 1, L = R;
    for (int s = 0; s < d.nst; ++s) {
      const unsigned r = d.rad[s], Q = L / r, dig = rem / Q;
      rem -= dig * Q;
      k += dig * mult;
      mult *= r;
      L = Q;
    }
    kmap[e] = (unsigned short)k;
  }
  const unsigned work = R << logT;
  const float invR = 1.0f / (float)R;
  constexpr int NB = 8;
  if (d.mode == FFT_ROWS && d.acc) {
    // ---- segment spectra that never leave the chip: sum over this workgroup's rows of |X_row[k]|^2
    constexpr int NACC = 16;            // work = R << logT <= 4096 elements = 16 per thread
    float a[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) a[i] = 0.f;
    const unsigned ntiles = (d.rows + T - 1u) >> logT;
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const size_t row0 = (size_t)tile * T;
      __syncthreads();   // twR / kmap (first trip); the previous tile's spectra have been read (later trips)
      for (unsigned w0 = tid; w0 < work; w0 += 256 * NB) {
        float2 v[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const unsigned w = min(w0 + 256 * u, work - 1u);
          const unsigned t = (unsigned)(((float)w + 0.5f) * invR), j = w - t * R;
          const size_t row = row0 + t;
          if (d.rows_real > ROWS_REAL) v[u] = row < d.rows ? rows_load_int(in, d.rows_real, row * R + j, (float)d.src_w8) : make_float2(0.f, 0.f);
          else if (d.rows_real) v[u] = row < d.rows ? make_float2(reinterpret_cast<const float *>(in)[row * R + j], 0.f) : make_float2(0.f, 0.f);
          else v[u] = row < d.rows ? in[row * R + j] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const unsigned w = w0 + 256 * u;
          if (w < work) {
            const unsigned t = (unsigned)(((float)w + 0.5f) * invR), j = w - t * R;
            buf[j * TP + t] = v[u];
          }
        }
      }
      __syncthreads();
      unsigned L = R;
      for (int s = 0; s < d.nst; ++s) {
        const unsigned r = d.rad[s];
        switch (r) {
          case 2: mix_stage<2>(buf, twR, R, L, logT, TP, tid); break;
          case 3: mix_stage<3>(buf, twR, R, L, logT, TP, tid); break;
          case 4: mix_stage<4>(buf, twR, R, L, logT, TP, tid); break;
          case 5: mix_stage<5>(buf, twR, R, L, logT, TP, tid); break;
          case 8: mix_stage<8>(buf, twR, R, L, logT, TP, tid); break;
          case 9: mix_stage<9>(buf, twR, R, L, logT, TP, tid); break;
          case 10: mix_stage<10>(buf, twR, R, L, logT, TP, tid); break;
          case 25: mix_stage<25>(buf, twR, R, L, logT, TP, tid); break;
          default: mix_stage<16>(buf, twR, R, L, logT, TP, tid); break;
        }
        L /= r;
      }
      // thread-fixed (row of the tile, position) slots: the same every trip, so the sums stay in registers
#pragma unroll
      for (int i = 0; i < NACC; ++i) {
        const unsigned w = tid + 256u * i;
        if (w < work) {
          const unsigned t = (unsigned)(((float)w + 0.5f) * invR), p = w - t * R;
          const float2 x = buf[p * TP + t];
          a[i] += x.x * x.x + x.y * x.y;
        }
      }
    }
    __syncthreads();
    float *F = reinterpret_cast<float *>(buf);   // [T][R] row-of-tile sums, then added over the T rows in order
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
      const unsigned w = tid + 256u * i;
      if (w < work) F[w] = a[i];
    }
    __syncthreads();
    for (unsigned p = tid; p < R; p += 256) {
      float S = F[p];
      for (unsigned t = 1; t < T; ++t) S += F[t * R + p];
      d.acc[(size_t)blockIdx.x * R + kmap[p]] = S;
    }
    return;
  }
  const unsigned bid = blockIdx.x;

  size_t base = 0, tbase = 0, row0 = 0;
  unsigned tile = 0, a = 0, kt = 0, arest = 0, col0 = 0;
  if (d.mode == FFT_STRIDED) {
    tile = bid % d.tiles;
    a = (bid / d.tiles) % d.A;
    const unsigned b = bid / (d.tiles * d.A);
    col0 = tile * T;
    base = (size_t)b * d.N + (size_t)a * R * d.B + col0;
    for (unsigned w0 = tid; w0 < work; w0 += 256 * NB) {
      float2 v[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const unsigned w = w0 + 256 * u;
        const unsigned t = w & (T - 1u), j = w >> logT;
        v[u] = (w < work && col0 + t < d.B) ? fft_load(in, d.src_mode, d.src_n, base + (size_t)j * d.B + t, d.src_w8, d.src_aux)
                                             : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const unsigned w = w0 + 256 * u;
        if (w < work) buf[(w >> logT) * TP + (w & (T - 1u))] = conj_if(v[u], smask);
      }
    }
  } else {
    if (d.mode == FFT_LAST) {
      kt = bid % d.k1tiles;
      arest = (bid / d.k1tiles) % d.Aprime;
      tbase = (size_t)(bid / (d.k1tiles * d.Aprime)) * d.N;
    } else {
      row0 = (size_t)bid * T;
    }
    for (unsigned w0 = tid; w0 < work; w0 += 256 * NB) {
      float2 v[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const unsigned w = min(w0 + 256 * u, work - 1u);
        const unsigned t = (unsigned)(((float)w + 0.5f) * invR), j = w - t * R;  // w < 2^13: exact
        if (d.mode == FFT_LAST) {
          const unsigned k1 = kt * T + t;
          v[u] = k1 < d.R1 ? in[tbase + ((size_t)k1 * d.Aprime + arest) * R + j] : make_float2(0.f, 0.f);
        } else {
          const size_t row = row0 + t;
          v[u] = row < d.rows ? in[row * R + j] : make_float2(0.f, 0.f);
        }
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const unsigned w = w0 + 256 * u;
        if (w < work) {
          const unsigned t = (unsigned)(((float)w + 0.5f) * invR), j = w - t * R;
          buf[j * TP + t] = conj_if(v[u], smask);
        }
      }
    }
  }
  __syncthreads();

  unsigned L = R;
  for (int s = 0; s < d.nst; ++s) {
    const unsigned r = d.rad[s];
    switch (r) {
      case 2: mix_stage<2>(buf, twR, R, L, logT, TP, tid); break;
      case 3: mix_stage<3>(buf, twR, R, L, logT, TP, tid); break;
      case 4: mix_stage<4>(buf, twR, R, L, logT, TP, tid); break;
      case 5: mix_stage<5>(buf, twR, R, L, logT, TP, tid); break;
      case 8: mix_stage<8>(buf, twR, R, L, logT, TP, tid); break;
      case 9: mix_stage<9>(buf, twR, R, L, logT, TP, tid); break;
      case 10: mix_stage<10>(buf, twR, R, L, logT, TP, tid); break;
      case 25: mix_stage<25>(buf, twR, R, L, logT, TP, tid); break;
      default: mix_stage<16>(buf, twR, R, L, logT, TP, tid); break;
    }
    L /= r;
  }

  if (d.mode == FFT_STRIDED) {
    const unsigned Ka = digit_swap_g(a, d.nprev, d.Rprev, d.Wprev);
    const unsigned t = tid & (T - 1u);  // T <= 256: fixed per thread
    const unsigned col = col0 + t;
    const unsigned nnext = col / d.Bnext;
    if (col < d.B) {
      for (unsigned w0 = tid; w0 < work; w0 += 256 * NB) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const unsigned w = w0 + 256 * u;
          if (w < work) {
            const unsigned p = w >> logT, k = kmap[p];
            const float2 tw = tw_q32(phase_q32(nnext * (Ka + k * d.Pprev), d.ntw_hi, d.ntw_lo));
            out[base + (size_t)k * d.B + t] = conj_if(cmul(buf[p * TP + t], tw), smask);
          }
        }
      }
    }
  } else if (d.mode == FFT_LAST) {
    // digits k_2..k_{p-1} of arest -> their natural-order weight
    const unsigned Kp = digit_swap_g(arest, d.nprev - 1, d.Rprev + 1, d.Wprev + 1);
    const unsigned t = tid & (T - 1u);
    const unsigned k1 = kt * T + t;
    unsigned long long best = 0ull;
    if (k1 < d.R1) {
      const size_t orel = (size_t)k1 + Kp;
      for (unsigned w = tid; w < work; w += 256) {
        const unsigned p = w >> logT, k = kmap[p];
        const size_t o = orel + (size_t)k * d.Pprev;
        if (o < d.keep) {
          const float2 x = buf[p * TP + t];
          const float2 y = conj_if(make_float2(x.x * d.scale, x.y * d.scale), smask);
          if (d.epi.out) epilogue_store(d.epi, o, y, best); else out[tbase + o] = y;
        }
      }
    }
    if (d.epi.amax_keys) {
      __syncthreads();  // the tile is dead: its first words carry the wavefronts' keys
      epi_argmax_finish(d.epi, best, reinterpret_cast<unsigned long long *>(sm), 4);
    }
  } else {
    for (unsigned w = tid; w < work; w += 256) {
      const unsigned t = (unsigned)(((float)w + 0.5f) * invR), p = w - t * R;
      const size_t row = row0 + t;
      if (row < d.rows) {
        const float2 x = buf[p * TP + t];
        out[row * R + kmap[p]] = conj_if(make_float2(x.x * d.scale, x.y * d.scale), smask);
      }
    }
  }
}

// ---- two register steps per pass (the structure of fft.hip's k_fft_pass with general radices) --------------------
// R = RA * RB, both taken from the register DFT sizes: with n = j0 + RB*m and k = ka + RA*kb
//   X[ka + RA*kb] = sum_j0 W_RB^(j0*kb) * ( W_R^(j0*ka) * sum_m W_RA^(m*ka) x[j0 + RB*m] ).
// Step 1: RA-point DFTs over m in registers (slot = (column t, residue j0)), twiddle, ONE exchange through LDS;
// step 2: RB-point DFTs over j0 in registers (slot = (column t, frequency ka)), stores straight from registers.
// The generic kernel above walks the tile through LDS once per stage and twice more for loading and storing.
// STRIDED loads go global -> registers; LAST stages its rows (contiguous over the DFT index) through LDS first.
// (Mix2Geom: fft_plan.h)
template <int RA, int RB, int MODE>
__global__ __launch_bounds__((Mix2Geom<RA, RB>::NT)) void k_fft_mix2(const float2 *__restrict__ in, float2 *__restrict__ out, MixDesc d) {
  using G = Mix2Geom<RA, RB>;
  constexpr int R = G::R, CA = G::CA, CB = G::CB, NT = G::NT;
  extern __shared__ float2 sm[];
  const int logT = d.logT, T = 1 << logT, TP = T + 1;
  const int SA = (RB << logT) + (T < 32 ? T : 0);  // pitch of one ka plane of the exchange buffer
  float2 *buf = sm;                                // staging tile [j][TP] (LAST) and exchange buffer [ka][SA], aliased
  float2 *twR = sm + (R * TP > RA * SA ? R * TP : RA * SA);
  float2 *twK = twR + R;  // STRIDED: tw_sets x R inter-pass twiddles
  const int tid = threadIdx.x;
  const unsigned smask = d.dir > 0 ? 0x80000000u : 0u;
  if (RB > 1)
    for (int e = tid; e < R; e += NT) twR[e] = tw_q32(phase_q32((unsigned)e, d.r_hi, d.r_lo));
  const unsigned bid = blockIdx.x;
  const int n1 = RB << logT, n2 = RA << logT;  // DFT slots of step 1 / step 2

  float2 v[CA * RA > CB * RB ? CA * RA : CB * RB];
  size_t base = 0, tbase = 0;
  unsigned col0 = 0, a = 0, kt = 0, arest = 0, Ka = 0, n0 = 0;
  if (MODE == FFT_STRIDED) {
    const unsigned tile = bid % d.tiles;
    a = (bid / d.tiles) % d.A;
    const unsigned b = bid / (d.tiles * d.A);
    col0 = tile << logT;
    base = (size_t)b * d.N + (size_t)a * R * d.B + col0;
    if (d.src_mode == SRC_C2C) {  // (decided once: the loader switch inside the unrolled loads costs code and SALU)
#pragma unroll
      for (int q = 0; q < CA; ++q) {
        const int s = tid + NT * q;
        const int t = s & (T - 1), j0 = s >> logT;
        const bool ok = s < n1 && col0 + (unsigned)t < d.B;
        const float2 *src = in + base + (size_t)j0 * d.B + t;
#pragma unroll
        for (int m = 0; m < RA; ++m) v[q * RA + m] = ok ? conj_if(src[(size_t)(RB * m) * d.B], smask) : make_float2(0.f, 0.f);
      }
    } else {
#pragma unroll
      for (int q = 0; q < CA; ++q) {
        const int s = tid + NT * q;
        const int t = s & (T - 1), j0 = s >> logT;
        const bool ok = s < n1 && col0 + (unsigned)t < d.B;
#pragma unroll
        for (int m = 0; m < RA; ++m)
          v[q * RA + m] = ok ? conj_if(fft_load(in, d.src_mode, d.src_n, base + (size_t)(j0 + RB * m) * d.B + t, d.src_w8, d.src_aux), smask)
                             : make_float2(0.f, 0.f);
      }
    }
    // inter-pass twiddles W^(n_{i+1} (Ka + k Pprev)).  n_{i+1} = col / Bnext takes tw_sets consecutive values inside a
    // tile (1 when T divides Bnext, 2 when a tile can straddle one boundary ...): the workgroup evaluates those
    // tw_sets * R values once into LDS, under the latency of the loads just issued.  The last strided pass
    // (Bnext = 1: a set per column) factors them as W^(col Ka) -- one evaluation per thread -- times the table
    // W_{R Rnext}^(col k).  Evaluating every output's own twiddle (the fallback) costs ~30 VALU instructions each,
    // +45 % on a pass that is VALU-bound.
    Ka = digit_swap_g(a, d.nprev, d.Rprev, d.Wprev);
    n0 = col0 / d.Bnext;
    for (int e = tid; e < d.tw_sets * R; e += NT) {
      const unsigned set = (unsigned)e / (unsigned)R, k = (unsigned)e - set * (unsigned)R;
      twK[e] = tw_q32(phase_q32((n0 + set) * (Ka + k * d.Pprev), d.ntw_hi, d.ntw_lo));
    }
  } else {
    kt = bid % d.k1tiles;
    arest = (bid / d.k1tiles) % d.Aprime;
    tbase = (size_t)(bid / (d.k1tiles * d.Aprime)) * d.N;
    const int work = R << logT;
    const float invR = 1.0f / (float)R;
    constexpr int NL = (R * G::TM + NT - 1) / NT;  // staged elements per thread
    float2 w[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int e = min(tid + NT * u, work - 1);
      const int t = (int)(((float)e + 0.5f) * invR), j = e - t * R;  // e < 2^13: exact
      const unsigned k1 = (kt << logT) + (unsigned)t;
      w[u] = k1 < d.R1 ? in[tbase + ((size_t)k1 * d.Aprime + arest) * R + j] : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int e = tid + NT * u;
      if (e < work) {
        const int t = (int)(((float)e + 0.5f) * invR), j = e - t * R;
        buf[j * TP + t] = conj_if(w[u], smask);
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CA; ++q) {
      const int s = min(tid + NT * q, n1 - 1);
      const int t = s & (T - 1), j0 = s >> logT;
#pragma unroll
      for (int m = 0; m < RA; ++m) v[q * RA + m] = buf[(j0 + RB * m) * TP + t];
    }
  }
  __syncthreads();  // twR visible; staging tile fully read before the exchange buffer overwrites it

  // ---- step 1: RA-point DFTs over m, twiddle, exchange ----
#pragma unroll
  for (int q = 0; q < CA; ++q) dft_nat<RA>(v + q * RA);
  if (RB > 1) {
#pragma unroll
    for (int q = 0; q < CA; ++q) {
      const int s = tid + NT * q;
      const int j0 = s >> logT;
      if (s < n1) {
#pragma unroll
        for (int ka = 0; ka < RA; ++ka) {
          float2 x = v[q * RA + ka];
          if (ka) x = cmul(x, twR[j0 * ka]);
          buf[ka * SA + s] = x;  // (j0, t) is the slot number itself
        }
      }
    }
    __syncthreads();
    // ---- step 2: RB-point DFTs over j0 ----
#pragma unroll
    for (int q = 0; q < CB; ++q) {
      const int s = min(tid + NT * q, n2 - 1);
      const int t = s & (T - 1), ka = s >> logT;
#pragma unroll
      for (int j0 = 0; j0 < RB; ++j0) v[q * RB + j0] = buf[ka * SA + (j0 << logT) + t];
    }
#pragma unroll
    for (int q = 0; q < CB; ++q) dft_nat<RB>(v + q * RB);
  }
  // register i of output slot q now holds X[ka + RA*i] (RB > 1) or X[i] of column slot q (RB == 1)
  constexpr int CO = RB > 1 ? CB : CA, RO = RB > 1 ? RB : RA;
  const int no = RB > 1 ? n2 : n1;
  if (MODE == FFT_STRIDED) {
#pragma unroll
    for (int q = 0; q < CO; ++q) {
      const int s = tid + NT * q;
      const int t = s & (T - 1);
      if (s < no && col0 + (unsigned)t < d.B) {
        float2 *dst = out + base + t;
        const unsigned col = col0 + (unsigned)t;
        if (d.tw_sets) {
          const unsigned set = d.tw_sets == 1 ? 0u : d.tw_sets == 2 ? (col >= (n0 + 1u) * d.Bnext ? 1u : 0u) : col / d.Bnext - n0;
          const float2 *tws = twK + set * R;
#pragma unroll
          for (int i = 0; i < RO; ++i) {
            const int k = RB > 1 ? ((s >> logT) + RA * i) : i;
            dst[(size_t)k * d.B] = conj_if(cmul(v[q * RO + i], tws[k]), smask);
          }
        } else if (d.twg) {
          const float2 w1 = tw_q32(phase_q32(col * Ka, d.ntw_hi, d.ntw_lo));
          const float2 *g = d.twg + col;
#pragma unroll
          for (int i = 0; i < RO; ++i) {
            const int k = RB > 1 ? ((s >> logT) + RA * i) : i;
            dst[(size_t)k * d.B] = conj_if(cmul(v[q * RO + i], cmul(w1, g[(size_t)k * d.B])), smask);
          }
        } else {
          const unsigned nnext = col / d.Bnext;
          const unsigned e0 = nnext * Ka, est = nnext * d.Pprev;  // exponent of output k: nnext*(Ka + k*Pprev) < N
#pragma unroll
          for (int i = 0; i < RO; ++i) {
            const int k = RB > 1 ? ((s >> logT) + RA * i) : i;
            dst[(size_t)k * d.B] = conj_if(cmul(v[q * RO + i], tw_q32(phase_q32(e0 + (unsigned)k * est, d.ntw_hi, d.ntw_lo))), smask);
          }
        }
      }
    }
  } else {
    const unsigned Kp = digit_swap_g(arest, d.nprev - 1, d.Rprev + 1, d.Wprev + 1);
    unsigned long long best = 0ull;
#pragma unroll
    for (int q = 0; q < CO; ++q) {
      const int s = tid + NT * q;
      const int t = s & (T - 1);
      const unsigned k1 = (kt << logT) + (unsigned)t;
      if (s < no && k1 < d.R1) {
        const size_t orel = (size_t)k1 + Kp;
#pragma unroll
        for (int i = 0; i < RO; ++i) {
          const int k = RB > 1 ? ((s >> logT) + RA * i) : i;
          const size_t o = orel + (size_t)k * d.Pprev;
          const float2 x = v[q * RO + i];
          if (o < d.keep) {
            const float2 y = conj_if(make_float2(x.x * d.scale, x.y * d.scale), smask);
            if (d.epi.out) epilogue_store(d.epi, o, y, best); else out[tbase + o] = y;
          }
        }
      }
    }
    if (d.epi.amax_keys) {
      __syncthreads();  // the exchange buffer is dead: its first words carry the wavefronts' keys
      epi_argmax_finish(d.epi, best, reinterpret_cast<unsigned long long *>(sm), NT / 64);
    }
  }
}


// ---- the middle of an autocorrelation: last forward pass + power spectrum + first inverse pass in ONE launch --------
// The forward transform's last pass leaves, per workgroup, T columns c (= the low-order digits of the output index) x all
// R values of the top digit k: Z[c + Bc*k], Bc = N/R.  An inverse transform whose FIRST factor is the same R reads exactly
// that set for its strided DFTs (stride Bc).  In between, the packed power spectrum (fft_load's SRC_POWER) needs
// Z[g] and Z[N - g]: column c pairs with column Bc - c (top digit R-1-k; column 0 with itself, top digit R-k).  So a
// workgroup takes T/2 "direct" columns d and their mirrors Bc - d, transforms their rows forward (two register steps,
// as FFT_LAST), parks Z in LDS, forms Y from the pairs, transforms inverse (two register steps, as FFT_STRIDED) and
// stores with the inverse's inter-pass twiddles.  Z is never written to memory and never read twice: one launch, one
// 16-byte-per-point round trip and one doubled read less per search.
// (MidDesc: fft_plan.h)

template <int RA, int RB>
__global__ __launch_bounds__((Mix2Geom<RA, RB>::NT)) void k_fft_mid(const float2 *__restrict__ in, float2 *__restrict__ out, MidDesc d) {
  using G = Mix2Geom<RA, RB>;
  constexpr int R = G::R, CA = G::CA, CB = G::CB, NT = G::NT;
  static_assert(RB > 1, "two register steps");
  extern __shared__ float2 sm[];
  const int logT = d.logT, T = 1 << logT, TP = T + 1, Th = T >> 1;
  const int SA = (RB << logT) + (T < 32 ? T : 0);
  float2 *buf = sm;
  float2 *twR = sm + (R * TP > RA * SA ? R * TP : RA * SA);
  float2 *twK = twR + R;
  const int nsets = d.tw_sets > 0 ? d.tw_sets : 0;
  unsigned *colinfo = reinterpret_cast<unsigned *>(twK + 2 * nsets * R);  // [T] column (~0: none), [T] source row
  const int tid = threadIdx.x;
  const unsigned smask = 0x80000000u;  // the second half of the kernel is an inverse transform
  for (int e = tid; e < R; e += NT) twR[e] = tw_q32(phase_q32((unsigned)e, d.r_hi, d.r_lo));
  const unsigned d0 = blockIdx.x * (unsigned)Th;
  if (tid < T) {
    const bool mir = tid >= Th;
    const unsigned dcol = d0 + (unsigned)(tid & (Th - 1));
    unsigned c = 0xFFFFFFFFu;
    if (dcol < d.ndir && !(mir && dcol == 0)) c = mir ? d.Bc - dcol : dcol;  // (the mirror of column 0 is column 0 itself)
    unsigned row = 0;
    if (c != 0xFFFFFFFFu) {
      unsigned cc = c;
      for (int j = 0; j < d.nprev; ++j) { const unsigned q = cc / d.Rprev[j]; row = row * d.Rprev[j] + (cc - q * d.Rprev[j]); cc = q; }
    }
    colinfo[tid] = c;
    colinfo[T + tid] = row;
  }
  __syncthreads();
  const int n1 = RB << logT, n2 = RA << logT;
  float2 v[CA * RA > CB * RB ? CA * RA : CB * RB];
  {  // stage the rows (contiguous over the DFT index), then the step-1 registers
    const int work = R << logT;
    const float invR = 1.0f / (float)R;
    constexpr int NL = (R * G::TM + NT - 1) / NT;
    float2 w[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int e = min(tid + NT * u, work - 1);
      const int t = (int)(((float)e + 0.5f) * invR), j = e - t * R;
      w[u] = colinfo[t] != 0xFFFFFFFFu ? in[(size_t)colinfo[T + t] * R + j] : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int e = tid + NT * u;
      if (e < work) {
        const int t = (int)(((float)e + 0.5f) * invR), j = e - t * R;
        buf[j * TP + t] = w[u];
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CA; ++q) {
      const int s = min(tid + NT * q, n1 - 1);
      const int t = s & (T - 1), j0 = s >> logT;
#pragma unroll
      for (int m = 0; m < RA; ++m) v[q * RA + m] = buf[(j0 + RB * m) * TP + t];
    }
  }
  __syncthreads();
  // two register steps of one length-R DFT per column; afterwards register i of slot q = X[ka + RA*i] of column t
  auto two_steps = [&]() {
#pragma unroll
    for (int q = 0; q < CA; ++q) dft_nat<RA>(v + q * RA);
#pragma unroll
    for (int q = 0; q < CA; ++q) {
      const int s = tid + NT * q;
      const int j0 = s >> logT;
      if (s < n1) {
#pragma unroll
        for (int ka = 0; ka < RA; ++ka) {
          float2 x = v[q * RA + ka];
          if (ka) x = cmul(x, twR[j0 * ka]);
          buf[ka * SA + s] = x;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CB; ++q) {
      const int s = min(tid + NT * q, n2 - 1);
      const int t = s & (T - 1), ka = s >> logT;
#pragma unroll
      for (int j0 = 0; j0 < RB; ++j0) v[q * RB + j0] = buf[ka * SA + (j0 << logT) + t];
    }
#pragma unroll
    for (int q = 0; q < CB; ++q) dft_nat<RB>(v + q * RB);
  };
  two_steps();
  __syncthreads();  // exchange buffer fully read
#pragma unroll
  for (int q = 0; q < CB; ++q) {  // park Z[k][t]
    const int s = tid + NT * q;
    if (s < n2) {
      const int t = s & (T - 1), ka = s >> logT;
#pragma unroll
      for (int i = 0; i < RB; ++i) buf[(ka + RA * i) * TP + t] = v[q * RB + i];
    }
  }
  // the inverse's inter-pass twiddles W_{R R'}^(n k): the columns of a half are consecutive, so n = c / Bnext takes
  // tw_sets consecutive values there
  unsigned n0h[2] = {0u, 0u};
  if (nsets) {
    const unsigned dmax = min(d0 + (unsigned)Th - 1u, d.ndir - 1u);
    n0h[0] = d0 / d.Bnext;
    n0h[1] = (dmax ? d.Bc - dmax : 0u) / d.Bnext;
    for (int e = tid; e < 2 * nsets * R; e += NT) {
      const unsigned hs = (unsigned)e / (unsigned)R, k = (unsigned)e - hs * (unsigned)R;
      const unsigned h = hs / (unsigned)nsets, set = hs - h * (unsigned)nsets;
      twK[e] = tw_q32(phase_q32((n0h[h] + set) * k, d.ntw_hi, d.ntw_lo));
    }
  }
  __syncthreads();
  // Y = packed power spectrum from Z[g] and Z[N-g] (fft_load's SRC_POWER arithmetic), conjugated for the inverse
#pragma unroll
  for (int q = 0; q < CA; ++q) {
    const int s = min(tid + NT * q, n1 - 1);
    const int t = s & (T - 1), j0 = s >> logT;
    const unsigned c = colinfo[t];
    const bool ok = tid + NT * q < n1 && c != 0xFFFFFFFFu;
    const int tp = c == 0u ? t : (t ^ Th);
#pragma unroll
    for (int m = 0; m < RA; ++m) {
      const int j = j0 + RB * m;
      const int jm = c == 0u ? (j ? R - j : 0) : R - 1 - j;
      const float2 a = buf[j * TP + t], b = buf[jm * TP + tp];
      const float2 E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
      const float2 D = make_float2(0.5f * (a.x - b.x), 0.5f * (a.y + b.y));
      const float2 O = make_float2(D.y, -D.x);
      const float2 W = tw_frac(ok ? c + d.Bc * (unsigned)j : 0u, d.w8);
      const float2 WO = cmul(W, O);
      const float2 X0 = make_float2(E.x + WO.x, E.y + WO.y), X1 = make_float2(E.x - WO.x, E.y - WO.y);
      const float P0 = X0.x * X0.x + X0.y * X0.y, P1 = X1.x * X1.x + X1.y * X1.y;
      const float sum = P0 + P1, dif = P0 - P1;
      v[q * RA + m] = ok ? conj_if(make_float2(sum + dif * W.y, dif * W.x), smask) : make_float2(0.f, 0.f);
    }
  }
  __syncthreads();  // Z fully read before the exchange buffer overwrites it
  two_steps();
#pragma unroll
  for (int q = 0; q < CB; ++q) {
    const int s = tid + NT * q;
    const int t = s & (T - 1), ka = s >> logT;
    const unsigned c = s < n2 ? colinfo[t] : 0xFFFFFFFFu;
    if (c != 0xFFFFFFFFu) {
      float2 *dst = out + c;
      const unsigned nn = c / d.Bnext;
      if (nsets) {
        const unsigned h = t >= Th ? 1u : 0u;
        const float2 *tws = twK + (h * (unsigned)nsets + (nn - n0h[h])) * R;
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          const int k = ka + RA * i;
          dst[(size_t)k * d.Bc] = conj_if(cmul(v[q * RB + i], tws[k]), smask);
        }
      } else {
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          const int k = ka + RA * i;
          dst[(size_t)k * d.Bc] = conj_if(cmul(v[q * RB + i], tw_q32(phase_q32(nn * (unsigned)k, d.ntw_hi, d.ntw_lo))), smask);
        }
      }
    }
  }
}

typedef void (*mid_fn)(const float2 *, float2 *, MidDesc);
#define TSDR_X(RA_, RB_) k_fft_mid<RA_, RB_>,
static const mid_fn kMidFn[] = {TSDR_MID_LIST(TSDR_X)};   // entry i of fft_plan.h:kMid
#undef TSDR_X
static_assert(sizeof(kMidFn) / sizeof(kMidFn[0]) == kNMid2, "one kernel per entry of TSDR_MID_LIST");


// ---- three register steps per pass: factors of 500 .. 2000 ---------------------------------------------------------------
// R = RA * RB * RC.  With n = (n1 RB + n2) RC + n3 and k = k1 + RA k2 + RA RB k3:
//   step 1  slot (n2, n3, t):  A[k1] = sum_n1 W_RA^(n1 k1) x[n1, n2, n3],       times W_{RA RB}^(n2 k1)
//   step 2  slot (k1, n3, t):  B[k2] = sum_n2 W_RB^(n2 k2) A[k1, n2, n3],       times W_R^(n3 (k1 + RA k2))
//   step 3  slot (k1, k2, t):  X[k1 + RA k2 + RA RB k3] = sum_n3 W_RC^(n3 k3) B[k1, k2, n3]
// One slot per thread in every step (the workgroup has as many threads as the largest step has slots), two exchanges
// through ONE LDS tile that every step overwrites in place (a slot reads and writes the same RA / RB positions), k1 planes
// padded by T elements so that the step-3 reads of a half-wavefront fall on distinct banks.  A 2e6-point transform is TWO
// such passes (1000 x 2000) instead of three of the two-step kernel's: the passes are latency-bound at that size (every
// workgroup resident at once), so their number is what counts.  STRIDED loads go global -> registers in T-element runs;
// LAST reads its rows contiguously (slot order with the column slowest).  Inter-pass twiddles W^(n (Ka + k P)) are linear
// in k3: one evaluation for the slot's first output, one for the step, then a product per output.
// (Mix3Geom and the whole-row modes M3_*: fft_plan.h)
template <int RA, int RB, int RC, int LOGT, int MODE>
__global__ __launch_bounds__((Mix3Geom<RA, RB, RC, LOGT>::NT)) void k_fft_mix3(const float2 *__restrict__ in, float2 *__restrict__ out, MixDesc d) {
  using G = Mix3Geom<RA, RB, RC, LOGT>;
  constexpr int R = G::R, T = G::T, NT = G::NT, PLANE = G::PLANE, R23 = RB * RC;
  extern __shared__ float2 sm[];
  float2 *buf = sm;                       // [RA][PLANE]: (k1 | n1, second digit, third digit, column)
  float2 *twR = sm + RA * PLANE;          // W_R^e, e < R
  const int tid = threadIdx.x;
  const unsigned smask = d.dir > 0 ? 0x80000000u : 0u;
  for (int e = tid; e < R; e += NT) twR[e] = tw_q32(phase_q32((unsigned)e, d.r_hi, d.r_lo));
  const unsigned bid = blockIdx.x;
  float2 v[G::VMAX];
  constexpr bool IQROWS = MODE >= M3_ACC_IQ;
  constexpr int BM = IQROWS ? MODE - (M3_ACC_IQ - M3_ACC) : MODE;   // the mode without the input format
  if (MODE >= M3_ACC) {
    // ---- getWelch's accumulator (see MixDesc::acc): rows = segments, T of them per tile, nothing stored per transform.
    // A thread's step-3 slot (kk, t3) is the same for every tile, so abs2 of its RC outputs accumulates in registers.
    float acc[RC];
#pragma unroll
    for (int k3 = 0; k3 < RC; ++k3) acc[k3] = 0.f;
    const unsigned ntiles = (d.rows + (unsigned)T - 1u) >> LOGT;
    const int t1 = tid / R23, r23 = tid - t1 * R23;
    const int t3 = tid & (T - 1), kk = tid >> LOGT;
    for (unsigned tile = bid; tile < ntiles; tile += gridDim.x) {
      const unsigned row1 = (tile << LOGT) + (unsigned)t1;
      const bool ok1 = tid < G::S1 && row1 < d.rows;
      if (IQROWS) {   // integer IQ rows: a wavefront still reads one row contiguously (2 or 4 bytes per lane)
        const size_t e0 = (size_t)row1 * R + r23;
        const float sc = (float)d.src_w8;
#pragma unroll
        for (int n1 = 0; n1 < RA; ++n1) v[n1] = ok1 ? rows_load_int(in, d.rows_real, e0 + n1 * R23, sc) : make_float2(0.f, 0.f);
      } else if (d.rows_real) {
        const float *src = reinterpret_cast<const float *>(in) + (size_t)row1 * R + r23;
#pragma unroll
        for (int n1 = 0; n1 < RA; ++n1) v[n1] = ok1 ? make_float2(src[n1 * R23], 0.f) : make_float2(0.f, 0.f);
      } else {
        const float2 *src = in + (size_t)row1 * R + r23;
#pragma unroll
        for (int n1 = 0; n1 < RA; ++n1) v[n1] = ok1 ? (BM == M3_ROWS ? conj_if(src[n1 * R23], smask) : src[n1 * R23]) : make_float2(0.f, 0.f);
      }
      __syncthreads();  // twR (first trip); the previous tile's step-3 reads (later trips)
      if (tid < G::S1) {
        dft_nat<RA>(v);
        const int n2 = r23 / RC;
#pragma unroll
        for (int k1 = 0; k1 < RA; ++k1) {
          float2 x = v[k1];
          if (k1) x = cmul(x, twR[(n2 * k1) * RC]);
          buf[k1 * PLANE + r23 * T + (t1 ^ G::swz(r23 - n2 * RC))] = x;
        }
      }
      __syncthreads();
      if (tid < G::S2) {
        const int t = tid & (T - 1), q = tid >> LOGT, k1 = q / RC, n3 = q - k1 * RC;
        float2 *p = buf + k1 * PLANE + n3 * T + (t ^ G::swz(n3));
#pragma unroll
        for (int n2 = 0; n2 < RB; ++n2) v[n2] = p[n2 * RC * T];
        dft_nat<RB>(v);
#pragma unroll
        for (int k2 = 0; k2 < RB; ++k2) {
          float2 x = v[k2];
          if (k2 || k1) x = cmul(x, twR[n3 * (k1 + RA * k2)]);
          p[k2 * RC * T] = x;
        }
      }
      __syncthreads();
      if (tid < G::S3 && (tile << LOGT) + (unsigned)t3 < d.rows) {
        const int k2 = kk / RA, k1 = kk - k2 * RA;
        const float2 *p = buf + k1 * PLANE + k2 * RC * T;
#pragma unroll
        for (int n3 = 0; n3 < RC; ++n3) v[n3] = p[n3 * T + (t3 ^ G::swz(n3))];
        dft_nat<RC>(v);
        if (BM == M3_ROWS) {
          float2 *row = d.rows_out + (size_t)((tile << LOGT) + (unsigned)t3) * R;
#pragma unroll
          for (int k3 = 0; k3 < RC; ++k3)
            row[kk + RA * RB * k3] = conj_if(make_float2(v[k3].x * d.scale, v[k3].y * d.scale), smask);
        } else if (BM == M3_WF) {
          double *row = d.wf + (size_t)((tile << LOGT) + (unsigned)t3) * R;
#pragma unroll
          for (int k3 = 0; k3 < RC; ++k3) {
            int j = kk + RA * RB * k3 + R / 2;   // fftshift: frequency k lands at (k + floor(R / 2)) mod R
            if (j >= R) j -= R;
            __builtin_nontemporal_store((double)(v[k3].x * v[k3].x + v[k3].y * v[k3].y), &row[j]);   // written once
          }
        } else {
#pragma unroll
          for (int k3 = 0; k3 < RC; ++k3) acc[k3] += v[k3].x * v[k3].x + v[k3].y * v[k3].y;
        }
      }
    }
    if (BM != M3_ACC) return;
    // the T segments of a tile sit in T adjacent lanes: added by a fixed xor tree, lane t3 = 0 stores
#pragma unroll
    for (int k3 = 0; k3 < RC; ++k3) {
      float sres = acc[k3];
#pragma unroll
      for (int off = 1; off < T; off <<= 1) sres += __shfl_xor(sres, off, 64);
      if (tid < G::S3 && t3 == 0) d.acc[(size_t)bid * R + (unsigned)(kk + RA * RB * k3)] = sres;
    }
    return;
  }
  size_t base = 0, tbase = 0;
  unsigned col0 = 0, a = 0, kt = 0, arest = 0;
  // ---- step 1 inputs
  int t1, r23;
  bool ok1;
  if (MODE == FFT_STRIDED) {
    const unsigned tile = bid % d.tiles;
    a = (bid / d.tiles) % d.A;
    const unsigned b = bid / (d.tiles * d.A);
    col0 = tile << LOGT;
    base = (size_t)b * d.N + (size_t)a * R * d.B + col0;
    t1 = tid & (T - 1); r23 = tid >> LOGT;
    ok1 = tid < G::S1 && col0 + (unsigned)t1 < d.B;
    const size_t g0 = base + (size_t)r23 * d.B + t1;
    if (d.src_mode == SRC_C2C) {
#pragma unroll
      for (int n1 = 0; n1 < RA; ++n1) v[n1] = ok1 ? conj_if(in[g0 + (size_t)(n1 * R23) * d.B], smask) : make_float2(0.f, 0.f);
    } else {
#pragma unroll
      for (int n1 = 0; n1 < RA; ++n1)
        v[n1] = ok1 ? conj_if(fft_load(in, d.src_mode, d.src_n, g0 + (size_t)(n1 * R23) * d.B, d.src_w8, d.src_aux), smask) : make_float2(0.f, 0.f);
    }
  } else {
    kt = bid % d.k1tiles;
    arest = (bid / d.k1tiles) % d.Aprime;
    tbase = (size_t)(bid / (d.k1tiles * d.Aprime)) * d.N;
    t1 = tid / R23; r23 = tid - t1 * R23;  // the column slowest: a wavefront reads one row contiguously
    const unsigned k1g = (kt << LOGT) + (unsigned)t1;
    ok1 = tid < G::S1 && k1g < d.R1;
    const float2 *src = in + tbase + ((size_t)k1g * d.Aprime + arest) * R + r23;
#pragma unroll
    for (int n1 = 0; n1 < RA; ++n1) v[n1] = ok1 ? conj_if(src[n1 * R23], smask) : make_float2(0.f, 0.f);
  }
  __syncthreads();  // twR
  if (tid < G::S1) {
    dft_nat<RA>(v);
    const int n2 = r23 / RC;
#pragma unroll
    for (int k1 = 0; k1 < RA; ++k1) {
      float2 x = v[k1];
      if (k1) x = cmul(x, twR[(n2 * k1) * RC]);  // W_{RA RB}^(n2 k1)
      buf[k1 * PLANE + r23 * T + (t1 ^ G::swz(r23 - n2 * RC))] = x;
    }
  }
  __syncthreads();
  // ---- step 2: slot (k1, n3, t), in place
  if (tid < G::S2) {
    const int t = tid & (T - 1), q = tid >> LOGT, k1 = q / RC, n3 = q - k1 * RC;
    float2 *p = buf + k1 * PLANE + n3 * T + (t ^ G::swz(n3));
#pragma unroll
    for (int n2 = 0; n2 < RB; ++n2) v[n2] = p[n2 * RC * T];
    dft_nat<RB>(v);
#pragma unroll
    for (int k2 = 0; k2 < RB; ++k2) {
      float2 x = v[k2];
      const int e = n3 * (k1 + RA * k2);
      if (k2 || k1) x = cmul(x, twR[e]);  // (e = 0 gives 1 anyway)
      p[k2 * RC * T] = x;
    }
  }
  __syncthreads();
  // ---- step 3: slot (kk = k1 + RA k2, t); outputs straight from registers
  const int t3 = tid & (T - 1), kk = tid >> LOGT;
  const bool ok3 = tid < G::S3;
  if (ok3) {
    const int k2 = kk / RA, k1 = kk - k2 * RA;
    const float2 *p = buf + k1 * PLANE + k2 * RC * T;
#pragma unroll
    for (int n3 = 0; n3 < RC; ++n3) v[n3] = p[n3 * T + (t3 ^ G::swz(n3))];
    dft_nat<RC>(v);
  }
  if (MODE == FFT_STRIDED) {
    const unsigned col = col0 + (unsigned)t3;
    if (ok3 && col < d.B) {
      const unsigned Ka = digit_swap_g(a, d.nprev, d.Rprev, d.Wprev);
      const unsigned nn = col / d.Bnext;
      float2 w = tw_q32(phase_q32(nn * (Ka + (unsigned)kk * d.Pprev), d.ntw_hi, d.ntw_lo));
      const float2 ws = tw_q32(phase_q32(nn * ((unsigned)(RA * RB) * d.Pprev), d.ntw_hi, d.ntw_lo));
      float2 *dst = out + base + (size_t)kk * d.B + t3;
#pragma unroll
      for (int k3 = 0; k3 < RC; ++k3) {
        dst[(size_t)(RA * RB * k3) * d.B] = conj_if(cmul(v[k3], w), smask);
        w = cmul(w, ws);
      }
    }
  } else {
    const unsigned Kp = digit_swap_g(arest, d.nprev - 1, d.Rprev + 1, d.Wprev + 1);
    const unsigned k1g = (kt << LOGT) + (unsigned)t3;
    unsigned long long best = 0ull;
    if (ok3 && k1g < d.R1) {
      const size_t orel = (size_t)k1g + Kp;
#pragma unroll
      for (int k3 = 0; k3 < RC; ++k3) {
        const size_t o = orel + (size_t)(kk + RA * RB * k3) * d.Pprev;
        if (o < d.keep) {
          const float2 y = conj_if(make_float2(v[k3].x * d.scale, v[k3].y * d.scale), smask);
          if (d.epi.out) epilogue_store(d.epi, o, y, best); else out[tbase + o] = y;
        }
      }
    }
    if (d.epi.amax_keys) {
      __syncthreads();
      epi_argmax_finish(d.epi, best, reinterpret_cast<unsigned long long *>(sm), NT / 64);
    }
  }
}

typedef void (*mix_fn)(const float2 *, float2 *, MixDesc);
// entry i of fft_plan.h:kMix3, by mode: FFT_STRIDED, FFT_LAST, M3_ACC, M3_WF, M3_ROWS, M3_ACC_IQ, M3_WF_IQ, M3_ROWS_IQ (the row-only entries: no pass kernels)
struct Mix3Fns { mix_fn fn[8]; };
#define TSDR_ROWS(RA_, RB_, RC_, LT_)                                                                                      \
  k_fft_mix3<RA_, RB_, RC_, LT_, M3_ACC>, k_fft_mix3<RA_, RB_, RC_, LT_, M3_WF>, k_fft_mix3<RA_, RB_, RC_, LT_, M3_ROWS>,   \
  k_fft_mix3<RA_, RB_, RC_, LT_, M3_ACC_IQ>, k_fft_mix3<RA_, RB_, RC_, LT_, M3_WF_IQ>, k_fft_mix3<RA_, RB_, RC_, LT_, M3_ROWS_IQ>
#define TSDR_X(RA_, RB_, RC_, LT_) {{k_fft_mix3<RA_, RB_, RC_, LT_, FFT_STRIDED>, k_fft_mix3<RA_, RB_, RC_, LT_, FFT_LAST>, TSDR_ROWS(RA_, RB_, RC_, LT_)}},
#define TSDR_XW(RA_, RB_, RC_, LT_) {{nullptr, nullptr, TSDR_ROWS(RA_, RB_, RC_, LT_)}},
static const Mix3Fns kMix3Fn[] = {TSDR_MIX3_LIST(TSDR_X) TSDR_WELCH3_LIST(TSDR_XW)};
#undef TSDR_X
#undef TSDR_XW
#undef TSDR_ROWS
static_assert(sizeof(kMix3Fn) / sizeof(kMix3Fn[0]) == kNMix3, "one set of kernels per entry of TSDR_MIX3_LIST + TSDR_WELCH3_LIST");

// ---- the fused middle (k_fft_mid) with three register steps: last forward factor = first inverse factor = 1000 or 2000 ----
// Same pairing of direct and mirrored columns, same power-spectrum arithmetic; the two length-R DFTs are k_fft_mix3's
// three steps.  With it a 2e6-point autocorrelation is THREE launches (1000 | 2000 + power + 2000 | 1000) and Z is never
// written.
template <int RA, int RB, int RC, int LOGT>
__global__ __launch_bounds__((Mix3Geom<RA, RB, RC, LOGT>::NT)) void k_fft_mid3(const float2 *__restrict__ in, float2 *__restrict__ out, MidDesc d) {
  using G = Mix3Geom<RA, RB, RC, LOGT>;
  constexpr int R = G::R, T = G::T, NT = G::NT, PLANE = G::PLANE, R23 = RB * RC, Th = T / 2;
  extern __shared__ float2 sm[];
  float2 *buf = sm;                       // [RA][PLANE] exchange tile; also Z[k][t] between the two transforms
  float2 *twR = sm + RA * PLANE;
  unsigned *colinfo = reinterpret_cast<unsigned *>(twR + R);  // [T] column (~0: none), [T] source row
  const int tid = threadIdx.x;
  const unsigned smask = 0x80000000u;
  for (int e = tid; e < R; e += NT) twR[e] = tw_q32(phase_q32((unsigned)e, d.r_hi, d.r_lo));
  const unsigned d0 = blockIdx.x * (unsigned)Th;
  if (tid < T) {
    const bool mir = tid >= Th;
    const unsigned dcol = d0 + (unsigned)(tid & (Th - 1));
    unsigned c = 0xFFFFFFFFu;
    if (dcol < d.ndir && !(mir && dcol == 0)) c = mir ? d.Bc - dcol : dcol;
    unsigned row = 0;
    if (c != 0xFFFFFFFFu) {
      unsigned cc = c;
      for (int j = 0; j < d.nprev; ++j) { const unsigned q = cc / d.Rprev[j]; row = row * d.Rprev[j] + (cc - q * d.Rprev[j]); cc = q; }
    }
    colinfo[tid] = c;
    colinfo[T + tid] = row;
  }
  __syncthreads();
  float2 v[G::VMAX];
  // three register steps of one length-R DFT per column; on entry v = the slot's RA inputs (slot = (r23, t1)), on exit
  // v[k3] = X[kk + RA RB k3] of column t3 for the slot (kk, t3) = (tid >> LOGT, tid & (T-1))
  auto three_steps = [&](int t1, int r23) {
    if (tid < G::S1) {
      dft_nat<RA>(v);
      const int n2 = r23 / RC;
#pragma unroll
      for (int k1 = 0; k1 < RA; ++k1) {
        float2 x = v[k1];
        if (k1) x = cmul(x, twR[(n2 * k1) * RC]);
        buf[k1 * PLANE + r23 * T + (t1 ^ G::swz(r23 - n2 * RC))] = x;
      }
    }
    __syncthreads();
    if (tid < G::S2) {
      const int t = tid & (T - 1), q = tid >> LOGT, k1 = q / RC, n3 = q - k1 * RC;
      float2 *p = buf + k1 * PLANE + n3 * T + (t ^ G::swz(n3));
#pragma unroll
      for (int n2 = 0; n2 < RB; ++n2) v[n2] = p[n2 * RC * T];
      dft_nat<RB>(v);
#pragma unroll
      for (int k2 = 0; k2 < RB; ++k2) {
        float2 x = v[k2];
        if (k2 || k1) x = cmul(x, twR[n3 * (k1 + RA * k2)]);
        p[k2 * RC * T] = x;
      }
    }
    __syncthreads();
    if (tid < G::S3) {
      const int t = tid & (T - 1), kk = tid >> LOGT, k2 = kk / RA, k1 = kk - k2 * RA;
      const float2 *p = buf + k1 * PLANE + k2 * RC * T;
#pragma unroll
      for (int n3 = 0; n3 < RC; ++n3) v[n3] = p[n3 * T + (t ^ G::swz(n3))];
      dft_nat<RC>(v);
    }
  };
  {  // forward: rows are contiguous over the DFT index (slot order with the column slowest)
    const int t1 = tid / R23, r23 = tid - t1 * R23;
    const bool ok = tid < G::S1 && colinfo[t1 < T ? t1 : 0] != 0xFFFFFFFFu;
    const float2 *src = in + (size_t)colinfo[T + (t1 < T ? t1 : 0)] * R + r23;
#pragma unroll
    for (int n1 = 0; n1 < RA; ++n1) v[n1] = ok ? src[n1 * R23] : make_float2(0.f, 0.f);
    three_steps(t1, r23);
  }
  const int t3 = tid & (T - 1), kk = tid >> LOGT;
  __syncthreads();  // every step-3 read of the tile is done
  if (tid < G::S3) {
#pragma unroll
    for (int k3 = 0; k3 < RC; ++k3) buf[(kk + RA * RB * k3) * T + t3] = v[k3];  // park Z[k][t]
  }
  __syncthreads();
  {  // Y from Z[g] and Z[N-g], conjugated for the inverse; slot (r23, t) with the column fastest
    const int t = tid & (T - 1), r23 = tid >> LOGT;
    const unsigned c = tid < G::S1 ? colinfo[t] : 0xFFFFFFFFu;
    const bool ok = c != 0xFFFFFFFFu;
    const int tp = c == 0u ? t : (t ^ Th);
#pragma unroll
    for (int n1 = 0; n1 < RA; ++n1) {
      const int j = ok ? n1 * R23 + r23 : 0;
      const int jm = c == 0u ? (j ? R - j : 0) : R - 1 - j;
      const float2 a = buf[j * T + t], b = buf[jm * T + tp];
      const float2 E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
      const float2 D = make_float2(0.5f * (a.x - b.x), 0.5f * (a.y + b.y));
      const float2 O = make_float2(D.y, -D.x);
      const float2 W = tw_frac(ok ? c + d.Bc * (unsigned)j : 0u, d.w8);
      const float2 WO = cmul(W, O);
      const float2 X0 = make_float2(E.x + WO.x, E.y + WO.y), X1 = make_float2(E.x - WO.x, E.y - WO.y);
      const float P0 = X0.x * X0.x + X0.y * X0.y, P1 = X1.x * X1.x + X1.y * X1.y;
      const float sum = P0 + P1, dif = P0 - P1;
      v[n1] = ok ? conj_if(make_float2(sum + dif * W.y, dif * W.x), smask) : make_float2(0.f, 0.f);
    }
    __syncthreads();  // Z fully read before the exchange tile overwrites it
    three_steps(t, r23);
  }
  if (tid < G::S3) {
    const unsigned c = colinfo[t3];
    if (c != 0xFFFFFFFFu) {
      const unsigned nn = c / d.Bnext;
      float2 w = tw_q32(phase_q32(nn * (unsigned)kk, d.ntw_hi, d.ntw_lo));
      const float2 ws = tw_q32(phase_q32(nn * (unsigned)(RA * RB), d.ntw_hi, d.ntw_lo));
      float2 *dst = out + c + (size_t)kk * d.Bc;
#pragma unroll
      for (int k3 = 0; k3 < RC; ++k3) {
        dst[(size_t)(RA * RB * k3) * d.Bc] = conj_if(cmul(v[k3], w), smask);
        w = cmul(w, ws);
      }
    }
  }
}
#define TSDR_X(RA_, RB_, RC_, LT_) k_fft_mid3<RA_, RB_, RC_, LT_>,
static const mid_fn kMid3Fn[] = {TSDR_MID3_LIST(TSDR_X)};   // entry kNMid2 + i of fft_plan.h:kMid
#undef TSDR_X
static_assert(sizeof(kMid3Fn) / sizeof(kMid3Fn[0]) == kNMid - kNMid2, "one kernel per entry of TSDR_MID3_LIST");
#define TSDR_X(RA_, RB_) {k_fft_mix2<RA_, RB_, FFT_STRIDED>, k_fft_mix2<RA_, RB_, FFT_LAST>},
static const mix_fn kMix2Fn[][2] = {TSDR_MIX2_LIST(TSDR_X)};   // entry i of fft_plan.h:kMix2, by mode
#undef TSDR_X
static_assert(sizeof(kMix2Fn) / sizeof(kMix2Fn[0]) == kNMix2, "one pair of kernels per entry of TSDR_MIX2_LIST");

// ---- the launcher: the only place that launches a pass kernel ----------------------------------------------------------------------
// (what is launched, on which buffers, with which tables: fft_plan.h.  A plan's invariants -- indices inside the tables they were
// made from, a buffer behind every role a step names -- are asserts: no caller can break them.)
// W_{R*Rn}^(col*k) at [k * Rn + col], k < R, col < Rn (built once per pair in extended precision, then resident)
static int get_twg(tsdr_ctx *ctx, unsigned R, unsigned Rn, const float2 **out) {
  const unsigned key = (R << 16) | Rn;
  auto it = ctx->twg.find(key);
  if (it != ctx->twg.end()) { *out = it->second; return TSDR_OK; }
  std::vector<float2> h((size_t)R * Rn);
  const unsigned long long M = (unsigned long long)R * Rn;
  for (unsigned k = 0; k < R; ++k)
    for (unsigned c = 0; c < Rn; ++c) {
      const long double ang = -2.0L * M_PIl * (long double)(((unsigned long long)k * c) % M) / (long double)M;
      h[(size_t)k * Rn + c] = make_float2((float)cosl(ang), (float)sinl(ang));
    }
  float2 *dev = nullptr;
  TSDR_HIP(ctx, hipMalloc((void **)&dev, h.size() * sizeof(float2)));
  TSDR_HIP(ctx, hipMemcpy(dev, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice));
  ctx->twg.emplace(key, dev);
  *out = dev;
  return TSDR_OK;
}

// kernels above 64 KiB of dynamic LDS have to be opted in once: every mode of a three-step entry together
static int mix3_prepare(tsdr_ctx *ctx, int inst) {
  for (mix_fn f : kMix3Fn[inst].fn) {
    if (!f) continue;
    int rc = lds_opt_in(ctx, (const void *)f, kMix3[inst].lds);
    if (rc) return rc;
  }
  return TSDR_OK;
}

// Launches ONE step: the plan's sink (FftPlan::sink), called the moment a step is complete, so that the planner fills the next
// pass's descriptor while this one runs -- as the drivers did that decided while they launched.
struct FftBufs { tsdr_ctx *ctx; float2 *buf[5]; };   // buf: by FftBuf; FB_WORK is taken at the first step that names it
static int launch_step(void *user, const FftPlan &pl, const FftStep &s) {
  FftBufs &L = *static_cast<FftBufs *>(user);
  tsdr_ctx *ctx = L.ctx;
  float2 *const *buf = L.buf;
  if (pl.work_bytes && !L.buf[FB_WORK]) {
    L.buf[FB_WORK] = (float2 *)ctx->scratch(WS_FFT_B, pl.work_bytes);
    if (!L.buf[FB_WORK]) return TSDR_ENOMEM;
  }
  assert(s.src != FB_NONE && buf[s.src] && (s.dst == FB_NONE || buf[s.dst]));
  const float2 *src = buf[s.src];
  float2 *dst = buf[s.dst];
  const dim3 grid(s.grid), block(s.block);
  if (s.kernel == FK_PASS) {
    assert(s.inst >= 1 && s.inst <= 8 && s.mode >= FFT_STRIDED && s.mode <= FFT_ROWS);
    if (int rc = ensure_tw_small(ctx)) return rc;
    TSDR_LAUNCH(ctx, s.name, fft_pass_kernel(s.mode, s.inst), grid, block, s.lds, src, dst, s.p.pass, (const float2 *)ctx->tw_small);
  } else if (s.kernel == FK_MID || s.kernel == FK_MID3) {
    assert(s.inst >= 0 && s.inst < kNMid && (s.inst >= kNMid2) == (s.kernel == FK_MID3));
    const mid_fn fn = s.kernel == FK_MID ? kMidFn[s.inst] : kMid3Fn[s.inst - kNMid2];
    if (s.opt_in)
      if (int rc = lds_opt_in(ctx, (const void *)fn, s.lds)) return rc;
    TSDR_LAUNCH(ctx, s.name, fn, grid, block, s.lds, src, dst, s.p.mid);
  } else {
    mix_fn fn = k_fft_mix;
    if (s.kernel == FK_MIX2) {
      assert(s.inst >= 0 && s.inst < kNMix2 && (s.mode == FFT_STRIDED || s.mode == FFT_LAST));
      fn = kMix2Fn[s.inst][s.mode];
    } else if (s.kernel == FK_MIX3) {
      assert(s.inst >= 0 && s.inst < kNMix3 && (s.mode <= FFT_LAST || (s.mode >= M3_ACC && s.mode <= M3_ROWS_IQ)));
      fn = kMix3Fn[s.inst].fn[s.mode <= FFT_LAST ? s.mode : s.mode - M3_ACC + 2];
    }
    assert(fn && s.kernel >= FK_MIX && s.kernel <= FK_MIX3);   // (the row-only entries have no pass kernels, and no plan asks for one)
    if (s.opt_in)
      if (int rc = s.kernel == FK_MIX3 ? mix3_prepare(ctx, s.inst) : lds_opt_in(ctx, (const void *)fn, s.lds)) return rc;
    if (s.twg_R) {   // the one pointer inside a descriptor that is the launcher's to set
      MixDesc d = s.p.mix;
      if (int rc = get_twg(ctx, s.twg_R, s.twg_Rn, &d.twg)) return rc;
      TSDR_LAUNCH(ctx, s.name, fn, grid, block, s.lds, src, dst, d);
    } else {
      TSDR_LAUNCH(ctx, s.name, fn, grid, block, s.lds, src, dst, s.p.mix);
    }
  }
  return TSDR_OK;
}

// runs plan(pl) with the launcher as the plan's sink; pl.nsteps then says how many steps were launched
template <class Plan>
static int fft_launch(tsdr_ctx *ctx, const float2 *in, float2 *out, float2 *mid, Plan &&plan, FftPlan &pl) {
  FftBufs L{ctx, {nullptr, const_cast<float2 *>(in), out, nullptr, mid}};
  pl.sink = launch_step;
  pl.user = &L;
  plan(pl);
  if (pl.status) return pl.err[0] ? set_err(ctx, pl.status, "%s", pl.err) : pl.status;
  if (int rf = run_fence(ctx)) return rf;   // (the copy below precedes the first launch)
  if (pl.copy_bytes && in != out) TSDR_HIP(ctx, hipMemcpyAsync(out, in, pl.copy_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return TSDR_OK;
}

// ---- host entry points (fft_dev.h) ------------------------------------------------------------------------------------------------
int fft_run(tsdr_ctx *ctx, const FftReq &q) {
  FftPlan pl;
  return fft_launch(ctx, q.in, q.out, nullptr, [&](FftPlan &p) { plan_fft(p, q, fft_opts(ctx)); }, pl);
}

int fft_run_autocorr(tsdr_ctx *ctx, const FftReq &q, float2 *Zbuf, bool *done) {
  FftPlan pl;
  int rc = fft_launch(ctx, q.in, q.out, Zbuf, [&](FftPlan &p) { plan_autocorr(p, q, fft_opts(ctx)); }, pl);
  *done = !rc && pl.nsteps > 0;
  return rc;
}

// the whole-row launches: *did = false (nothing launched) when the length or count is not one they serve
static int rows_run(tsdr_ctx *ctx, RowsReq r, const SigSrc &sig, size_t N, size_t rows, bool *did, unsigned *grid = nullptr) {
  r.kind = sig.kind; r.sig_scale = sig.scale; r.N = N; r.rows = rows;
  FftPlan pl;
  int rc = fft_launch(ctx, sig.c32(), nullptr, nullptr, [&](FftPlan &p) { plan_rows(p, r, fft_opts(ctx)); }, pl);
  *did = !rc && pl.nsteps > 0;
  if (*did && grid) *grid = pl.step[0].grid;
  return rc;
}
// getWelch's accumulation for any 2^a 3^b 5^c segment length up to 4096 without writing a segment spectrum: *nparts partial
// power spectra of N floats each (natural order) land in `part` (room for fft_rows_welch_parts() of them)
unsigned fft_rows_welch_parts(tsdr_ctx *ctx) { return welch_parts(fft_opts(ctx)); }
int fft_rows_welch(tsdr_ctx *ctx, const SigSrc &sig, size_t N, size_t nbSeg, float *part, unsigned *nparts, bool *did) {
  RowsReq r;
  r.what = ROWS_TO_WELCH; r.acc = part;
  return rows_run(ctx, r, sig, N, nbSeg, did, nparts);
}
// Batched row transforms (tsdr_fft_c2c with batch > 1) of the lengths the three-step kernels serve, in ONE launch: a row never
// leaves the chip between its steps.  (The pass engines split a 512 .. 4096-point row into two passes whose strided one has only
// 16-64 columns to work on: 67-197 us for 1e7 points against 35-50 us here; rows up to 256 points are one pass there already.)
int fft_rows_store(tsdr_ctx *ctx, const SigSrc &in, float2 *out, size_t N, size_t batch, int dir, float scale, bool *did) {
  RowsReq r;
  r.what = ROWS_TO_STORE; r.rows_out = out; r.dir = dir; r.scale = scale;
  return rows_run(ctx, r, in, N, batch, did);
}
// getWaterfall for the segment lengths the three-step kernels serve (1024 has k_seg1024): segments -> Float64 power spectra,
// fftshifted, in ONE launch -- the segment spectra never reach HBM (the route through a batched FFT + k_waterfall writes and
// re-reads them: 109-250 us per C2 buffer at 512 .. 4096 against 40-60 us here)
int fft_rows_waterfall(tsdr_ctx *ctx, const SigSrc &sig, size_t N, size_t nbSeg, double *wf, bool *did) {
  RowsReq r;
  r.what = ROWS_TO_WATERFALL; r.wf = wf;
  return rows_run(ctx, r, sig, N, nbSeg, did);
}

// what the planner answers about a length
int fft_passes(size_t N) { return fft_split(N, true); }
bool fft_mixed_ok(size_t N) {
  MixPlan pl;
  return fft_mixed_plan(N, &pl);
}
int fft_mixed_passes(tsdr_ctx *ctx, size_t N, size_t batch) {   // the split plan_fft makes for this call
  MixPlan pl;
  return fft_mixed_plan(N, &pl, fft_big_ok(fft_opts(ctx), N * batch)) ? pl.p : 0;
}

}  // namespace tsdr

extern "C" int tsdr_fft_plan(size_t n, unsigned *factors, int cap) {
  using namespace tsdr;
  if (n < 2) return 0;
  return fft_split(n, fft_big_ok(FftOpts{}, n), factors, cap);   // (the default options, one transform)
}
