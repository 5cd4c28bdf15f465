// spectra64.hip -- getWelch / getWaterfall (GetSpectrum.jl:36-66) and the resampler! closure (Resampler.jl:26-62) on Float64 /
// ComplexF64, with transforms of their own (fft64.hip's one-launch-per-factor passes are set-up code: no batch, sincospi per
// element).  One engine under all of it: a complex f64 Stockham transform of a tile of at most 4096 values held in LDS
// (64 KiB), radix 2 / 3 / 4 / 5 passes, every thread reading its butterflies' inputs into registers, a barrier, then writing
// their outputs in place; twiddles from a table per length (tw64, built once on the host in long double, cached on the
// context).  Routes:
//   getWelch / getWaterfall, sizeFFT = 2^a 3^b 5^c <= 4096: k_seg64 -- a workgroup loads whole segments (Float64 widened to
//     (x, 0), or ComplexF64) straight from the caller's buffer into LDS, transforms them and either adds abs2 (re*re + im*im, no
//     FMA) per frequency into registers across the segments it walks (Welch: one partial row per workgroup, then
//     k_welch64_sum adds the rows in index order, fftshift, 10log10) or writes fftshift(abs2) into the segment's column of
//     sMatrix (waterfall).  No segment spectrum goes through HBM.
//   any other sizeFFT: segments in chunks through HBM (WS_F64_A / _B), transformed batched: k_col64 passes (each factor
//     <= 4096 through the LDS engine) for larger smooth lengths, Bluestein on a power-of-two length for the rest.
//   resampler!, N = bufferSize * upCoeff: N <= 4096 smooth -- one workgroup, one launch (k_resamp64_small); larger smooth N --
//     two or three k_col64 passes per transform, the zero-stuffing the forward transform's first loader, the H multiply the
//     inverse transform's first loader, 2 upCoeff real(.) the store of its last pass; anything else -- fft64_d.
// Everything here transforms in WS_F64_* or the resampler's own buffers: no f64 call moves a workspace of the f32 paths.
#include <algorithm>
#include <cmath>
#include <vector>

#include "fft_dev.h"
#include "resampler_state.h"

namespace tsdr {


constexpr int kT64 = 256;          // threads of every workgroup here
constexpr int kTile64 = 4096;      // complex f64 values one workgroup holds in LDS at most (64 KiB)
constexpr size_t kTwSplit = 4096;  // two-level tables above this length: W_n^e = hi[e / 4096] * lo[e % 4096]

struct Plan64 {           // radices of one LDS-resident transform, in pass order
  unsigned char r[16];
  int np;
};

__device__ inline double2 zadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ inline double2 zsub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ inline double2 zmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline double2 zscl(double2 a, double c) { return make_double2(a.x * c, a.y * c); }
__device__ inline double2 zrot(double2 v, double sg) { return make_double2(-sg * v.y, sg * v.x); }   // sg * i * v
__device__ inline double pow64(double2 c) { return __dadd_rn(__dmul_rn(c.x, c.x), __dmul_rn(c.y, c.y)); }
__device__ inline size_t shift64(size_t j, size_t N) {   // fftshift: output j takes input (j + ceil(N/2)) mod N
  const size_t s = j + (N - N / 2);
  return s >= N ? s - N : s;
}

// y_u = sum_t a_t W_R^(t u), W_R = exp(sg 2 pi i / R)
template <int R>
__device__ inline void dft64(double2 (&a)[R], double sg) {
  if constexpr (R == 2) {
    const double2 t = a[0];
    a[0] = zadd(t, a[1]); a[1] = zsub(t, a[1]);
  } else if constexpr (R == 3) {
    const double h = 0.86602540378443864676;   // sin(2 pi / 3)
    const double2 b = zadd(a[1], a[2]), d = zscl(zsub(a[1], a[2]), h);
    const double2 m = make_double2(a[0].x - 0.5 * b.x, a[0].y - 0.5 * b.y), r = zrot(d, sg);
    a[0] = zadd(a[0], b); a[1] = zadd(m, r); a[2] = zsub(m, r);
  } else if constexpr (R == 4) {
    const double2 t0 = zadd(a[0], a[2]), t1 = zsub(a[0], a[2]), t2 = zadd(a[1], a[3]), t3 = zrot(zsub(a[1], a[3]), sg);
    a[0] = zadd(t0, t2); a[2] = zsub(t0, t2); a[1] = zadd(t1, t3); a[3] = zsub(t1, t3);
  } else {
    static_assert(R == 5, "radix");
    const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;   // cos(2 pi / 5), cos(4 pi / 5)
    const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;    // sin(2 pi / 5), sin(4 pi / 5)
    const double2 b1 = zadd(a[1], a[4]), d1 = zsub(a[1], a[4]), b2 = zadd(a[2], a[3]), d2 = zsub(a[2], a[3]);
    const double2 m1 = zadd(a[0], zadd(zscl(b1, c1), zscl(b2, c2))), m2 = zadd(a[0], zadd(zscl(b1, c2), zscl(b2, c1)));
    const double2 r1 = zrot(zadd(zscl(d1, s1), zscl(d2, s2)), sg), r2 = zrot(zsub(zscl(d1, s2), zscl(d2, s1)), sg);
    a[0] = zadd(a[0], zadd(b1, b2)); a[1] = zadd(m1, r1); a[4] = zsub(m1, r1); a[2] = zadd(m2, r2); a[3] = zsub(m2, r2);
  }
}

// One Stockham pass of radix R over nseg transforms of length len held at lds[seg * ld + i] (n = len / s, m = n / R):
//   y[q + s (R p + u)] = W_n^(p u) sum_t x[q + s (p + t m)] W_R^(t u),   p < m, q < s
// tw: W_len^e = exp(-2 pi i e / len), e < len (conjugated when sg > 0).  Reads, barrier, writes, barrier.
template <int R, int TILE>
__device__ void lds_pass64(double2 *lds, unsigned len, unsigned nseg, unsigned ld, unsigned s, const double2 *__restrict__ tw, double sg) {
  constexpr int KB = (TILE / R + kT64 - 1) / kT64;
  const unsigned nb = len / R, tot = nb * nseg, m = len / s / R;
  double2 v[KB][R];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const unsigned g = threadIdx.x + k * kT64;
    if (g < tot) {
      const unsigned sgm = g / nb, gg = g - sgm * nb, p = gg / s, q = gg - p * s;
      const double2 *x = lds + sgm * ld + q + s * p;
#pragma unroll
      for (int t = 0; t < R; ++t) v[k][t] = x[s * m * t];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const unsigned g = threadIdx.x + k * kT64;
    if (g < tot) {
      const unsigned sgm = g / nb, gg = g - sgm * nb, p = gg / s, q = gg - p * s;
      dft64<R>(v[k], sg);
      double2 *y = lds + sgm * ld + q + s * R * p;
      y[0] = v[k][0];
#pragma unroll
      for (int u = 1; u < R; ++u) {
        double2 w = tw[p * u * s];
        if (sg > 0) w.y = -w.y;
        y[s * u] = p ? zmul(v[k][u], w) : v[k][u];
      }
    }
  }
  __syncthreads();
}

// the whole transform of each of the nseg rows (unnormalised both ways); nseg * len <= TILE
template <int TILE>
__device__ void lds_fft64(double2 *lds, unsigned len, unsigned nseg, unsigned ld, const Plan64 &pl, const double2 *__restrict__ tw, double sg) {
  unsigned s = 1;
  for (int i = 0; i < pl.np; ++i) {
    switch (pl.r[i]) {
      case 2: lds_pass64<2, TILE>(lds, len, nseg, ld, s, tw, sg); break;
      case 3: lds_pass64<3, TILE>(lds, len, nseg, ld, s, tw, sg); break;
      case 4: lds_pass64<4, TILE>(lds, len, nseg, ld, s, tw, sg); break;
      default: lds_pass64<5, TILE>(lds, len, nseg, ld, s, tw, sg); break;
    }
    s *= pl.r[i];
  }
}

// ---- segments of at most 4096 points: load, transform, reduce without leaving the chip ----------------------------------
enum { SEG64_WELCH = 0, SEG64_WATERFALL = 1, SEG64_ROWS = 2 };

// G segments of N points per tile (G N <= TILE), tiles [blockIdx.x * tpw, ...) walked in order.  WELCH: thread slot f of the
// tile (f = threadIdx.x + 256 j) keeps sum over the walked tiles of abs2(X_tile[f]); at the end the slots of one frequency are
// added in segment order into part[blockIdx.x][k].  WATERFALL: outm[seg * N + j] = abs2(X_seg[shift(j)]).  ROWS: the spectra
// themselves into rows[seg * N + k] (batched transform for the chunked routes; in place when rows == sig).
template <int MODE, bool CPLX, int TILE>
__global__ __launch_bounds__(kT64) void k_seg64(const double *__restrict__ sig, size_t nbSeg, unsigned N, unsigned G, Plan64 pl,
                                                const double2 *__restrict__ tw, double sg, size_t tpw, double *__restrict__ part,
                                                double *__restrict__ outm, double2 *rows) {
  extern __shared__ double2 lds64[];
  constexpr int KA = TILE / kT64;
  const unsigned GN = G * N;
  const size_t ntiles = (nbSeg + G - 1) / G;
  const size_t t0 = (size_t)blockIdx.x * tpw, t1 = t0 + tpw < ntiles ? t0 + tpw : ntiles;
  double acc[KA];
#pragma unroll
  for (int j = 0; j < KA; ++j) acc[j] = 0.0;
  for (size_t tile = t0; tile < t1; ++tile) {
    const size_t seg0 = tile * G, e0 = seg0 * N;
    const unsigned nvalid = (unsigned)((nbSeg - seg0 < G ? nbSeg - seg0 : G) * N);
#pragma unroll
    for (int j = 0; j < KA; ++j) {
      const unsigned f = threadIdx.x + j * kT64;
      if (f < GN) {
        double2 v = make_double2(0.0, 0.0);
        if (f < nvalid) v = CPLX ? reinterpret_cast<const double2 *>(sig)[e0 + f] : make_double2(sig[e0 + f], 0.0);
        lds64[f] = v;
      }
    }
    __syncthreads();
    lds_fft64<TILE>(lds64, N, G, N, pl, tw, sg);
#pragma unroll
    for (int j = 0; j < KA; ++j) {
      const unsigned f = threadIdx.x + j * kT64;
      if (f < nvalid) {
        if (MODE == SEG64_WELCH) {
          acc[j] += pow64(lds64[f]);
        } else if (MODE == SEG64_WATERFALL) {
          const unsigned g = f / N, k = f - g * N;
          outm[e0 + f] = pow64(lds64[g * N + shift64(k, N)]);
        } else {
          rows[e0 + f] = lds64[f];
        }
      }
    }
    __syncthreads();
  }
  if (MODE == SEG64_WELCH) {
    double *dl = reinterpret_cast<double *>(lds64);
#pragma unroll
    for (int j = 0; j < KA; ++j) {
      const unsigned f = threadIdx.x + j * kT64;
      if (f < GN) dl[f] = acc[j];
    }
    __syncthreads();
    for (unsigned k = threadIdx.x; k < N; k += kT64) {
      double S = 0.0;
      for (unsigned g = 0; g < G; ++g) S += dl[g * N + k];
      part[(size_t)blockIdx.x * N + k] = S;
    }
  }
}

// y[j] = sum over rows c of part[c][shift(j)], 10log10 unless lin: sixteen interleaved partial sums per frequency (rows g, g + 16,
// ...), then those in order of g.  nparts == 0: zeros (-Inf dB), the reference's zero-initialised accumulator.
__global__ __launch_bounds__(256) void k_welch64_sum(const double *__restrict__ part, size_t N, unsigned nparts, int lin, double *__restrict__ y) {
  __shared__ double sm[16][17];
  const int kq = threadIdx.x & 15, g = threadIdx.x >> 4;
  const size_t j = (size_t)blockIdx.x * 16 + kq;
  const size_t k = j < N ? shift64(j, N) : 0;
  double t = 0.0;
  if (j < N)
    for (unsigned c = g; c < nparts; c += 16) t += part[(size_t)c * N + k];
  sm[g][kq] = t;
  __syncthreads();
  if (g == 0 && j < N) {
    double S = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) S += sm[i][kq];
    y[j] = lin ? S : __dmul_rn(10.0, log10(S));
  }
}

// ---- one LDS-blocked pass of a long transform ----------------------------------------------------------------------------
// The big Stockham pass of radix R <= 4096 at stride s of a length-N transform (batch blockIdx.y, rows N apart): column
// c = q + s p (c < N / R) holds x[c + t N / R], t < R; the workgroup loads C consecutive columns (coalesced along c), transforms
// each in LDS (row stride ld), multiplies output u by W_N^(s p u) and stores it at q + s (R p + u).
enum { LD64_C = 0, LD64_STUFF = 1, LD64_MULH = 2 };
enum { ST64_C = 0, ST64_REAL = 1 };
struct Col64 {
  const double2 *src;   // LD64_C / LD64_MULH input
  const double *in;     // LD64_STUFF: the resampler's bufferSize real inputs, src[k] = (in[k / up], 0) where up | k, else 0
  const double2 *H;     // LD64_MULH: src[k] * H[k]
  double2 *dst;         // ST64_C
  double *out;          // ST64_REAL: out[k] = gain * (re * invN)
  size_t N, s;
  unsigned R, C, ld, up;
  double sg, invN, gain;
  const double2 *twN;   // two-level W_N table
  const double2 *twR;   // W_R table of the LDS passes
  Plan64 pl;
};

template <int LD, int ST>
__global__ __launch_bounds__(kT64) void k_col64(Col64 a) {
  extern __shared__ double2 lds64[];
  const size_t ncol = a.N / a.R, c0 = (size_t)blockIdx.x * a.C, boff = (size_t)blockIdx.y * a.N;
  const unsigned cv = (unsigned)(ncol - c0 < a.C ? ncol - c0 : a.C);
  const unsigned tot = a.C * a.R;
  for (unsigned e = threadIdx.x; e < tot; e += kT64) {
    const unsigned t = e / a.C, i = e - t * a.C;
    double2 v = make_double2(0.0, 0.0);
    if (i < cv) {
      const size_t k = c0 + i + (size_t)t * ncol;
      if (LD == LD64_STUFF) {
        const size_t j = k / a.up;
        if (j * a.up == k) v = make_double2(a.in[j], 0.0);
      } else if (LD == LD64_MULH) {
        v = zmul(a.src[boff + k], a.H[k]);
      } else {
        v = a.src[boff + k];
      }
    }
    lds64[i * a.ld + t] = v;
  }
  __syncthreads();
  lds_fft64<kTile64>(lds64, a.R, a.C, a.ld, a.pl, a.twR, a.sg);
  const bool first = a.s == 1;   // columns are consecutive p: outputs of one column are contiguous
  for (unsigned e = threadIdx.x; e < tot; e += kT64) {
    unsigned i, u;
    if (first) { i = e / a.R; u = e - i * a.R; } else { u = e / a.C; i = e - u * a.C; }
    if (i >= cv) continue;
    const size_t c = c0 + i, p = c / a.s, q = c - p * a.s, k = q + a.s * ((size_t)a.R * p + u);
    double2 v = lds64[i * a.ld + u];
    const size_t ex = a.s * p * u;
    if (ex) {
      double2 w = zmul(a.twN[kTwSplit + (ex >> 12)], a.twN[ex & 4095]);
      if (a.sg > 0) w.y = -w.y;
      v = zmul(v, w);
    }
    if (ST == ST64_REAL) a.out[k] = a.gain * (v.x * a.invN);
    else a.dst[boff + k] = v;
  }
}

// ---- the resampler in one workgroup (N <= 4096): stuff, fft, * H, ifft, 2 up real ----------------------------------------
__global__ __launch_bounds__(kT64) void k_resamp64_small(const double *__restrict__ in, unsigned N, unsigned up, const double2 *__restrict__ H,
                                                         Plan64 pl, const double2 *__restrict__ tw, double invN, double gain,
                                                         double *__restrict__ out) {
  extern __shared__ double2 lds64[];
  for (unsigned i = threadIdx.x; i < N; i += kT64) lds64[i] = (i % up == 0) ? make_double2(in[i / up], 0.0) : make_double2(0.0, 0.0);
  __syncthreads();
  lds_fft64<kTile64>(lds64, N, 1, N, pl, tw, -1.0);
  for (unsigned i = threadIdx.x; i < N; i += kT64) lds64[i] = zmul(lds64[i], H[i]);
  __syncthreads();
  lds_fft64<kTile64>(lds64, N, 1, N, pl, tw, +1.0);
  for (unsigned i = threadIdx.x; i < N; i += kT64) out[i] = gain * (lds64[i].x * invN);
}

// ---- small streaming kernels of the chunked / fallback routes ----------------------------------------------------------
__global__ __launch_bounds__(256) void k_widen64(const double *__restrict__ sig, int cplx, size_t n, double2 *__restrict__ X) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    X[i] = cplx ? reinterpret_cast<const double2 *>(sig)[i] : make_double2(sig[i], 0.0);
}
// Bluestein on B segments of N points, rows of L: a[b][k] = x[b][k] c[k] for k < N, zero beyond
__global__ __launch_bounds__(256) void k_blue64b_prep(const double *__restrict__ sig, int cplx, size_t N, size_t L, size_t B,
                                                      const double2 *__restrict__ chirp, double2 *__restrict__ X) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < B * L; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / L, k = i - b * L;
    double2 v = make_double2(0.0, 0.0);
    if (k < N) {
      const size_t e = b * N + k;
      v = zmul(cplx ? reinterpret_cast<const double2 *>(sig)[e] : make_double2(sig[e], 0.0), chirp[k]);
    }
    X[i] = v;
  }
}
__global__ __launch_bounds__(256) void k_mulrow64(double2 *__restrict__ X, const double2 *__restrict__ F, size_t L, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) X[i] = zmul(X[i], F[i % L]);
}
__global__ __launch_bounds__(256) void k_blue64b_post(double2 *__restrict__ X, size_t N, size_t L, size_t B, const double2 *__restrict__ chirp, double g) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < B * N; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / N, k = i - b * N;
    X[b * L + k] = zscl(zmul(X[b * L + k], chirp[k]), g);
  }
}
// Welch, chunked: acc[k] (+)= sum over rows b in order of abs2(X[b][k])
__global__ __launch_bounds__(256) void k_welch64_acc(const double2 *__restrict__ X, size_t rs, size_t N, size_t B, int first, double *__restrict__ acc) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += (size_t)gridDim.x * blockDim.x) {
    double S = first ? 0.0 : acc[k];
    for (size_t b = 0; b < B; ++b) S += pow64(X[b * rs + k]);
    acc[k] = S;
  }
}
__global__ __launch_bounds__(256) void k_wf64_rows(const double2 *__restrict__ X, size_t rs, size_t N, size_t B, double *__restrict__ m) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < B * N; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / N, j = i - b * N;
    m[i] = pow64(X[b * rs + shift64(j, N)]);
  }
}
__global__ __launch_bounds__(256) void k_stuff64(const double *__restrict__ in, size_t N, unsigned up, double2 *__restrict__ X) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (size_t)gridDim.x * blockDim.x)
    X[i] = (i % up == 0) ? make_double2(in[i / up], 0.0) : make_double2(0.0, 0.0);
}
__global__ __launch_bounds__(256) void k_mulH64(double2 *__restrict__ X, const double2 *__restrict__ H, size_t N) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (size_t)gridDim.x * blockDim.x) X[i] = zmul(X[i], H[i]);
}
__global__ __launch_bounds__(256) void k_real64(const double2 *__restrict__ X, size_t N, double gain, double *__restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (size_t)gridDim.x * blockDim.x) out[i] = gain * X[i].x;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static bool smooth235(size_t n) {
  if (n == 0) return false;
  for (size_t p : {2, 3, 5})
    while (n % p == 0) n /= p;
  return n == 1;
}

// radices of a smooth len <= 4096: fours first, then a two, threes, fives
static Plan64 plan64(size_t len) {
  Plan64 pl{};
  size_t m = len;
  auto add = [&](unsigned r) { pl.r[pl.np++] = (unsigned char)r; m /= r; };
  while (m % 4 == 0) add(4);
  while (m % 2 == 0) add(2);
  while (m % 3 == 0) add(3);
  while (m % 5 == 0) add(5);
  return pl;
}

// factors <= 4096 of a smooth N > 4096, as few as possible (each <= 1024 when three or fewer passes allow it: a tile then holds
// at least four columns, 64-byte runs along c), largest prime first into the smallest group
static std::vector<size_t> split64(size_t N) {
  std::vector<size_t> primes;
  size_t m = N;
  for (size_t p : {5, 3, 2})
    while (m % p == 0) { primes.push_back(p); m /= p; }
  for (size_t cap : {(size_t)1024, (size_t)4096})
    for (int k = 2; k <= 3 + (cap == 4096 ? 6 : 0); ++k) {
      std::vector<size_t> g(k, 1);
      for (size_t p : primes) *std::min_element(g.begin(), g.end()) *= p;
      if (*std::max_element(g.begin(), g.end()) <= cap) {
        g.erase(std::remove(g.begin(), g.end(), (size_t)1), g.end());
        return g;
      }
    }
  return {};
}

// W_n table (see tsdr_ctx::tw64), built once per n
static const double2 *tw64_table(tsdr_ctx *ctx, size_t n) {
  auto it = ctx->tw64.find(n);
  if (it != ctx->tw64.end()) return it->second;
  const long double w0 = 6.283185307179586476925286766559005768L / (long double)n;
  const size_t count = n <= kTwSplit ? n : kTwSplit + ceil_div(n, kTwSplit), bytes = count * sizeof(double2);
  HostStage st(ctx);   // (owns the table's host image: a wait that gives up leaves the copy reading it)
  double2 *t = (double2 *)st.temp(bytes), *d = nullptr;
  if (!t || hipMalloc((void **)&d, bytes) != hipSuccess) { set_err(ctx, TSDR_ENOMEM, "f64 twiddle table"); return nullptr; }
  size_t m = 0;
  auto put = [&](size_t e) { t[m++] = make_double2((double)cosl(w0 * (long double)e), -(double)sinl(w0 * (long double)e)); };
  if (n <= kTwSplit) {
    for (size_t e = 0; e < n; ++e) put(e);
  } else {
    for (size_t e = 0; e < kTwSplit; ++e) put(e);
    for (size_t h = 0; h * kTwSplit < n; ++h) put(h * kTwSplit);
  }
  st.in_to(d, t, bytes);
  if (st.run("f64 twiddle table")) {
    if (!st.pending()) (void)hipFree(d);   // (a copy that may still run keeps its target: hipFree would wait for it without a bound)
    set_err(ctx, TSDR_EHIP, "f64 twiddle table upload");
    return nullptr;
  }
  ctx->tw64[n] = d;
  return d;
}

// the LDS-blocked passes of a smooth N > 4096, rows N apart, batch rows: `first` loads per ld, the last pass stores per st.
// Returns the buffer that holds the result (X or T) through *res (ST64_REAL: nothing).
static int col_passes(tsdr_ctx *ctx, size_t N, size_t batch, double sg, int ld, const double *in, unsigned up, const double2 *H,
                      double2 *X, double2 *T, int st, double *out, double invN, double gain, double2 **res) {
  const std::vector<size_t> f = split64(N);
  if (f.empty()) return set_err(ctx, TSDR_EINVAL, "f64 transform: no split of %zu", N);
  if (batch >= 65536) return set_err(ctx, TSDR_EINVAL, "f64 transform: batch too large");
  const double2 *twN = tw64_table(ctx, N);
  if (!twN) return TSDR_ENOMEM;
  const double2 *src = X;
  double2 *dst = T;
  size_t s = 1;
  for (size_t i = 0; i < f.size(); ++i) {
    const size_t R = f[i];
    Col64 a{};
    a.twR = tw64_table(ctx, R);
    if (!a.twR) return TSDR_ENOMEM;
    a.src = src; a.in = in; a.H = H; a.dst = dst; a.out = out;
    a.N = N; a.s = s; a.R = (unsigned)R; a.up = up; a.sg = sg; a.invN = invN; a.gain = gain; a.twN = twN;
    a.pl = plan64(R);
    const size_t ncol = N / R;
    a.ld = (unsigned)R;
    a.C = (unsigned)std::min<size_t>(ncol, kTile64 / R);
    if (a.C > 1 && (R & 1) == 0 && a.C * (R + 1) <= (size_t)kTile64) a.ld = (unsigned)R + 1;   // odd row stride: fewer LDS bank conflicts
    const size_t shm = (size_t)a.C * a.ld * sizeof(double2);
    const dim3 grid((unsigned)ceil_div(ncol, a.C), (unsigned)batch);
    const bool last = i + 1 == f.size();
    const int l = i == 0 ? ld : LD64_C;
    if (last && st == ST64_REAL) {
      if (l == LD64_MULH) TSDR_LAUNCH(ctx, "col64_pass", (k_col64<LD64_MULH, ST64_REAL>), grid, dim3(kT64), shm, a);
      else TSDR_LAUNCH(ctx, "col64_pass", (k_col64<LD64_C, ST64_REAL>), grid, dim3(kT64), shm, a);
    } else if (l == LD64_STUFF) {
      TSDR_LAUNCH(ctx, "col64_pass", (k_col64<LD64_STUFF, ST64_C>), grid, dim3(kT64), shm, a);
    } else if (l == LD64_MULH) {
      TSDR_LAUNCH(ctx, "col64_pass", (k_col64<LD64_MULH, ST64_C>), grid, dim3(kT64), shm, a);
    } else {
      TSDR_LAUNCH(ctx, "col64_pass", (k_col64<LD64_C, ST64_C>), grid, dim3(kT64), shm, a);
    }
    s *= R;
    src = dst;
    dst = dst == T ? X : T;
  }
  if (res) *res = const_cast<double2 *>(src);
  return TSDR_OK;
}

static unsigned seg64_tile(unsigned N) { return N <= 2048 ? 2048u : 4096u; }

template <int MODE, bool CPLX>
static int launch_seg64(tsdr_ctx *ctx, const char *name, const double *sig, size_t nbSeg, unsigned N, double sg, unsigned nwg_cap,
                        unsigned *nwg_out, double *part, double *outm, double2 *rows) {
  const unsigned tile = seg64_tile(N), G = std::max(1u, tile / N);
  const size_t ntiles = ceil_div(nbSeg, G);
  const size_t occ = tile == 2048 ? 3 : 2;   // resident workgroups per CU (LDS: 32 / 64 KiB each)
  size_t nwg = std::min<size_t>(ntiles, std::min<size_t>(nwg_cap, (size_t)(ctx->cu_count > 0 ? ctx->cu_count : 256) * occ));
  const size_t tpw = ceil_div(ntiles, nwg);
  nwg = ceil_div(ntiles, tpw);
  const double2 *tw = tw64_table(ctx, N);
  if (!tw) return TSDR_ENOMEM;
  const Plan64 pl = plan64(N);
  const size_t shm = (size_t)G * N * sizeof(double2);
  if (tile == 2048)
    TSDR_LAUNCH(ctx, name, (k_seg64<MODE, CPLX, 2048>), dim3((unsigned)nwg), dim3(kT64), shm, sig, nbSeg, N, G, pl, tw, sg, tpw, part, outm, rows);
  else
    TSDR_LAUNCH(ctx, name, (k_seg64<MODE, CPLX, 4096>), dim3((unsigned)nwg), dim3(kT64), shm, sig, nbSeg, N, G, pl, tw, sg, tpw, part, outm, rows);
  if (nwg_out) *nwg_out = (unsigned)nwg;
  return TSDR_OK;
}

// the most workgroups a fast-route Welch call uses (rows of WS_F64_C it needs)
static size_t welch64_max_parts(tsdr_ctx *ctx) { return (size_t)(ctx->cu_count > 0 ? ctx->cu_count : 256) * 3; }

// unnormalised transforms (sg -1 forward, +1 inverse) of B rows of n points (rows n apart), in place in X (T: as much scratch)
static int fft64_rows(tsdr_ctx *ctx, double2 *X, double2 *T, size_t n, size_t B, double sg) {
  if (n <= kTwSplit) {
    if (B >= (size_t(1) << 31) / std::max<size_t>(1, n)) return set_err(ctx, TSDR_EINVAL, "f64 transform: batch too large");
    return launch_seg64<SEG64_ROWS, true>(ctx, "rows64", reinterpret_cast<const double *>(X), B, (unsigned)n, sg, 1u << 30, nullptr,
                                          nullptr, nullptr, X);
  }
  double2 *res = nullptr;
  if (int rc = col_passes(ctx, n, B, sg, LD64_C, nullptr, 1, nullptr, X, T, ST64_C, nullptr, 1.0, 1.0, &res)) return rc;
  if (res != X) TSDR_HIP(ctx, hipMemcpyAsync(X, res, B * n * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));
  return TSDR_OK;
}

// Bluestein tables of length n (tsdr_ctx::blu64): chirp c[k] = exp(-i pi k^2 / n), k < n (k^2 reduced mod 2n exactly), then
// FFT_L of the wrapped conj chirp
static const double2 *blu64_tables(tsdr_ctx *ctx, size_t n, size_t L, double2 *X, double2 *T) {
  auto it = ctx->blu64.find(n);
  if (it != ctx->blu64.end()) return it->second;
  HostStage st(ctx);   // (owns the tables' host image, as in tw64_table)
  double2 *h = (double2 *)st.temp((n + L) * sizeof(double2));
  if (!h) { set_err(ctx, TSDR_ENOMEM, "f64 Bluestein tables"); return nullptr; }
  for (size_t k = 0; k < n + L; ++k) h[k] = make_double2(0.0, 0.0);
  const long double pi = 3.141592653589793238462643383279502884L;
  for (size_t k = 0; k < n; ++k) {
    const unsigned long long e = (unsigned long long)(((unsigned __int128)k * k) % (2 * (unsigned __int128)n));
    const long double a = pi * (long double)e / (long double)n;
    h[k] = make_double2((double)cosl(a), -(double)sinl(a));
    const double2 cc = make_double2(h[k].x, -h[k].y);
    h[n + k] = cc;
    if (k) h[n + L - k] = cc;
  }
  double2 *d = nullptr;
  if (hipMalloc((void **)&d, (n + L) * sizeof(double2)) != hipSuccess) { set_err(ctx, TSDR_ENOMEM, "f64 Bluestein tables"); return nullptr; }
  st.in_to(X, h + n, L * sizeof(double2));   // the wrapped conj chirp, transformed in place below
  st.in_to(d, h, n * sizeof(double2));       // (goes up with it now, not behind the transform: the two touch different memory)
  int rc = st.begin();
  if (!rc) rc = fft64_rows(ctx, X, T, L, 1, -1.0);
  if (!rc && hipMemcpyAsync(d + n, X, L * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) rc = TSDR_EHIP;
  if (!rc) rc = st.finish("f64 Bluestein tables");
  if (rc) {
    if (!st.pending()) (void)hipFree(d);   // (as in tw64_table)
    set_err(ctx, TSDR_EHIP, "f64 Bluestein tables");
    return nullptr;
  }
  ctx->blu64[n] = d;
  return d;
}

// Segments s0 .. s0 + B of N points from sig, transformed: rows of X, rs apart (N smooth: rs = N; Bluestein: rs = L)
static int segs64_chunk(tsdr_ctx *ctx, const double *sig, int cplx, size_t N, size_t s0, size_t B, double2 *X, double2 *T, size_t *rs) {
  const double *base = sig + s0 * N * (cplx ? 2 : 1);
  if (smooth235(N)) {
    *rs = N;
    TSDR_LAUNCH(ctx, "seg64_widen", k_widen64, dim3(stream_grid(ctx, B * N)), dim3(256), 0, base, cplx, B * N, X);
    return fft64_rows(ctx, X, T, N, B, -1.0);
  }
  size_t L = 1;
  while (L < 2 * N - 1) L <<= 1;
  *rs = L;
  const double2 *bt = blu64_tables(ctx, N, L, X, T);
  if (!bt) return TSDR_ENOMEM;
  TSDR_LAUNCH(ctx, "seg64_blue_prep", k_blue64b_prep, dim3(stream_grid(ctx, B * L)), dim3(256), 0, base, cplx, N, L, B, bt, X);
  if (int rc = fft64_rows(ctx, X, T, L, B, -1.0)) return rc;
  TSDR_LAUNCH(ctx, "seg64_blue_mul", k_mulrow64, dim3(stream_grid(ctx, B * L)), dim3(256), 0, X, bt + N, L, B * L);
  if (int rc = fft64_rows(ctx, X, T, L, B, +1.0)) return rc;
  TSDR_LAUNCH(ctx, "seg64_blue_post", k_blue64b_post, dim3(stream_grid(ctx, B * N)), dim3(256), 0, X, N, L, B, bt, 1.0 / (double)L);
  return TSDR_OK;
}

}  // namespace tsdr

namespace tsdr {

static int welch64_core(tsdr_ctx *ctx, const double *sig, int cplx, size_t len, size_t N, int lin, double *y) {
  const size_t nbSeg = len / N;
  if (nbSeg == 0) {   // sum over no segments: zeros (-Inf dB), as the reference's zero-initialised accumulator gives
    TSDR_LAUNCH(ctx, "welch64_sum", k_welch64_sum, dim3((unsigned)ceil_div(N, 16)), dim3(256), 0, (const double *)nullptr, N, 0u, lin, y);
    return TSDR_OK;
  }
  if (N <= kTwSplit && smooth235(N) && nbSeg < (size_t(1) << 40)) {
    double *part = (double *)ctx->scratch(WS_F64_C, welch64_max_parts(ctx) * N * sizeof(double));
    if (!part) return TSDR_ENOMEM;
    unsigned nwg = 0;
    int rc = cplx ? launch_seg64<SEG64_WELCH, true>(ctx, "welch64_seg", sig, nbSeg, (unsigned)N, -1.0, (unsigned)welch64_max_parts(ctx), &nwg, part, nullptr, nullptr)
                  : launch_seg64<SEG64_WELCH, false>(ctx, "welch64_seg", sig, nbSeg, (unsigned)N, -1.0, (unsigned)welch64_max_parts(ctx), &nwg, part, nullptr, nullptr);
    if (rc) return rc;
    TSDR_LAUNCH(ctx, "welch64_sum", k_welch64_sum, dim3((unsigned)ceil_div(N, 16)), dim3(256), 0, (const double *)part, N, nwg, lin, y);
    return TSDR_OK;
  }
  // chunked: segments through WS_F64_A / _B, their power added into one row (WS_F64_C) chunk after chunk
  size_t Lw = N;
  if (!smooth235(N)) { Lw = 1; while (Lw < 2 * N - 1) Lw <<= 1; }
  const size_t B = std::max<size_t>(1, std::min<size_t>({nbSeg, (size_t(1) << 22) / Lw, 65535}));
  double2 *X = (double2 *)ctx->scratch(WS_F64_A, B * Lw * sizeof(double2));
  double2 *T = (double2 *)ctx->scratch(WS_F64_B, B * Lw * sizeof(double2));
  double *acc = (double *)ctx->scratch(WS_F64_C, N * sizeof(double));
  if (!X || !T || !acc) return TSDR_ENOMEM;
  for (size_t s0 = 0; s0 < nbSeg; s0 += B) {
    const size_t b = std::min(B, nbSeg - s0);
    size_t rs = 0;
    if (int rc = segs64_chunk(ctx, sig, cplx, N, s0, b, X, T, &rs)) return rc;
    TSDR_LAUNCH(ctx, "welch64_acc", k_welch64_acc, dim3(stream_grid(ctx, N)), dim3(256), 0, (const double2 *)X, rs, N, b, (int)(s0 == 0), acc);
  }
  TSDR_LAUNCH(ctx, "welch64_sum", k_welch64_sum, dim3((unsigned)ceil_div(N, 16)), dim3(256), 0, (const double *)acc, N, 1u, lin, y);
  return TSDR_OK;
}

static int waterfall64_core(tsdr_ctx *ctx, const double *sig, int cplx, size_t len, size_t N, double *m) {
  const size_t nbSeg = len / N;
  if (nbSeg == 0) return TSDR_OK;
  if (N <= kTwSplit && smooth235(N) && nbSeg < (size_t(1) << 40)) {
    return cplx ? launch_seg64<SEG64_WATERFALL, true>(ctx, "waterfall64_seg", sig, nbSeg, (unsigned)N, -1.0, 1u << 30, nullptr, nullptr, m, nullptr)
                : launch_seg64<SEG64_WATERFALL, false>(ctx, "waterfall64_seg", sig, nbSeg, (unsigned)N, -1.0, 1u << 30, nullptr, nullptr, m, nullptr);
  }
  size_t Lw = N;
  if (!smooth235(N)) { Lw = 1; while (Lw < 2 * N - 1) Lw <<= 1; }
  const size_t B = std::max<size_t>(1, std::min<size_t>({nbSeg, (size_t(1) << 22) / Lw, 65535}));
  double2 *X = (double2 *)ctx->scratch(WS_F64_A, B * Lw * sizeof(double2));
  double2 *T = (double2 *)ctx->scratch(WS_F64_B, B * Lw * sizeof(double2));
  if (!X || !T) return TSDR_ENOMEM;
  for (size_t s0 = 0; s0 < nbSeg; s0 += B) {
    const size_t b = std::min(B, nbSeg - s0);
    size_t rs = 0;
    if (int rc = segs64_chunk(ctx, sig, cplx, N, s0, b, X, T, &rs)) return rc;
    TSDR_LAUNCH(ctx, "waterfall64_rows", k_wf64_rows, dim3(stream_grid(ctx, b * N)), dim3(256), 0, (const double2 *)X, rs, N, b, m + s0 * N);
  }
  return TSDR_OK;
}

static int resampler64_core(tsdr_resampler *r, const double *in, double *out) {
  tsdr_ctx *ctx = r->ctx;
  const size_t N = r->sizeFFT;
  const double invN = 1.0 / (double)N, gain = (double)(2 * r->up);
  if (smooth235(N) && N <= kTwSplit) {   // one workgroup, one launch
    const double2 *tw = tw64_table(ctx, N);
    if (!tw) return TSDR_ENOMEM;
    TSDR_LAUNCH(ctx, "resampler64_small", k_resamp64_small, dim3(1), dim3(kT64), N * sizeof(double2), in, (unsigned)N, (unsigned)r->up,
                (const double2 *)r->H, plan64(N), tw, invN, gain, out);
    return TSDR_OK;
  }
  if (smooth235(N)) {
    // two transforms of LDS-blocked passes and nothing else: the zero-stuffing is the forward transform's first loader (it reads
    // the bufferSize inputs only), the filter the inverse transform's, 2 upCoeff real(.) the store of its last pass
    double2 *F = nullptr;
    if (int rc = col_passes(ctx, N, 1, -1.0, LD64_STUFF, in, (unsigned)r->up, nullptr, r->A64, r->B64, ST64_C, nullptr, 1.0, 1.0, &F)) return rc;
    double2 *G = F == r->A64 ? r->B64 : r->A64;
    return col_passes(ctx, N, 1, +1.0, LD64_MULH, nullptr, 1, r->H, F, G, ST64_REAL, out, invN, gain, nullptr);
  }
  // any other length: fft64.hip's transform (Stockham passes / Bluestein) with plain stuff, multiply and real kernels
  TSDR_LAUNCH(ctx, "resampler64_stuff", k_stuff64, dim3(stream_grid(ctx, N)), dim3(256), 0, in, N, (unsigned)r->up, r->A64);
  if (int rc = fft64_d(ctx, r->A64, r->B64, N, -1)) return rc;
  TSDR_LAUNCH(ctx, "resampler64_filter", k_mulH64, dim3(stream_grid(ctx, N)), dim3(256), 0, r->A64, (const double2 *)r->H, N);
  if (int rc = fft64_d(ctx, r->A64, r->B64, N, +1)) return rc;
  TSDR_LAUNCH(ctx, "resampler64_out", k_real64, dim3(stream_grid(ctx, N)), dim3(256), 0, (const double2 *)r->A64, N, gain, out);
  return TSDR_OK;
}

}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_welch_f64_d(tsdr_ctx *ctx, const double *sig, int is_complex, size_t len, size_t sizeFFT, int lin, double *y) {
  if (!ctx || !y || (len && !sig)) return TSDR_EINVAL;
  if (sizeFFT == 0) return set_err(ctx, TSDR_EINVAL, "welch_f64: sizeFFT must be positive");
  if (is_complex && ((uintptr_t)sig & 15)) return set_err(ctx, TSDR_EINVAL, "welch_f64: complex input must be 16-byte aligned");
  return welch64_core(ctx, sig, is_complex, len, sizeFFT, lin, y);
}

int tsdr_welch_f64(tsdr_ctx *ctx, const double *sig, int is_complex, size_t len, size_t sizeFFT, int lin, double *y) {
  if (!ctx) return TSDR_EINVAL;
  if (sizeFFT == 0) return set_err(ctx, TSDR_EINVAL, "welch_f64: sizeFFT must be positive");
  return host_map(ctx, sig, len * (is_complex ? 16 : 8), y, sizeFFT * 8,
                  [&](void *i, void *o) { return welch64_core(ctx, (const double *)i, is_complex, len, sizeFFT, lin, (double *)o); });
}

int tsdr_waterfall_f64_d(tsdr_ctx *ctx, const double *sig, int is_complex, size_t len, size_t sizeFFT, double *sMatrix) {
  if (!ctx || (len && !sig)) return TSDR_EINVAL;
  if (sizeFFT == 0) return set_err(ctx, TSDR_EINVAL, "waterfall_f64: sizeFFT must be positive");
  if (len / sizeFFT && !sMatrix) return TSDR_EINVAL;
  if (is_complex && ((uintptr_t)sig & 15)) return set_err(ctx, TSDR_EINVAL, "waterfall_f64: complex input must be 16-byte aligned");
  return waterfall64_core(ctx, sig, is_complex, len, sizeFFT, sMatrix);
}

int tsdr_waterfall_f64(tsdr_ctx *ctx, const double *sig, int is_complex, size_t len, size_t sizeFFT, double *sMatrix) {
  if (!ctx) return TSDR_EINVAL;
  if (sizeFFT == 0) return set_err(ctx, TSDR_EINVAL, "waterfall_f64: sizeFFT must be positive");
  const size_t nb = len / sizeFFT;
  return host_map(ctx, sig, len * (is_complex ? 16 : 8), sMatrix, nb * sizeFFT * 8,
                  [&](void *i, void *o) { return waterfall64_core(ctx, (const double *)i, is_complex, len, sizeFFT, (double *)o); });
}

int tsdr_resampler_init_f64(tsdr_ctx *ctx, size_t bufferSize, int upCoeff, tsdr_resampler **out) {
  return resampler_init_kind(ctx, bufferSize, upCoeff, true, out);
}

int tsdr_resampler_run_f64_d(tsdr_resampler *r, const double *in, size_t n_in, double *out) {
  if (!r || !in || !out) return TSDR_EINVAL;
  if (!r->f64) return set_err(r->ctx, TSDR_EINVAL, "resampler!: a Float32 resampler takes Float32 buffers (tsdr_resampler_run)");
  if (n_in != r->bufferSize) return set_err(r->ctx, TSDR_EINVAL, "Size of input %zu should match size used during init %zu", n_in, r->bufferSize);
  return resampler64_core(r, in, out);
}

int tsdr_resampler_run_f64(tsdr_resampler *r, const double *in, size_t n_in, double *out) {
  if (!r) return TSDR_EINVAL;
  if (!r->f64) return set_err(r->ctx, TSDR_EINVAL, "resampler!: a Float32 resampler takes Float32 buffers (tsdr_resampler_run)");
  if (n_in != r->bufferSize) return set_err(r->ctx, TSDR_EINVAL, "Size of input %zu should match size used during init %zu", n_in, r->bufferSize);
  return host_map(r->ctx, in, n_in * 8, out, r->sizeFFT * 8,
                  [&](void *i, void *o) { return resampler64_core(r, (const double *)i, (double *)o); });
}

}  // extern "C"
