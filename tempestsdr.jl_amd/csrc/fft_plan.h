// fft_plan.h -- what a transform will launch, decided as a value before anything is launched.
//
// plan_fft(request, options) returns an FftPlan: a status, an error text and an ordered list of steps.  A step names its kernel
// (family + index into the family's entry list below + mode), its profile name, grid, block and dynamic LDS bytes, the buffers
// it reads and writes as ROLES (the caller's in / out, WS_FFT_B, the fused autocorrelation's second buffer), the tables that
// have to exist before it runs, and its filled parameter struct.  Pointers the REQUEST carries (loader factor array, epilogue,
// the whole-row sinks) are copied into the parameters; buffer and table pointers are the launcher's to resolve
// (fft_mixed.hip:launch_step, the only place that launches a pass kernel; the library hands it each step as the plan's sink).  The same header plans the whole-row launches
// (plan_rows) and the fused autocorrelation sequence (plan_autocorr: forward strided steps, the middle, the inverse steps).
//
// Nothing here makes a HIP call or sees a tsdr_ctx: tools/host_plan/fft_plan_dump_main.hip compiles it host-only and prints
// every decision for a list of cases, and tests/test_fft_plan_host.py compares that with a record made from the code that
// decided all this while it launched (tests/golden/fft_plans_v1.txt; NOTEBOOK.md, "FFT plans").
//
// The entry lists (TSDR_MIX2_LIST, ...) exist once: the geometry tables here and the kernel-pointer tables of fft_mixed.hip are
// both expanded from them, so index i is the same instantiation on both sides by construction.
#pragma once
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdarg>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "fft_dev.h"

namespace tsdr {

// ---- kernel parameters (by value in the kernel argument segment) -----------------------------------------------------------
struct PassDesc {
  int mode, logR, logT, dir;
  float scale;
  unsigned long long N;  // elements per transform
  unsigned A, B, tiles;  // strided: outer count, inner size (= stride of the DFT index), B/T
  int logNtw, logBnext, logPprev;
  int nprev;
  int logRprev[4];       // radices of the passes before this one (pass order)
  int logR1;
  unsigned Aprime, k1tiles;  // last pass: A / R_1, R_1 / T
  unsigned rows;             // rows mode: number of transforms
  int src_mode;              // first pass loader (SRC_*); only with batch == 1
  unsigned long long src_n;  // real samples behind SRC_REAL / SRC_IQPOW
  unsigned long long keep;   // last pass: complex outputs >= keep (per transform) are not stored
  const float2 *src_aux;     // SRC_MULH: the factor array
  double src_w8;             // fft_load's f64 parameter: the scale of an integer IQ source (else 0)
  FftEpilogue epi;           // last pass: epilogue when epi.out != nullptr (fft_dev.h)
};
typedef void (*fft_pass_fn)(const float2 *, float2 *, PassDesc, const float2 *);
fft_pass_fn fft_pass_kernel(int mode, int logR);   // fft.hip: k_fft_pass<logR, mode>, for the launcher in fft_mixed.hip

enum { MIX_MAX_PASS = 6, MIX_MAX_STAGE = 8 };

struct MixDesc {
  int mode, dir, logT, nst;
  float scale;
  unsigned R;
  unsigned char rad[MIX_MAX_STAGE];  // stage radices, product R
  unsigned long long N;              // elements per transform
  unsigned A, B, tiles;              // strided: outer count, inner size (= stride of the DFT index), ceil(B/T)
  unsigned Bnext, Pprev;             // B / R_{i+1};  R_1..R_{i-1}
  unsigned ntw_hi, ntw_lo;           // floor(2^64 / (Pprev * R * R_{i+1})): twiddle phase e/Ntw as a 32-bit fraction
  unsigned r_hi, r_lo;               // floor(2^64 / R)
  int nprev;
  unsigned Rprev[MIX_MAX_PASS], Wprev[MIX_MAX_PASS];  // radices of the earlier passes and their weights in k
  unsigned R1, Aprime, k1tiles;      // last pass: first radix, A / R_1, ceil(R_1 / T)
  unsigned rows;                     // rows mode: number of transforms
  int src_mode;
  unsigned long long src_n, keep;
  int tw_sets;                       // strided, two-step kernels: inter-pass twiddle sets held in LDS (0: none)
  const float2 *twg;                 // strided, Bnext == 1: W_{R*Rnext}^(col*k) at [k * B + col] (else nullptr)
  const float2 *src_aux;             // SRC_MULH: the factor array
  double src_w8;                     // SRC_POWER with M = 2*src_n not a power of two: 8/M (else 0)
  FftEpilogue epi;                   // last pass: autocorrelation epilogue when epi.out != nullptr
  // rows mode as getWelch's accumulator (GetSpectrum.jl:36-52): nothing is stored per transform; every workgroup walks
  // tiles blockIdx.x, blockIdx.x + gridDim.x, ... of `rows` segments, adds abs2 of every spectrum it forms in registers and
  // leaves ONE partial power spectrum, acc[blockIdx.x * R + k] (natural frequency order).  rows_real: the rows are real f32
  // (1) or integer IQ (fft_dev.h:ROWS_*, converted by the row loader with the scale in src_w8).
  float *acc;
  int rows_real;
  // ... or getWaterfall's writer (GetSpectrum.jl:54-66; three-step kernels only): Float64(abs2) of every spectrum straight from
  // the registers to wf[segment * R + fftshift position], acc unused (non-null only to select the branch)
  double *wf;
  // ... or plain batched row transforms (tsdr_fft_c2c with batch > 1, three-step kernels only): rows_out[row * R + k] = scale * X[k],
  // either direction; may alias the input (a tile's rows are all loaded before any of them is stored)
  float2 *rows_out;
};

// the fused autocorrelation middle (fft_mixed.hip: k_fft_mid, k_fft_mid3)
struct MidDesc {
  unsigned R, Bc, ndir;           // radix, columns N/R, direct columns Bc/2 + 1
  int logT, nprev;                // tile width (direct + mirrored halves), earlier forward factors
  unsigned Rprev[MIX_MAX_PASS];   // forward factors R_1 .. R_{p-1} (column digits, least significant first)
  unsigned r_hi, r_lo;            // floor(2^64 / R)
  unsigned Bnext, ntw_hi, ntw_lo; // inverse pass 2: Bc / R'_2 and floor(2^64 / (R * R'_2))
  int tw_sets;                    // inverse inter-pass twiddle sets per half held in LDS (0: evaluated per output)
  double w8;                      // 8 / (2N): phase unit of W_{2N}^g
};

// MODE of k_fft_mix3 beyond FFT_STRIDED / FFT_LAST: the three whole-row modes = rows of R points, T per tile, walked by
// persistent workgroups (separate instantiations: as run-time branches of one kernel the row store's conjugations and the
// writers' extra live values cost the accumulator 15-60 %)
enum { M3_ACC = 10, M3_WF = 11, M3_ROWS = 12,     // getWelch's accumulator | getWaterfall's writer | batched row transforms
       M3_ACC_IQ = 13, M3_WF_IQ = 14, M3_ROWS_IQ = 15 };   // the same three on integer IQ rows (MixDesc::rows_real = ROWS_SC16 ..): instantiations
                                                           // of their own, so that the ComplexF32 / real ones keep their registers and occupancy

// ---- kernel geometry (compile-time halves of the kernels' tables) -----------------------------------------------------------
template <int RA, int RB>
struct Mix2Geom {
  static constexpr int R = RA * RB;
  static constexpr int tmax() { int t = 1; while (2 * t * R <= 4096 && 2 * t <= 256) t *= 2; return t; }
  static constexpr int TM = tmax();                       // widest tile (columns, a power of two)
  // threads per workgroup: one DFT slot per thread in the larger step when that fits 384 threads (10 x 10 with 32
  // columns: 320 threads, every lane busy in both steps), else 256 threads with several slots each
  static constexpr int BIG = (RA > RB ? RA : RB) * TM;
  static constexpr int NT = BIG <= 384 ? (BIG + 63) / 64 * 64 : 256;
  static constexpr int CA = (RB * TM + NT - 1) / NT;      // step-1 slots per thread
  static constexpr int CB = (RA * TM + NT - 1) / NT;      // step-2 slots per thread
};

template <int RA, int RB, int RC, int LOGT>
struct Mix3Geom {
  static constexpr int R = RA * RB * RC, T = 1 << LOGT;
  static constexpr int S1 = RB * RC * T, S2 = RA * RC * T, S3 = RA * RB * T;
  static constexpr int SMAX = S1 > S2 ? (S1 > S3 ? S1 : S3) : (S2 > S3 ? S2 : S3);
  static constexpr int NT = (SMAX + 63) / 64 * 64;
  static_assert(NT <= 1024, "three-step kernel: a step has more slots than a workgroup has threads");
  static constexpr int PLANE = RB * RC * T + T;
  static constexpr int VMAX = RA > RB ? (RA > RC ? RA : RC) : (RB > RC ? RB : RC);
  static constexpr size_t LDS = ((size_t)RA * PLANE + R) * sizeof(float2);
  // Exchange-tile position of (second digit, third digit n3, column t) within a k1 plane: (n2 RC + n3) T + (t ^ swz(n3)).
  // The passes that read their rows contiguously (FFT_LAST, the fused middle's forward half, getWelch's accumulator) write
  // step 1 with the lanes of a wavefront running along n3: unswizzled that is a stride of T float2 -- 16 (8) lanes of a
  // 16-lane group on the same bank pair, 7.7 (3.8) LDS passes per ds_write_b64 for T = 8 (4), SQ_LDS_BANK_CONFLICT = 3400
  // cycles per workgroup.  The column is XORed with n3 / 2: 2.0 (1.9) passes there, and the other three access patterns
  // (step-1 writes with the column fastest, steps 2 and 3: lanes along t, then n3 or k1) stay conflict-free -- n3 is
  // constant per thread in step 2 and a compile-time constant in step 3, so the swizzle costs a handful of XORs per pass.
  static __device__ __forceinline__ int swz(int n3) { return (n3 >> 1) & (T - 1); }
};

// The entry lists.  X(template arguments...) once per instantiation; order is lookup order.
// two-step pass kernels k_fft_mix2<RA, RB, FFT_STRIDED | FFT_LAST>: the factor sizes that have one (RB > 1 everywhere); for a size
// listed twice the first entry wins.  The balanced splits come first: with RA ~ RB one thread owns one DFT of each step and nobody
// idles, and 10- or 16-point register DFTs keep the kernel near 64 VGPRs; 25 x 5 leaves 3 of 8 lanes without a step-1 DFT at 160 VGPRs.
#define TSDR_MIX2_LIST(X)                                                                                               \
  X(10, 10) X(10, 20) X(10, 5)                                                                                          \
  X(16, 16) X(16, 10) X(16, 9) X(16, 8) X(16, 5) X(25, 10) X(25, 9) X(25, 8)                                            \
  X(25, 5)  X(25, 4)  X(25, 3) X(25, 2) X(10, 9) X(9, 9)   X(9, 8)  X(9, 5)                                             \
  X(8, 8)   X(8, 5)   X(5, 5)
// three-step pass kernels k_fft_mix3<RA, RB, RC, LOGT, every mode>: 8000-point tiles (64 KiB of LDS + the twiddle table):
// 1000 x 8 columns, 2000 x 4; 500 x 8 (4000 points)
// (tiles half as wide -- 32-byte runs -- measured 25.8 / 22.9 us per pass against 18.5 / 19.9 at 2e6 points)
#define TSDR_MIX3_LIST(X) X(10, 10, 10, 3) X(20, 10, 10, 2) X(5, 10, 10, 3)
// k_fft_mix3 in the whole-row modes only (the pass planner does not see these): the power-of-two segment lengths next to the 1024
// that k_seg1024 serves -- 2048 = 16 x 16 x 8 (two segments per tile), 4096 = 16 x 16 x 16 (one), 512 = 8 x 8 x 8 (eight),
// 256 = 8 x 8 x 4 (eight), 128 -- and the round lengths that split into three of the register DFT sizes (4000, 3200, 2500, 1600,
// 1280, 1200, 768; 960 = 20 x 16 x 3 measured slower than the generic kernel: 108 against 88 us); everything else: the generic
// LDS-stage kernel
#define TSDR_WELCH3_LIST(X)                                                                                              \
  X(16, 16, 8, 1) X(16, 16, 16, 0) X(8, 8, 8, 3) X(8, 8, 4, 3) X(8, 4, 4, 4)       /* 2048 4096 512 256 128 */           \
  X(10, 10, 10, 2) X(5, 10, 10, 2)   /* 1000 500 on half the pass kernels' tiles: row / waterfall modes */              \
  /* (1000: rows 50.5 -> 40.8 us, waterfall 57 -> 47 us, but the accumulator 44 -> 50 us; 2000 on 4000-point tiles lost everywhere) */ \
  X(20, 20, 10, 0) X(25, 10, 10, 0) X(20, 16, 10, 0) X(20, 10, 8, 1)                /* 4000 2500 3200 1600 */            \
  X(16, 16, 5, 1) X(20, 20, 3, 1) X(16, 16, 3, 2)                                   /* 1280 1200 768 */
// fused middle k_fft_mid<RA, RB>: last forward factors that have the kernel (the planner puts the factor with the most twos last)
#define TSDR_MID_LIST(X) X(10, 20) X(10, 10) X(16, 16) X(16, 10) X(16, 9) X(16, 8) X(16, 5) X(8, 8) X(8, 5)
// ... and k_fft_mid3<RA, RB, RC, LOGT>: last forward factor = first inverse factor = 2000 or 1000
#define TSDR_MID3_LIST(X) X(20, 10, 10, 2) X(10, 10, 10, 3)

struct Mix2Info { unsigned R, RA; int tm, nt; };
struct Mix3Info { unsigned R; int logT, nt; size_t lds; };
struct MidInfo { unsigned R, RA; int tm, nt; size_t lds3; };   // RA == 0: a three-step kernel, lds3 its dynamic LDS
#define TSDR_X(RA_, RB_) {RA_ * RB_, RA_, Mix2Geom<RA_, RB_>::TM, Mix2Geom<RA_, RB_>::NT},
inline constexpr Mix2Info kMix2[] = {TSDR_MIX2_LIST(TSDR_X)};
#undef TSDR_X
#define TSDR_X(RA_, RB_, RC_, LT_) {RA_ * RB_ * RC_, LT_, Mix3Geom<RA_, RB_, RC_, LT_>::NT, Mix3Geom<RA_, RB_, RC_, LT_>::LDS},
inline constexpr Mix3Info kMix3[] = {TSDR_MIX3_LIST(TSDR_X) TSDR_WELCH3_LIST(TSDR_X)};   // the pass kernels, then the row-only ones
#undef TSDR_X
#define TSDR_X(...) +1
constexpr int kNMix2 = 0 TSDR_MIX2_LIST(TSDR_X), kNMix3Pass = 0 TSDR_MIX3_LIST(TSDR_X), kNMix3 = kNMix3Pass TSDR_WELCH3_LIST(TSDR_X);
constexpr int kNMid2 = 0 TSDR_MID_LIST(TSDR_X), kNMid = kNMid2 TSDR_MID3_LIST(TSDR_X);
#undef TSDR_X
#define TSDR_X(RA_, RB_) {RA_ * RB_, RA_, Mix2Geom<RA_, RB_>::TM, Mix2Geom<RA_, RB_>::NT, 0},
#define TSDR_X3(RA_, RB_, RC_, LT_) \
  {RA_ * RB_ * RC_, 0, 1 << LT_, Mix3Geom<RA_, RB_, RC_, LT_>::NT, Mix3Geom<RA_, RB_, RC_, LT_>::LDS + 2 * (size_t)(1 << LT_) * 4},
inline constexpr MidInfo kMid[] = {TSDR_MID_LIST(TSDR_X) TSDR_MID3_LIST(TSDR_X3)};   // the two-step kernels, then the three-step ones
#undef TSDR_X
#undef TSDR_X3

inline const Mix2Info *mix2_lookup(unsigned R) {
  for (const Mix2Info &e : kMix2)
    if (e.R == R) return &e;
  return nullptr;
}
inline const Mix3Info *mix3_lookup(unsigned R) {   // the pass kernels
  for (int i = 0; i < kNMix3Pass; ++i)
    if (kMix3[i].R == R) return &kMix3[i];
  return nullptr;
}
inline const Mix3Info *welch3_lookup(unsigned R, bool accumulator) {
  if (accumulator)
    if (const Mix3Info *e = mix3_lookup(R)) return e;   // getWelch: the pass kernels' 8000-point tiles measured better
  for (int i = kNMix3Pass; i < kNMix3; ++i)
    if (kMix3[i].R == R) return &kMix3[i];
  return mix3_lookup(R);
}
inline const MidInfo *mid_lookup(unsigned R) {
  for (const MidInfo &e : kMid)
    if (e.R == R) return &e;
  return nullptr;
}

// ---- dynamic LDS ---------------------------------------------------------------------------------------------------------
constexpr size_t kPassLds = (4096 + 256 + 16 + 256 + 256) * sizeof(float2);   // k_fft_pass
inline size_t mix_lds(unsigned R, int logT) {                                  // k_fft_mix
  return ((size_t)R * ((1u << logT) + 1) + R) * sizeof(float2) + ((size_t)R * 2 + 15) / 16 * 16;
}
// k_fft_mix2 (sets twiddle sets of R, at least one) and k_fft_mid (sets per half + the tile's column lists)
inline size_t mix2_tile(unsigned R, unsigned RA, int logT) {
  const size_t T = (size_t)1 << logT, RB = R / RA;
  const size_t SA = (RB << logT) + (T < 32 ? T : 0);
  return std::max((size_t)R * (T + 1), (size_t)RA * SA);
}
inline size_t mix2_lds(unsigned R, unsigned RA, int logT, int tw_sets = 1) {
  return (mix2_tile(R, RA, logT) + (size_t)(1 + std::max(tw_sets, 1)) * R) * sizeof(float2);
}
inline size_t mid2_lds(unsigned R, unsigned RA, int logT, int tw_sets) {
  return (mix2_tile(R, RA, logT) + (size_t)(1 + 2 * tw_sets) * R) * sizeof(float2) + 2 * ((size_t)1 << logT) * 4;
}

// ---- small arithmetic ------------------------------------------------------------------------------------------------------
struct Recip64 { unsigned hi, lo; };
inline Recip64 recip64(unsigned long long d) {   // floor(2^64 / d) as two 32-bit words (phase_q32's reciprocal)
  const auto inv = ((unsigned __int128)1 << 64) / d;
  return Recip64{(unsigned)(inv >> 32), (unsigned)inv};
}
inline unsigned twos(unsigned v) {   // factors of two of v, counted up to 2^4 (every stride a multiple of 16 elements)
  unsigned t = 0;
  while (v % 2 == 0 && t < 4) { v /= 2; ++t; }
  return t;
}
inline int floor_log2(unsigned v) { int l = 0; while ((2u << l) <= v) ++l; return l; }
inline int ceil_log2(unsigned v) { int l = 0; while ((1u << l) < v) ++l; return l; }
// N = 2^a 3^b 5^c?  (the exponents in ex)
inline bool factor235(size_t N, unsigned *ex) {
  ex[0] = ex[1] = ex[2] = 0;
  const unsigned pr[3] = {2, 3, 5};
  size_t m = N;
  for (int i = 0; i < 3; ++i)
    while (m % pr[i] == 0) { m /= pr[i]; ++ex[i]; }
  return m == 1;
}

// Tile width: as wide as 4096 elements allow, narrowed (not below 16 columns = 128-byte runs) until the launch has
// enough workgroups to keep several resident per CU -- a workgroup is a chain of dependent LDS stages, and with one
// or two of them per CU nothing hides that latency.
inline int pick_logT(int maxlog, int minlog, size_t other, size_t span) {
  int logT = std::max(maxlog, 0);
  while (logT > minlog && other * ceil_div(span, (size_t)1 << logT) < 2048) --logT;
  return logT;
}

// ---- the split of a length into passes ---------------------------------------------------------------------------------------
// power of two: the bits dealt evenly over ceil(log2 n / 8) passes
inline int pow2_split(int logN, int *bits) {
  const int p = logN <= 8 ? 1 : (logN + 7) / 8;
  for (int i = 0; i < p; ++i) bits[i] = logN / p + (i < logN % p ? 1 : 0);
  return p;
}

struct MixPlan {
  int p = 0;
  unsigned R[MIX_MAX_PASS];
  std::vector<unsigned char> rad[MIX_MAX_PASS];
};

inline void stage_radices(unsigned e2, unsigned e3, unsigned e5, std::vector<unsigned char> &out) {
  out.clear();
  while (e5 >= 2) { out.push_back(25); e5 -= 2; }
  if (e5) {
    if (e2) { out.push_back(10); --e2; } else out.push_back(5);
  }
  while (e3 >= 2) { out.push_back(9); e3 -= 2; }
  if (e3) out.push_back(3);
  while (e2 >= 4) { out.push_back(16); e2 -= 4; }
  if (e2 == 3) out.push_back(8);
  if (e2 == 2) out.push_back(4);
  if (e2 == 1) out.push_back(2);
}

// What one pass through a factor costs relative to the best kernels (every pass moves the same 16 bytes per point;
// measured on MI355X at 2e6..2e7 points): balanced two-step kernels 1, the 25 x n ones ~1.6, the generic LDS-stage
// kernel ~2.2.
inline double factor_cost(unsigned R) {
  if (mix3_lookup(R)) return 1.35;  // one pass through a three-step kernel (measured against the balanced two-step ones)
  const Mix2Info *e = mix2_lookup(R);
  if (!e) return 2.2;
  return e->RA == 25 ? 1.6 : 1.0;
}

struct PlanSearch {
  unsigned ex[3];
  bool allow_big = true;  // factors of 500 .. 2000 (three-step kernels)
  int best_p = 0;
  double best = 1e30;
  unsigned cur[MIX_MAX_PASS][3], out[MIX_MAX_PASS][3];
  static unsigned val(const unsigned *e) {
    unsigned v = 1;
    for (unsigned i = 0; i < e[0]; ++i) v *= 2;
    for (unsigned i = 0; i < e[1]; ++i) v *= 3;
    for (unsigned i = 0; i < e[2]; ++i) v *= 5;
    return v;
  }
  // factors in non-increasing order (the order is fixed afterwards), depth-first with a cost bound
  void go(int depth, unsigned cap, double cost) {
    if (!(ex[0] | ex[1] | ex[2])) {
      if (depth == 1 && val(cur[0]) > 256) return;  // the three-step kernels are passes of a multi-pass transform only
      // ties: prefer a factor carrying 2^4 (it goes last: every stride a multiple of 16 elements)
      unsigned m2 = 0;
      for (int i = 0; i < depth; ++i) m2 = std::max(m2, std::min(cur[i][0], 4u));
      const double c = cost - 0.01 * m2;
      if (c < best - 1e-9) {
        best = c;
        best_p = depth;
        for (int i = 0; i < depth; ++i) for (int j = 0; j < 3; ++j) out[i][j] = cur[i][j];
      }
      return;
    }
    if (depth == MIX_MAX_PASS) return;
    {
      double rem = 1.0;
      for (unsigned i = 0; i < ex[0]; ++i) rem *= 2;
      for (unsigned i = 0; i < ex[1]; ++i) rem *= 3;
      for (unsigned i = 0; i < ex[2]; ++i) rem *= 5;
      const double need = std::max(1.0, std::ceil(std::log(rem) / std::log((double)cap) - 1e-9));  // passes still to come
      if (depth + (int)need > MIX_MAX_PASS || cost + need >= best + 0.05) return;
    }
    for (unsigned a = 0; a <= ex[0]; ++a)
      for (unsigned b = 0; b <= ex[1]; ++b)
        for (unsigned c = 0; c <= ex[2]; ++c) {
          const unsigned e[3] = {a, b, c};
          if (a > 8 || b > 5 || c > 3) continue;
          const unsigned R = val(e);
          if (R < 2 || R > cap) continue;
          if (R > 256 && !(allow_big && mix3_lookup(R))) continue;
          std::vector<unsigned char> rad;
          stage_radices(a, b, c, rad);
          if (rad.size() > MIX_MAX_STAGE) continue;
          for (int j = 0; j < 3; ++j) { cur[depth][j] = e[j]; ex[j] -= e[j]; }
          go(depth + 1, R, cost + factor_cost(R));
          for (int j = 0; j < 3; ++j) ex[j] += e[j];
        }
  }
};

// true when N = 2^a 3^b 5^c (N >= 2) and a pass split with every factor <= 256 exists.  The split minimises the
// summed pass costs above; the factor with the most twos goes last, the others largest first.
inline bool fft_mixed_plan_search(size_t N, MixPlan *plan, bool allow_big) {
  if (N < 2 || N >= (size_t(1) << 31)) return false;
  PlanSearch ps;
  ps.allow_big = allow_big;
  if (!factor235(N, ps.ex)) return false;
  ps.go(0, allow_big ? 2000 : 256, 0.0);
  if (!ps.best_p) return false;
  const int p = ps.best_p;
  int last = 0;
  for (int i = 1; i < p; ++i) {
    const unsigned ti = std::min(ps.out[i][0], 4u), tl = std::min(ps.out[last][0], 4u);
    if (ti > tl || (ti == tl && PlanSearch::val(ps.out[i]) > PlanSearch::val(ps.out[last]))) last = i;
  }
  plan->p = p;
  int o = 0;
  for (int i = 0; i < p; ++i) {
    if (i == last) continue;
    plan->R[o] = PlanSearch::val(ps.out[i]);
    stage_radices(ps.out[i][0], ps.out[i][1], ps.out[i][2], plan->rad[o]);
    ++o;
  }
  plan->R[o] = PlanSearch::val(ps.out[last]);
  stage_radices(ps.out[last][0], ps.out[last][1], ps.out[last][2], plan->rad[o]);
  return true;
}
inline bool fft_mixed_plan(size_t N, MixPlan *plan, bool allow_big = true) {  // the search runs once per length
  static std::mutex mu;
  static std::unordered_map<size_t, std::pair<bool, MixPlan>> cache[2];
  std::lock_guard<std::mutex> g(mu);
  auto &c = cache[allow_big ? 1 : 0];
  auto it = c.find(N);
  if (it == c.end()) {
    if (c.size() > 4096) c.clear();
    MixPlan pl;
    const bool ok = fft_mixed_plan_search(N, &pl, allow_big);
    it = c.emplace(N, std::make_pair(ok, pl)).first;
  }
  if (it->second.first) *plan = it->second.second;
  return it->second.first;
}

// ---- options, steps, plans ----------------------------------------------------------------------------------------------------
inline unsigned opts_cus(const FftOpts &o) { return (unsigned)(o.cu_count > 0 ? o.cu_count : 256); }

// The three-step kernels (factors of 500 .. 2000) trade pass count for narrow tiles -- 8000 points are 1000 x 8 columns,
// i.e. 64-byte runs.  That wins while a pass is latency-bound and its data cache-resident (2e6 points, 16 MB: two passes of
// 16 us instead of three of 12), and loses once passes stream from HBM (2e7 points: 128-174 us per pass against 75-85 us
// for the two-step kernels' 256-byte runs).  So: only for transforms of at most 2^22 points in all.
inline bool fft_big_ok(const FftOpts &o, size_t total_points) { return o.big && !o.no_mix2 && total_points <= (size_t(1) << 22); }

// the factors of n's passes, first pass first (0: n is not a 2^a 3^b 5^c length); `factors` may be null
inline int fft_split(size_t n, bool allow_big, unsigned *factors = nullptr, int cap = 0) {
  if (n < 2) return is_pow2(n) ? 1 : 0;
  if (is_pow2(n)) {
    int bits[8];
    const int p = pow2_split(ilog2(n), bits);
    for (int i = 0; i < p && i < cap && factors; ++i) factors[i] = 1u << bits[i];
    return p;
  }
  MixPlan pl;
  if (!fft_mixed_plan(n, &pl, allow_big)) return 0;
  for (int i = 0; i < pl.p && i < cap && factors; ++i) factors[i] = pl.R[i];
  return pl.p;
}

enum FftKernel { FK_PASS = 0, FK_MIX, FK_MIX2, FK_MIX3, FK_MID, FK_MID3 };   // k_fft_pass | k_fft_mix | k_fft_mix2 | k_fft_mix3 | k_fft_mid | k_fft_mid3
enum FftBuf { FB_NONE = 0, FB_IN, FB_OUT, FB_WORK, FB_MID };                 // nothing | the caller's in / out | WS_FFT_B | the fused autocorrelation's Z
enum { FFT_MAX_STEPS = 2 * MIX_MAX_PASS };

struct FftStep {             // (filled by FftPlan::add: no initialisers, a plan's unused steps cost nothing)
  int kernel;                // FftKernel.  FK_PASS also needs ctx->tw_small, the kernel's last argument
  int inst;                  // FK_PASS: logR; FK_MIX2 / FK_MIX3 / FK_MID / FK_MID3: index into kMix2 / kMix3 / kMid
  int mode;                  // the kernel's MODE template argument (FFT_* / M3_*)
  const char *name;          // profile name
  unsigned grid, block;
  size_t lds;
  int src, dst;              // FftBuf
  unsigned twg_R, twg_Rn;    // != 0: needs the get_twg(R, Rn) table (MixDesc::twg)
  bool opt_in;               // the kernel has to be opted in to its dynamic LDS first
  union Params {
    PassDesc pass; MixDesc mix; MidDesc mid;
    Params() {}
  } p;
};

struct FftPlan {
  int status = TSDR_OK;
  char err[96];
  size_t copy_bytes = 0;    // a one-point transform: out = in, that many bytes (no step)
  size_t work_bytes = 0;    // WS_FFT_B, when a step names FB_WORK
  int nsteps = 0;
  FftStep step[FFT_MAX_STEPS];
  // A plan can hand every step on the moment it is complete instead of collecting them: the library launches it there
  // (fft_mixed.hip:launch_step), so that the later steps are planned while the first one runs, and one slot is all the memory the
  // steps touch -- with cold caches the descriptors of a whole plan cost 0.4-0.9 us ahead of the first launch (NOTEBOOK.md, "FFT
  // plans").  The sink's status ends the plan (err stays empty: the sink has reported).  Without a sink the plan is the value.
  int (*sink)(void *user, const FftPlan &pl, const FftStep &s) = nullptr;
  void *user = nullptr;
  FftPlan() { err[0] = 0; }
  FftPlan &fail(int st, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); std::vsnprintf(err, sizeof err, fmt, ap); va_end(ap);
    status = st; nsteps = 0;
    return *this;
  }
  FftStep &add(int kernel, int inst, int mode, const char *name, size_t grid, unsigned block, size_t lds, int src, int dst) {
    assert(sink || nsteps < FFT_MAX_STEPS);   // (the longest plan: five strided passes, the middle, five more of the inverse)
    FftStep &s = step[sink ? 0 : nsteps];
    ++nsteps;
    s.opt_in = false; s.twg_R = s.twg_Rn = 0;
    s.kernel = kernel; s.inst = inst; s.mode = mode; s.name = name; s.grid = (unsigned)grid; s.block = block; s.lds = lds; s.src = src; s.dst = dst;
    return s;
  }
  bool commit(const FftStep &s) {   // the step is complete; false: stop planning
    if (sink)
      if (int rc = sink(user, *this, s)) { status = rc; err[0] = 0; }
    return status == TSDR_OK;
  }
};

// ---- power-of-two lengths (fft.hip: k_fft_pass) -----------------------------------------------------------------------------------
inline void plan_pow2(const FftReq &q, FftPlan &pl) {
  const int logN = ilog2(q.n);
  if (logN < 0 || logN > 31) { pl.fail(TSDR_EINVAL, "fft: unsupported power-of-two length 2^%d", logN); return; }
  const size_t batch = q.batch;
  if (batch == 0) return;
  const size_t N = size_t(1) << logN;
  if (N * batch >= (size_t(1) << 40)) { pl.fail(TSDR_EINVAL, "fft: batch too large"); return; }
  if (logN == 0) { pl.copy_bytes = batch * sizeof(float2); return; }
  int bits[8];
  const int p = pow2_split(logN, bits);
  PassDesc d{};
  d.dir = q.dir < 0 ? -1 : 1;
  d.N = N;
  d.src_mode = SRC_C2C;
  d.src_n = 0;
  d.keep = q.keep ? q.keep : N;
  // (the integer IQ loaders are element-wise like SRC_C2C: any batch, as long as there is a strided pass to load through)
  if ((q.src_mode != SRC_C2C || q.epi) && ((batch != 1 && (q.epi || !src_is_cplx_int(q.src_mode))) || logN <= 8)) {
    pl.fail(TSDR_EINVAL, "fft: fused loader / epilogue needs one multi-pass transform");
    return;
  }
  d.src_aux = q.src_aux;
  d.src_w8 = src_is_int_iq(q.src_mode) ? (double)q.src_scale : 0.0;
  if (p == 1) {
    d.mode = FFT_ROWS;
    d.logR = logN;
    d.logT = 12 - logN;  // R*T = 4096
    d.scale = q.scale;
    d.rows = (unsigned)batch;
    if (batch >= (size_t(1) << 32)) { pl.fail(TSDR_EINVAL, "fft: too many rows"); return; }
    FftStep &s = pl.add(FK_PASS, d.logR, FFT_ROWS, "fft_rows", ceil_div(batch, (size_t)1 << d.logT), 256, kPassLds, FB_IN, FB_OUT);
    s.p.pass = d;
    pl.commit(s);
    return;
  }
  pl.work_bytes = N * batch * sizeof(float2);
  int logP = 0;  // log2(R_1..R_{i-1})
  for (int i = 0; i < p - 1; ++i) {
    const int logB = logN - logP - bits[i];
    d.mode = FFT_STRIDED;
    d.src_mode = i == 0 ? q.src_mode : SRC_C2C;
    d.src_n = q.src_n;
    d.logR = bits[i];
    d.logT = std::min(12 - bits[i], logB);
    d.scale = 1.0f;
    d.A = 1u << logP;
    d.B = 1u << logB;
    d.tiles = d.B >> d.logT;
    d.logNtw = logP + bits[i] + bits[i + 1];
    d.logBnext = logB - bits[i + 1];
    d.logPprev = logP;
    d.nprev = i;
    for (int j = 0; j < i; ++j) d.logRprev[j] = bits[j];
    const size_t grid = batch * d.A * d.tiles;
    if (grid >= (size_t(1) << 31)) { pl.fail(TSDR_EINVAL, "fft: grid too large"); return; }
    static const char *const kStridedName[3] = {"fft_strided1", "fft_strided2", "fft_strided3"};
    FftStep &s = pl.add(FK_PASS, d.logR, FFT_STRIDED, kStridedName[i], grid, 256, kPassLds, i == 0 ? FB_IN : FB_WORK, FB_WORK);
    s.p.pass = d;
    if (!pl.commit(s)) return;
    logP += bits[i];
  }
  d.mode = FFT_LAST;
  d.src_mode = SRC_C2C;
  if (q.epi) d.epi = *q.epi;
  d.logR = bits[p - 1];
  d.logR1 = bits[0];
  d.logT = std::min(12 - bits[p - 1], bits[0]);
  d.scale = q.scale;
  d.logPprev = logP;
  d.nprev = p - 1;
  for (int j = 0; j < p - 1; ++j) d.logRprev[j] = bits[j];
  d.Aprime = 1u << (logP - bits[0]);
  d.k1tiles = 1u << (bits[0] - d.logT);
  const size_t grid = batch * d.Aprime * d.k1tiles;
  if (grid >= (size_t(1) << 31)) { pl.fail(TSDR_EINVAL, "fft: grid too large"); return; }
  FftStep &s = pl.add(FK_PASS, d.logR, FFT_LAST, "fft_last", grid, 256, kPassLds, FB_WORK, FB_OUT);
  s.p.pass = d;
  pl.commit(s);
}

// ---- 2^a 3^b 5^c lengths (fft_mixed.hip) ----------------------------------------------------------------------------------------
// which kernel takes a factor: three register steps, two, or the generic LDS-stage kernel
struct MixPick { const Mix3Info *m3; const Mix2Info *m2; };
inline MixPick mix_pick(const FftOpts &o, unsigned R) {
  MixPick k;
  k.m3 = o.no_mix2 ? nullptr : mix3_lookup(R);
  k.m2 = (o.no_mix2 || k.m3) ? nullptr : mix2_lookup(R);
  return k;
}
// tile width of a pass over `span` columns (strided: B; last: R_1) with `other` tiles' worth of everything else
// (the two- and three-step kernels keep their full tile: a narrower one leaves most threads without a step-1 DFT)
inline int pass_logT(const MixPick &k, unsigned R, size_t other, size_t span) {
  if (k.m3) return k.m3->logT;
  return pick_logT(std::min({8, k.m2 ? floor_log2((unsigned)k.m2->tm) : floor_log2(4096u / R), ceil_log2((unsigned)span)}), k.m2 ? 8 : 4, other, span);
}
inline bool add_mix_pass(FftPlan &pl, const MixPick &k, const char *name, size_t grid, const MixDesc &d, int src, int dst, bool table = false) {
  FftStep *s;
  if (k.m3) {
    s = &pl.add(FK_MIX3, (int)(k.m3 - kMix3), d.mode, name, grid, (unsigned)k.m3->nt, k.m3->lds, src, dst);
    s->opt_in = true;
  } else if (k.m2) {
    s = &pl.add(FK_MIX2, (int)(k.m2 - kMix2), d.mode, name, grid, (unsigned)k.m2->nt, mix2_lds(d.R, k.m2->RA, d.logT, d.mode == FFT_STRIDED ? d.tw_sets : 1), src, dst);
  } else {
    s = &pl.add(FK_MIX, 0, d.mode, name, grid, 256, mix_lds(d.R, d.logT), src, dst);
  }
  if (table) { s->twg_R = d.R; s->twg_Rn = d.B; }   // the column table W_{R B}^(col k) of a strided two-step pass (MixDesc::twg)
  s->p.mix = d;
  return pl.commit(*s);
}
inline void set_radix(MixDesc &d, unsigned R, const std::vector<unsigned char> &rad) {
  d.R = R;
  d.nst = (int)rad.size();
  for (int s = 0; s < d.nst; ++s) d.rad[s] = rad[s];
  const Recip64 inv = recip64(R);
  d.r_hi = inv.hi;
  d.r_lo = inv.lo;
}

// The steps of passes first .. p-1 of `split` (without `last`: .. p-2, the strided ones only): the first of them reads `src`,
// the strided ones write `work`, the last pass writes `dst`.  A whole transform is (0, true, FB_IN, FB_WORK, FB_OUT).  The fused
// autocorrelation takes two slices, because its middle step stands for the forward split's last pass and the inverse split's
// first: (0, false) of the forward split into FB_WORK, and (1, true) of the inverse split in place in FB_MID (src == work), where
// the middle left pass 0's output.  These are the planner's own parameters; no caller of the engines sees them.
inline void plan_mixed_passes(FftPlan &pl, const FftReq &q, const FftOpts &o, const MixPlan &split, int first, bool last, int src, int work, int dst) {
  const size_t N = q.n, batch = q.batch;
  if (batch == 0) return;
  if (N * batch >= (size_t(1) << 40)) { pl.fail(TSDR_EINVAL, "fft: batch too large"); return; }
  const int p = split.p;
  // (the integer IQ loaders are element-wise like SRC_C2C: any batch)
  if (q.src_mode != SRC_C2C && ((batch != 1 && !src_is_cplx_int(q.src_mode)) || p == 1)) { pl.fail(TSDR_EINVAL, "fft: fused loader needs one multi-pass transform"); return; }
  MixDesc d{};
  d.dir = q.dir < 0 ? -1 : 1;
  d.N = N;
  d.src_mode = SRC_C2C;
  d.keep = q.keep ? q.keep : N;
  d.src_w8 = q.src_mode == SRC_POWER && !is_pow2(q.src_n) ? 4.0 / (double)q.src_n : src_is_int_iq(q.src_mode) ? (double)q.src_scale : 0.0;
  d.src_aux = q.src_aux;
  if (q.epi && (batch != 1 || p == 1)) { pl.fail(TSDR_EINVAL, "fft: epilogue needs one multi-pass transform"); return; }
  if (p == 1) {
    d.mode = FFT_ROWS;
    set_radix(d, split.R[0], split.rad[0]);
    d.logT = pick_logT(std::min(8, floor_log2(4096u / d.R)), 0, 1, batch);
    d.scale = q.scale;
    d.rows = (unsigned)batch;
    if (batch >= (size_t(1) << 32)) { pl.fail(TSDR_EINVAL, "fft: too many rows"); return; }
    FftStep &s = pl.add(FK_MIX, 0, FFT_ROWS, "fftm_rows", ceil_div(batch, (size_t)1 << d.logT), 256, mix_lds(d.R, d.logT), src, dst);
    s.p.mix = d;
    pl.commit(s);
    return;
  }
  if (work == FB_WORK) pl.work_bytes = N * batch * sizeof(float2);
  size_t P = 1;  // R_1..R_{i-1}
  size_t B = N;
  for (int i = 0; i < first && i < p - 1; ++i) { B /= split.R[i]; P *= split.R[i]; }
  static const char *const kStridedName[MIX_MAX_PASS] = {"fftm_strided1", "fftm_strided2", "fftm_strided3",
                                                         "fftm_strided4", "fftm_strided5", "fftm_strided6"};
  for (int i = first; i < p - 1; ++i) {
    set_radix(d, split.R[i], split.rad[i]);
    B /= d.R;
    d.mode = FFT_STRIDED;
    d.src_mode = i == 0 ? q.src_mode : SRC_C2C;
    d.src_n = q.src_n;
    const MixPick k = mix_pick(o, d.R);
    d.logT = pass_logT(k, d.R, batch * P, B);
    d.scale = 1.0f;
    d.A = (unsigned)P;
    d.B = (unsigned)B;
    d.tiles = (unsigned)ceil_div(B, (size_t)1 << d.logT);
    d.Bnext = (unsigned)(B / split.R[i + 1]);
    d.Pprev = (unsigned)P;
    const Recip64 ntw = recip64((unsigned long long)P * d.R * split.R[i + 1]);
    d.ntw_hi = ntw.hi;
    d.ntw_lo = ntw.lo;
    d.nprev = i;
    size_t wgt = 1;
    for (int j = 0; j < i; ++j) { d.Rprev[j] = split.R[j]; d.Wprev[j] = (unsigned)wgt; wgt *= split.R[j]; }
    const size_t grid = batch * d.A * d.tiles;
    if (grid >= (size_t(1) << 31)) { pl.fail(TSDR_EINVAL, "fft: grid too large"); return; }
    d.tw_sets = 0;
    bool table = false;
    if (k.m2) {
      // how the two-step kernel gets its inter-pass twiddles (see the kernel): sets in LDS, or the column table
      const unsigned T = 1u << d.logT;
      if (d.Bnext % T == 0) d.tw_sets = 1;
      else if (d.Bnext == 1) table = true;
      else if ((T - 1) / d.Bnext + 2 <= 4) d.tw_sets = (int)((T - 1) / d.Bnext + 2);
    }
    if (!add_mix_pass(pl, k, kStridedName[i], grid, d, i == first ? src : work, work, table)) return;
    P *= d.R;
  }
  if (!last) return;
  set_radix(d, split.R[p - 1], split.rad[p - 1]);
  d.mode = FFT_LAST;
  d.src_mode = SRC_C2C;
  if (q.epi) d.epi = *q.epi;
  d.R1 = split.R[0];
  const MixPick k = mix_pick(o, d.R);
  d.logT = pass_logT(k, d.R, batch * (P / split.R[0]), d.R1);
  d.scale = q.scale;
  d.Pprev = (unsigned)P;
  d.nprev = p - 1;
  {
    size_t wgt = 1;
    for (int j = 0; j < p - 1; ++j) { d.Rprev[j] = split.R[j]; d.Wprev[j] = (unsigned)wgt; wgt *= split.R[j]; }
  }
  d.Aprime = (unsigned)(P / split.R[0]);
  d.k1tiles = (unsigned)ceil_div((size_t)d.R1, (size_t)1 << d.logT);
  const size_t grid = batch * d.Aprime * d.k1tiles;
  if (grid >= (size_t(1) << 31)) { pl.fail(TSDR_EINVAL, "fft: grid too large"); return; }
  add_mix_pass(pl, k, "fftm_last", grid, d, first >= p - 1 ? src : work, dst);
}

// One 2^a 3^b 5^c transform request (in/out may alias; callers must not hand WS_FFT_B buffers in): the engine is chosen here.
inline void plan_fft(FftPlan &pl, const FftReq &q, const FftOpts &o) {
  if (is_pow2(q.n)) { plan_pow2(q, pl); return; }
  MixPlan split;
  if (!fft_mixed_plan(q.n, &split, fft_big_ok(o, q.n * q.batch))) { pl.fail(TSDR_EINVAL, "fft_mixed: length %zu is not 2^a*3^b*5^c", q.n); return; }
  plan_mixed_passes(pl, q, o, split, 0, true, FB_IN, FB_WORK, FB_OUT);
  return;
}

// The circular autocorrelation of 2 * q.n real samples (q.in: the samples behind the packing loader q.src_mode / q.src_n) as
//   forward passes 1..p-1  ->  [last forward pass + power spectrum + first inverse pass] (k_fft_mid)  ->  inverse passes 2..p
// with q's scale, keep and epilogue on the last one: forward strided steps into WS_FFT_B, the middle into FB_MID, the inverse's
// strided steps in place there, its last pass into q.out.  No steps: this length has no fused middle (the caller runs the two
// transforms separately).
inline void plan_autocorr(FftPlan &pl, const FftReq &q, const FftOpts &o) {
  const size_t Mc = q.n;
  MixPlan F;
  if (o.no_mix2 || !fft_mixed_plan(Mc, &F, fft_big_ok(o, Mc)) || F.p < 2 || Mc >= (size_t(1) << 31)) return;
  const int p = F.p;
  // the factor that goes LAST in the forward split (and first in the inverse one) must have the fused kernel: of those
  // that do, the one with the most twos (as the planner's own rule); the others keep their order
  {
    int pick = -1;
    for (int i = 0; i < p; ++i)
      if (mid_lookup(F.R[i]) && (pick < 0 || twos(F.R[i]) > twos(F.R[pick]) || (twos(F.R[i]) == twos(F.R[pick]) && F.R[i] > F.R[pick]))) pick = i;
    // (2e6 points: 1000 | 2000-mid | 1000 and 2000 | 1000-mid | 2000 measured the same, 74-75 us per search)
    if (pick < 0) return;
    if (pick != p - 1) {
      const unsigned r = F.R[pick];
      const std::vector<unsigned char> rd = F.rad[pick];
      for (int i = pick; i < p - 1; ++i) { F.R[i] = F.R[i + 1]; F.rad[i] = F.rad[i + 1]; }
      F.R[p - 1] = r;
      F.rad[p - 1] = rd;
    }
  }
  const MidInfo *me = mid_lookup(F.R[p - 1]);
  // inverse split: the forward's last factor first; of the others the one with the most twos last, the rest largest first
  MixPlan I;
  I.p = p;
  I.R[0] = F.R[p - 1];
  I.rad[0] = F.rad[p - 1];
  {
    int last = 0;
    for (int i = 0; i < p - 1; ++i)
      if (twos(F.R[i]) > twos(F.R[last]) || (twos(F.R[i]) == twos(F.R[last]) && F.R[i] > F.R[last])) last = i;
    std::vector<int> order;
    for (int i = 0; i < p - 1; ++i) if (i != last) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return F.R[a] > F.R[b]; });
    order.push_back(last);
    for (int k = 0; k < (int)order.size(); ++k) { I.R[k + 1] = F.R[order[k]]; I.rad[k + 1] = F.rad[order[k]]; }
  }
  MidDesc m{};
  m.R = F.R[p - 1];
  m.Bc = (unsigned)(Mc / m.R);
  m.ndir = m.Bc / 2 + 1;
  m.logT = floor_log2((unsigned)me->tm);
  if (m.logT < 1) return;
  m.nprev = p - 1;
  for (int j = 0; j < p - 1; ++j) m.Rprev[j] = F.R[j];
  const Recip64 inv = recip64(m.R), inv2 = recip64((unsigned long long)m.R * I.R[1]);
  m.r_hi = inv.hi;
  m.r_lo = inv.lo;
  m.ntw_hi = inv2.hi;
  m.ntw_lo = inv2.lo;
  m.Bnext = m.Bc / I.R[1];
  const unsigned Th = 1u << (m.logT - 1);
  const unsigned sets = (Th - 1) / m.Bnext + 2;
  m.tw_sets = sets <= 4 ? (int)sets : 0;
  m.w8 = 4.0 / (double)Mc;
  FftReq f;   // the forward transform, up to its last pass
  f.n = Mc; f.dir = -1; f.src_mode = q.src_mode; f.src_n = q.src_n; f.src_scale = q.src_scale;
  plan_mixed_passes(pl, f, o, F, 0, false, FB_IN, FB_WORK, FB_NONE);
  if (pl.status) return;
  const bool three = me->RA == 0;
  FftStep &s = pl.add(three ? FK_MID3 : FK_MID, (int)(me - kMid), 0, "fftm_mid", ceil_div((size_t)m.ndir, (size_t)Th), (unsigned)me->nt,
                      three ? me->lds3 : mid2_lds(m.R, me->RA, m.logT, m.tw_sets), FB_WORK, FB_MID);
  s.opt_in = three;
  s.p.mid = m;
  if (!pl.commit(s)) return;
  FftReq b;   // the inverse transform, from its second pass
  b.n = Mc; b.dir = +1; b.scale = q.scale; b.keep = q.keep; b.epi = q.epi;
  plan_mixed_passes(pl, b, o, I, 1, true, FB_MID, FB_MID, FB_OUT);
  return;
}

// ---- whole rows in one launch: getWelch's accumulator, tsdr_fft_c2c's batched rows, getWaterfall's writer ---------------------------
// `rows` rows of N points (N <= 4096) from samples of any kind, a row never leaving the chip between its steps.  No steps: not a
// length / count this launch serves (the caller takes the pass engines).
enum { ROWS_TO_WELCH = 0, ROWS_TO_STORE = 1, ROWS_TO_WATERFALL = 2 };
struct RowsReq {
  int what = ROWS_TO_STORE;
  int kind = SIG_CF32; float sig_scale = 1.0f;   // SigSrc::kind / scale of the rows
  size_t N = 0, rows = 0;
  int dir = -1; float scale = 1.0f;              // ROWS_TO_STORE; the other two are forward and unscaled
  float *acc = nullptr;                          // ROWS_TO_WELCH: partial power spectra, one per workgroup (room for 3 per CU)
  float2 *rows_out = nullptr;                    // ROWS_TO_STORE
  double *wf = nullptr;                          // ROWS_TO_WATERFALL
};
inline unsigned welch_parts(const FftOpts &o) { return opts_cus(o) * 3u; }
inline void plan_rows(FftPlan &pl, const RowsReq &q, const FftOpts &o) {
  const size_t N = q.N;
  const bool welch = q.what == ROWS_TO_WELCH, store = q.what == ROWS_TO_STORE;
  if (N > 4096 || q.rows >= (size_t(1) << 31)) return;
  if (store ? (N <= 256 || q.rows < 2) : (N < 2 || q.rows == 0)) return;
  if (!welch && o.no_mix2) return;
  MixDesc d{};
  d.dir = store ? (q.dir < 0 ? -1 : 1) : -1; d.N = N; d.src_mode = SRC_C2C; d.keep = N; d.scale = store ? q.scale : 1.0f;
  d.R = (unsigned)N;
  const Mix3Info *m3 = (welch && o.no_mix2) ? nullptr : welch3_lookup(d.R, welch);
  if (welch) {
    // the whole segment as ONE factor of the generic LDS-stage kernel where no three-step kernel has it (the pass planner caps
    // factors at 256 / 2000: its costs are those of HBM-sized passes)
    unsigned ex[3];
    if (!factor235(N, ex)) return;
    std::vector<unsigned char> rad;
    stage_radices(ex[0], ex[1], ex[2], rad);
    if (rad.size() > MIX_MAX_STAGE) return;
    set_radix(d, d.R, rad);
  } else {
    if (!m3) return;
    const Recip64 inv = recip64(d.R);
    d.r_hi = inv.hi;
    d.r_lo = inv.lo;
  }
  d.rows = (unsigned)q.rows;
  d.acc = q.acc; d.wf = q.wf; d.rows_out = q.rows_out;
  d.rows_real = rows_of(q.kind);
  if (q.kind >= SIG_SC16) d.src_w8 = (double)q.sig_scale;   // (ROWS_TO_STORE of integer IQ is forward only: no conjugation on the way in)
  const bool iq = d.rows_real > ROWS_REAL;
  if (m3) {
    // 500 / 1000 / 2000 (and 256 / 512 / 2048 / 4096 / 4000 ...): the three-register-step kernel, 8 (4, 2, 1) rows per workgroup
    d.logT = m3->logT;
    d.mode = FFT_LAST;
    const unsigned ntiles = (unsigned)ceil_div(q.rows, (size_t)1 << d.logT);
    // (getWelch: at most welch_parts() workgroups -- the caller's buffer holds that many partial spectra --, i.e. three per CU:
    // every partial is one more row for k_welch_sum to add, and the short lengths' small tiles would otherwise put eight
    // workgroups on a CU)
    size_t per_cu = (size_t)(160 * 1024) / m3->lds;
    if (q.what != ROWS_TO_WATERFALL) per_cu = std::min<size_t>(3, per_cu);
    per_cu = std::max<size_t>(1, per_cu);
    unsigned grid = std::min(ntiles, opts_cus(o) * (unsigned)per_cu);
    if (welch) grid = std::min(grid, welch_parts(o));
    const int mode = (welch ? M3_ACC : store ? M3_ROWS : M3_WF) + (iq ? M3_ACC_IQ - M3_ACC : 0);
    FftStep &s = pl.add(FK_MIX3, (int)(m3 - kMix3), mode, welch ? "welch_rows_acc3" : store ? "fft_rows3" : "waterfall_rows3", grid, (unsigned)m3->nt, m3->lds,
                        FB_IN, FB_NONE);
    s.opt_in = true;
    s.p.mix = d;
    pl.commit(s);
    return;
  }
  d.mode = FFT_ROWS;
  d.logT = floor_log2(4096u / d.R);
  const size_t lds = mix_lds(d.R, d.logT);
  const unsigned ntiles = (unsigned)ceil_div(q.rows, (size_t)1 << d.logT);
  const unsigned per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(3, (size_t)(150 * 1024) / lds));
  FftStep &s = pl.add(FK_MIX, 0, FFT_ROWS, "welch_rows_acc", std::min(ntiles, opts_cus(o) * per_cu), 256, lds, FB_IN, FB_NONE);
  s.opt_in = lds > 64 * 1024;   // (4096-point tiles + tables: above what a kernel gets without opting in)
  s.p.mix = d;
  pl.commit(s);
}

}  // namespace tsdr
