// raster_gram.hip -- the Gram matrix of a buffer's frames along a track (include/tempest_hip_gram.h): G[f][g] = sum_m v_f(m) conj(v_g(m)),
// v_f(m) = w_f(l) z_f(m) the probe's term (raster_ctrack.hip).  A GEMM X X^H with K = the pixels, on the f32-input matrix instruction
// (v_mfma_f32_32x32x2_f32: bit for bit an fmaf chain in k order, so a call repeats its bits).
//
//   gram_tile / gram_direct   k_gram<TP, NB>: the host side is a flavour's (fold_check, fold_launch: the refusals, the tiled / direct
//               choice, the tiles of 64 lines x TP = 128 or 16 pixels), the body is its own.  Four wavefronts.  The tile's weights
//               (F x 64 lines) and the frames' origins are evaluated once into LDS.  The tile is walked in PANELS of 128 pixels (one line
//               x 128, or 8 lines x 16): lane t samples (frame_pos, fold_s, fold_tap, ld_iq, coh_blend) and turns (coh_mul) pixel t & 127
//               of the panel for the frames of parity t >> 7 and stores Re and Im into X[row][pixel] -- rows 0 .. FP-1 the frames' real
//               parts, FP .. 2FP-1 their imaginary parts, FP = 32 NB >= F, the rows past F zero; pitch 130 floats: the operand reads
//               (row on the lane, 8 bytes) and the stores (pixel on the lane) are both free of bank conflicts.  Nothing is staged:
//               in the tiled kernel a wavefront's lanes are neighbours along a raster line and their loads coalesce.
//               After a barrier every wavefront runs its block products over the panel (GramJob): with 32-row blocks R_i, I_i,
//               Re G = R R^T + I I^T and M = I R^T, Im G = M - M^T; one triangle only, 3 products at NB = 1 and 10 at NB = 2, no
//               reduction across wavefronts.  The A operand of block a and the B operand of block b are both "row (lane & 31) of the block,
//               pixel pair by lane >> 5".  Every 8 panels (TSDR_GRAM_CHUNK pixels) the accumulators are widened to f64 partial sums
//               in registers; at the end they go to the workspace WS_GRAM, [tile][slot][16 registers][64 lanes], the slots in use only
//               (3 at NB = 1, 7 at NB = 2).
//   gram_sum    one lane per entry f >= g: the tiles' partial sums in tile order, both triangles written.
// No atomics.
#define TSDR_CTRACK_NO_ENTRY_POINTS
#include "raster_ctrack.hip"

namespace tsdr {
namespace {

constexpr int kGramPanel = 128;               // pixels of an LDS panel
constexpr int kGramPitch = kGramPanel + 2;    // floats between the rows of a panel (2 mod 64: see above)
constexpr int kGramWaves = 4, kGramThreads = kGramWaves * 64;
constexpr int kGramChunkPanels = TSDR_GRAM_CHUNK / kGramPanel;
constexpr int kGramSlot = 16 * 64;            // doubles of one accumulator's partial sums: [register][lane]
constexpr int gram_slots(int NB) { return NB == 1 ? 3 : 7; }   // accumulators of a tile that the sum reads
static_assert(TSDR_GRAM_CHUNK % kGramPanel == 0 && TSDR_GRAM_CHUNK <= 1024, "whole panels per chunk; the header's chain length");
static_assert(kGramThreads == 2 * kGramPanel, "a lane samples one pixel of the panel for the frames of one parity");
static_assert(TSDR_GRAM_MAX_FRAMES == 64, "two 32-row blocks per component");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct GramTrial {
  double T;
  const double *track;    // may be null: the zero track
};

constexpr size_t gram_lds(int NB, int F) { return (size_t)(64 * NB) * kGramPitch * 4 + (size_t)F * kFoldLines * 8; }
static_assert(gram_lds(2, TSDR_GRAM_MAX_FRAMES) + TSDR_GRAM_MAX_FRAMES * sizeof(FramePos) <= 160 * 1024, "the panel, the weights and the origins fit the CU's LDS");
static_assert(gram_lds(1, 32) <= 65536, "F <= 32 needs no opt-in");

// A wavefront's block products.  Blocks of 32 rows of X: NB = 1: R0, I0 = 0, 1;  NB = 2: R0, R1, I0, I1 = 0 .. 3.
//   accumulator 0 += X[a0] X[b0]^T (+ X[a1] X[b1]^T when a1 >= 0);  accumulator 1 += X[a2] X[b2]^T when a2 >= 0;  a0 < 0: nothing to do
// Workspace slots, packed (gram_first_slot: a wavefront's first; its second accumulator follows):
//   NB = 1:  Re_00 = slot 0 (R0 R0^T) + slot 1 (I0 I0^T),  M_00 = slot 2
//   NB = 2:  Re_00, M_00 = 0, 1;  Re_10, M_10 = 2, 3;  Re_11 = 4;  M_01, M_11 = 5, 6        (M_ij = I_i R_j^T)
struct GramJob {
  int a0, b0, a1, b1, a2, b2;
};
template <int NB>
__device__ inline GramJob gram_job(int wave) {
  if constexpr (NB == 1) {
    if (wave == 0) return GramJob{0, 0, -1, -1, -1, -1};
    if (wave == 1) return GramJob{1, 1, -1, -1, -1, -1};
    if (wave == 2) return GramJob{1, 0, -1, -1, -1, -1};
    return GramJob{-1, -1, -1, -1, -1, -1};
  } else {
    if (wave == 0) return GramJob{0, 0, 2, 2, 2, 0};
    if (wave == 1) return GramJob{1, 0, 3, 2, 3, 0};
    if (wave == 2) return GramJob{1, 1, 3, 3, -1, -1};
    return GramJob{2, 1, -1, -1, 3, 1};
  }
}
__device__ inline int gram_first_slot(int NB, int wave) { return NB == 1 ? wave : (wave < 3 ? 2 * wave : 5); }
// the slots the sum reads for the 32 x 32 block (bi, bj), bi >= bj, of Re and for M_ij
__host__ __device__ inline int gram_re_slot(int NB, int bi, int bj, int which) {
  if (NB == 1) return which == 0 ? 0 : 1;
  return which == 0 ? (bi == 0 ? 0 : (bj == 0 ? 2 : 4)) : -1;
}
__host__ __device__ inline int gram_m_slot(int NB, int bi, int bj) {
  if (NB == 1) return 2;
  return bi == 0 ? (bj == 0 ? 1 : 5) : (bj == 0 ? 3 : 6);
}

// one block product over a panel: acc += X[a] X[b]^T, pixels in the order 4t + 2h, then 4t + 2h + 1 (h = lane >> 5), t = 0 .. 31
__device__ inline void gram_panel_product(f32x16 &acc, const float *X, int a, int b, int lane) {
  const int r = lane & 31, h = lane >> 5;
  const float *xa = X + (a * 32 + r) * kGramPitch + 2 * h, *xb = X + (b * 32 + r) * kGramPitch + 2 * h;
#pragma unroll 4
  for (int t = 0; t < kGramPanel / 4; ++t) {
    const float2 va = *reinterpret_cast<const float2 *>(xa + 4 * t), vb = *reinterpret_cast<const float2 *>(xb + 4 * t);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va.x, vb.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va.y, vb.y, acc, 0, 0, 0);
  }
}

template <int TP, int NB>
__global__ __launch_bounds__(kGramThreads) void k_gram(FoldArgs<GramTrial> A) {
  constexpr int FP = 32 * NB, ROWS = 2 * FP;
  constexpr int LPP = kGramPanel / TP;            // raster lines of a panel
  static_assert(kGramPanel % TP == 0 && kFoldLines % LPP == 0, "whole lines per panel, whole panels per tile");
  extern __shared__ __align__(16) float gsm[];    // X[ROWS][kGramPitch], then the weights [F][64]
  __shared__ FramePos fps[TSDR_GRAM_MAX_FRAMES];  // the frames' origins
  float *X = gsm;
  float2 *wts = reinterpret_cast<float2 *>(gsm + ROWS * kGramPitch);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tp = (int)(blockIdx.x / (unsigned)A.tiles_l), tl = (int)(blockIdx.x - (unsigned)tp * (unsigned)A.tiles_l);
  const int l0 = tl * kFoldLines, p0 = tp * TP;
  const double T = A.tr.T;
  const unsigned P = (unsigned)A.y_t * (unsigned)A.x_t;
  const double spp = T / (double)P;

  for (int i = tid; i < A.F * kFoldLines; i += kGramThreads)
    wts[i] = track_weight(A.tr.track, i / kFoldLines, min(l0 + (i & (kFoldLines - 1)), A.y_t - 1), A.y_t);
  if (tid < A.F) fps[tid] = frame_pos(A, T, tid);
  for (int i = tid; i < ROWS * kGramPitch; i += kGramThreads) X[i] = 0.f;   // (the rows past F stay zero)
  __syncthreads();

  const GramJob job = gram_job<NB>(wave);
  f32x16 c0, c1;
  double s0[16], s1[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    c0[r] = c1[r] = 0.f;
    s0[r] = s1[r] = 0.0;
  }

  const int j = tid & (kGramPanel - 1), fs = tid >> 7;   // this lane's pixel of a panel, and the parity of its frames
  const int jl = j / TP, p = p0 + (j % TP);
  const int n_panels = (min(kFoldLines, A.y_t - l0) + LPP - 1) / LPP;
  for (int pn = 0; pn < n_panels; ++pn) {
    const int ll = pn * LPP + jl, l = l0 + ll;
    const bool on = l < A.y_t && p < A.x_t;
    const unsigned m = (unsigned)min(l, A.y_t - 1) * (unsigned)A.x_t + (unsigned)min(p, A.x_t - 1);
#pragma unroll 2
    for (int f = fs; f < A.F; f += kGramThreads / kGramPanel) {
      float2 v = make_float2(0.f, 0.f);
      if (on) {
        const FramePos fp = fps[f];
        double d;
        const int k = fold_tap(fp, fold_s(fp, spp, m), d);
        const unsigned ka = (unsigned)(fp.bi + (long long)k);
        const float2 a = ld_iq(A.iq, ka, A.fmt), b = ld_iq(A.iq, ka + 1u, A.fmt);
        v = coh_mul(coh_blend(a, b, d), wts[f * kFoldLines + ll]);
      }
      X[f * kGramPitch + j] = v.x;
      X[(FP + f) * kGramPitch + j] = v.y;
    }
    __syncthreads();   // the panel is complete
    if (job.a0 >= 0) {
      gram_panel_product(c0, X, job.a0, job.b0, lane);
      if (job.a1 >= 0) gram_panel_product(c0, X, job.a1, job.b1, lane);
      if (job.a2 >= 0) gram_panel_product(c1, X, job.a2, job.b2, lane);
      if ((pn + 1) % kGramChunkPanels == 0 || pn + 1 == n_panels) {   // the end of a chunk: widen, and start the next chains at zero
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s0[r] += (double)c0[r];
          s1[r] += (double)c1[r];
          c0[r] = c1[r] = 0.f;
        }
      }
    }
    __syncthreads();   // every wavefront has read the panel
  }

  if (job.a0 >= 0) {
    double *o = A.part + ((size_t)blockIdx.x * gram_slots(NB) + (size_t)gram_first_slot(NB, wave)) * kGramSlot + (size_t)lane;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r * 64] = s0[r];
    if (job.a2 >= 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) o[kGramSlot + r * 64] = s1[r];
    }
  }
}

// Entry (i, j) of a 32 x 32 accumulator sits in register (i & 3) + 4 (i >> 3) of lane j + 32 ((i >> 2) & 1).
__device__ inline unsigned gram_at(int i, int j) { return (unsigned)(((i & 3) + 4 * (i >> 3)) * 64 + j + 32 * ((i >> 2) & 1)); }

// one lane per entry f >= g: per tile Re = the partial sums of Re added, Im = M[f][g] - M[g][f]; the tiles in tile order; both triangles
__global__ __launch_bounds__(kFoldThreads) void k_gram_sum(const double *__restrict__ part, unsigned tiles, int F, int NB,
                                                           double *__restrict__ gram) {
  const int e = (int)(blockIdx.x * kFoldThreads + threadIdx.x);
  if (e >= F * F) return;
  const int f = e / F, g = e - f * F;
  if (g > f) return;
  const int bi = f >> 5, bj = g >> 5;
  const unsigned fg = gram_at(f & 31, g & 31), gf = gram_at(g & 31, f & 31);
  const int re1 = gram_re_slot(NB, bi, bj, 1);
  const double *q_re0 = part + (size_t)gram_re_slot(NB, bi, bj, 0) * kGramSlot + fg;
  const double *q_re1 = part + (size_t)(re1 < 0 ? 0 : re1) * kGramSlot + fg;
  const double *q_fg = part + (size_t)gram_m_slot(NB, bi, bj) * kGramSlot + fg;
  const double *q_gf = part + (size_t)gram_m_slot(NB, bj, bi) * kGramSlot + gf;
  const size_t kTile = (size_t)gram_slots(NB) * kGramSlot;
  double re = 0.0, im = 0.0;
  // two loops, not a condition per tile: a conditional load waits for itself, and the walk becomes one memory latency per tile
  if (re1 >= 0) {
#pragma unroll 8
    for (unsigned t = 0; t < tiles; ++t) {
      const size_t at = (size_t)t * kTile;
      re += q_re0[at] + q_re1[at];
      im += q_fg[at] - q_gf[at];
    }
  } else {
#pragma unroll 8
    for (unsigned t = 0; t < tiles; ++t) {
      const size_t at = (size_t)t * kTile;
      re += q_re0[at];
      im += q_fg[at] - q_gf[at];
    }
  }
  double *o = gram + 2 * ((size_t)f * (size_t)F + (size_t)g);
  o[0] = re;
  o[1] = f == g ? 0.0 : im;
  if (f != g) {
    double *c = gram + 2 * ((size_t)g * (size_t)F + (size_t)f);
    c[0] = re;
    c[1] = -im;
  }
}

// The host side of a flavour with kernels of its own, as the probe's.  FoldCall::state carries `gram`.
struct Gram {
  using Sample = float2;
  using Trial = GramTrial;
  static constexpr int NS = 0, kMaxTrials = 1, kStageMax = TSDR_CFOLD_STAGE_MAX, kSlot = WS_GRAM;
  static constexpr const char *name = "ctrack_gram";
  static int tile_p(bool) { return kFoldTileP; }
  static int batch(bool) { return 1; }
  static int refuse(tsdr_ctx *ctx, const char *fn, const FoldCall &c) {
    if (c.F > TSDR_GRAM_MAX_FRAMES)
      return set_err(ctx, TSDR_EINVAL, "%s: n_frames must be at most %d (got %d)", fn, TSDR_GRAM_MAX_FRAMES, c.F);
    if (int rc = refuse_period(ctx, fn, c)) return rc;
    // the tiles fold_launch will make: fewer than TSDR_GRAM_MAX_TILES, so that the f64 sums stay as shallow as the header's bound counts
    const size_t tiles = fold_tiles<Gram>(c, fold_staged<Gram>(c));
    if (tiles >= TSDR_GRAM_MAX_TILES)
      return set_err(ctx, TSDR_EINVAL, "%s: %d x %d makes %zu tiles, the limit is below %d", fn, c.y_t, c.x_t, tiles, TSDR_GRAM_MAX_TILES);
    return TSDR_OK;
  }
  static Trial trial(const FoldCall &c) { return Trial{c.T, c.track}; }
  static int launch(tsdr_ctx *ctx, const FoldCall &c, const FoldGeom &g, const FoldArgs<Trial> &A0) {
    FoldArgs<Trial> A = A0;
    const int NB = c.F > 32 ? 2 : 1;
    A.part = (double *)ctx->scratch(WS_GRAM, g.tiles * (size_t)gram_slots(NB) * kGramSlot * 8);
    if (!A.part) return TSDR_ENOMEM;
    const size_t lds = gram_lds(NB, c.F);
    void (*const kfn)(FoldArgs<Trial>) = g.staged ? (NB == 1 ? k_gram<kFoldTileP, 1> : k_gram<kFoldTileP, 2>)
                                                  : (NB == 1 ? k_gram<kFoldDirectP, 1> : k_gram<kFoldDirectP, 2>);
    if (lds > 64 * 1024)   // above what a kernel gets without opting in
      if (int rc = lds_opt_in(ctx, (const void *)kfn, gram_lds(2, TSDR_GRAM_MAX_FRAMES))) return rc;
    const dim3 grid((unsigned)g.tiles), wg(kGramThreads);
    if (g.staged) TSDR_LAUNCH(ctx, "gram_tile", kfn, grid, wg, lds, A);
    else TSDR_LAUNCH(ctx, "gram_direct", kfn, grid, wg, lds, A);
    TSDR_LAUNCH(ctx, "gram_sum", k_gram_sum, dim3((unsigned)ceil_div((size_t)c.F * (size_t)c.F, kFoldThreads)), dim3(kFoldThreads), 0,
                (const double *)A.part, (unsigned)g.tiles, c.F, NB, reinterpret_cast<double *>(c.state));
    return TSDR_OK;
  }
};

// an entry point: the refusals, then the device form, or the host form around it (upload iq and the track, launch, download gram, wait)
int gram_entry(tsdr_ctx *ctx, const char *fn, const char *what, FoldCall c, double *gram, bool device) {
  if (!ctx) return TSDR_EINVAL;
  if (!gram) return set_err(ctx, TSDR_EINVAL, "%s: gram is NULL", fn);
  c.state = reinterpret_cast<float *>(gram);
  IqFmt f;
  if (int rc = fold_check<Gram>(ctx, fn, c, device, f)) return rc;
  if (device) {
    TSDR_PTR_ALIGNED(ctx, fn, gram, 8);
    TSDR_PTR_ALIGNED(ctx, fn, c.track, 8);
  } else if (int rc = refuse_track_values(ctx, fn, c)) {
    return rc;
  }
  if (c.F == 0) return TSDR_OK;
  if (device) return fold_launch<Gram>(ctx, c, f);
  HostStage st(ctx);
  c.iq = st.in(WS_IN, c.iq, c.n * iq_bytes(f));
  c.state = (float *)st.out(WS_OUT, gram, 16 * (size_t)c.F * (size_t)c.F);
  c.track = (const double *)st.in(WS_AUX, c.track, 16 * (size_t)c.F);   // absent or present
  return st.run(what, [&] { return fold_launch<Gram>(ctx, c, f); });
}

}  // namespace
}  // namespace tsdr

using namespace tsdr;

extern "C" {

int tsdr_ctrack_gram_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                          int n_frames, int y_t, int x_t, double *gram) {
  return gram_entry(ctx, "ctrack_gram_iq", __func__, track_call(iq, iq_fmt, scale, n, t0, T, track, n_frames, y_t, x_t), gram, true);
}

int tsdr_ctrack_gram_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                        int n_frames, int y_t, int x_t, double *gram) {
  return gram_entry(ctx, "ctrack_gram_iq", __func__, track_call(iq, iq_fmt, scale, n, t0, T, track, n_frames, y_t, x_t), gram, false);
}

}  // extern "C"
