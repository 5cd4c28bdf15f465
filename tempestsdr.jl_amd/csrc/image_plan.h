// image_plan.h -- what the first launch(es) of a buffer will be, decided once, as a value.
//
// plan_images() turns a request (geometry, input format, precision, raster / images / projection sums wanted) and the options
// the decision reads into an ImagePlan: at most three steps, each naming a kernel family, its template arguments, profile
// name, grid, block, dynamic LDS bytes and the filled parameter struct.  It makes no HIP call and touches no context, so a
// host-only program can print it (tools/host_plan); resample.hip:launch_images walks it and is the only code that launches
// these kernels.  Pointers enter at the launch and nowhere earlier: a parameter struct's pointer fields stay null here.
//
// The routes, in the order they are tried (FAST = TSDR_FAST with IQ input):
//   1  FAST, no raster wanted     k_down_fused (the tap kernel: four taps of every output pixel from staged samples), when its
//                                 tiling fits and the sampling ratio is within "down_spp_max_pct"
//   2  FAST, raster, "raster_split"   k_raster_shear (raster only, stores on the 128-byte grid) + k_down_fused  (A/B)
//   3  raster wanted, or FAST     the tile walk: k_raster_fast / k_raster_fast4 (FAST), k_raster_tile (EXACT), with the image
//                                 and its projection sums from the same launch where the tiling allows; k_raster_direct for
//                                 ratios nothing can stage
//   4  images still missing       k_down_fused in the request's precision; failing that, per frame: raster into WS_RASTER,
//                                 then k_resize2d (`fallback`: the plan's last two steps run once per frame)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "down_fused.h"
#include "sync_layout.h"

namespace tsdr {

// ---- FAST coordinate: exact rational, incremental ---------------------------------------------------------
struct FastAx {
  unsigned S, P, D;       // D = 2P
  unsigned qstep, rstep;  // 2S = qstep*D + rstep : advance of (k, r) per output sample
  double invDd;           // 1/D
};

static inline FastAx fast_axis(size_t S, size_t P) {
  FastAx f;
  f.S = (unsigned)S; f.P = (unsigned)P; f.D = (unsigned)(2 * P);
  f.qstep = (unsigned)((2 * S) / (2 * P));
  f.rstep = (unsigned)((2 * S) % (2 * P));
  f.invDd = 1.0 / (double)(2 * P);
  return f;
}

// parameters of the tile kernels (k_raster_tile, k_raster_fast, k_raster_fast4; k_raster_direct reads S, y_t, x_t, iqf)
struct TileParams {
  unsigned S;
  int y_t, x_t;
  int TP, W;            // pixels per tile, LDS row capacity (samples)
  int tiles_l, tiles_p; // tiles per frame
  int frames;
  int own_l, own_p;     // owned lines / pixels per tile (64/TP, or 63/TP-1 with DOWN)
  int h_out, w_out;     // DOWN only
  int NR, NC;           // DOWN: candidate output rows / columns per tile
  int lpl_log;          // log2(lanes per line) of the staging loop
  int cs;               // k_raster_fast: consecutive samples per staging lane (<= 4)
  int xcd_group;        // neighbouring pixel strips dealt to the same XCD
  int xcd_group_log;    // log2(xcd_group)
  float inv_tiles_p;    // 1/tiles_p (unit -> frame, strip without an integer division)
  RsAxis ax, ay, axx;   // sig->raster, raster lines->rows, raster pixels->columns (host-computed)
  double inv_sfy, inv_sfx;
  float *proj;          // k_raster_fast<DOWN>: projection partial sums of the (h_out, w_out) images, or null
  size_t proj_stride;   // floats per frame: colpart[tiles_l][w_out] | rowpart[tiles_p][h_out]
  unsigned long long *keys;  // with proj: two vsync argmax keys per frame, cleared here for k_beta's atomicMax
  IqFmt iqf;            // CPLX input: ComplexF32 or int16 pairs (common.h)
};

struct FastInc {
  unsigned qL, rL;    // advance of (k, r) per raster line       : 2*x_t*S       = qL*D + rL
  unsigned qTL, rTL;  // per tile row (own_l lines)
  unsigned qTP, rTP;  // per tile column (own_p pixels)
  int k00;            // position of pixel 0 of a frame: floor((S - P)/D) ...
  unsigned r00;       // ... and remainder
  float invD;
};

static inline FastInc fast_inc(size_t S, size_t P, int x_t, int own_l, int own_p) {
  FastInc n;
  const long long D = 2 * (long long)P;
  auto split = [&](long long delta, unsigned &q, unsigned &r) { q = (unsigned)(delta / D); r = (unsigned)(delta % D); };
  split(2LL * x_t * (long long)S, n.qL, n.rL);
  split(2LL * x_t * (long long)S * own_l, n.qTL, n.rTL);
  split(2LL * (long long)S * own_p, n.qTP, n.rTP);
  const long long num = (long long)S - (long long)P;
  long long q = num / D;
  if (num % D < 0) --q;
  n.k00 = (int)q;
  n.r00 = (unsigned)(num - q * D);
  n.invD = 1.0f / (float)D;
  return n;
}

// parameters of k_raster_shear (raster_shear.hip)
struct ShearParams {
  unsigned S;
  int y_t, x_t, frames;
  int W, rows;            // staged samples per row, staged rows (64 + 31 with SHEAR)
  int tiles_p, tiles_l;
  int c;                  // y_t mod 32
  unsigned out_mis;       // (out address / 4) mod 32
  double sf;
  long long XA, XB;       // 32.32 increments per column: sf (1 + delta x_t) for delta = -c and 32 - c
  float inv_W;
};

constexpr int kShearTP = 128;   // pixel columns per workgroup: 4 wavefronts x 32
// (256 threads per 64 x 64-pixel tile of k_down_fused: 512 threads measured 55.9 us, 512 threads on 64 x 128 58.5 us, 128 threads 70.4 us, against 54.3 us)
constexpr int kDownNT = 256;

// ---- the request and the plan ---------------------------------------------------------------------------------
struct PlanOpts {   // the options the decision reads (tsdr_ctx::opt_*), by value
  int raster_rec4 = -1, raster_v4 = 0, raster_split = 0, fast_walk_only = 0, down_spp_max_pct = 200, down_xcd = 1, cu_count = 0;
};
static inline PlanOpts plan_opts(const tsdr_ctx *c) {
  return PlanOpts{c->opt_raster_rec4, c->opt_raster_v4, c->opt_raster_split, c->opt_fast_walk_only, c->opt_down_spp_max_pct, c->opt_down_xcd,
                  c->cu_count};
}

struct ImageReq {
  int cplx = 1;                   // IQ input (format iqf) or real samples
  IqFmt iqf;
  int precision = TSDR_FAST;
  size_t S = 0, in_stride = 0;    // samples per frame, samples from one frame to the next
  int y_t = 0, x_t = 0, h_out = 0, w_out = 0, frames = 0;
  bool raster = false;            // the (y_t, x_t) rasters are wanted
  bool images = false;            // the (h_out, w_out) images are wanted
  bool sums = false;              // ... and their projection partial sums, where the image kernel can form them
  uintptr_t raster_addr = 0;      // route 2 only: the raster pointer's address (its low 7 bits decide the shear) and stride
  size_t raster_stride = 0;
};

enum { IK_NONE = 0, IK_FAST, IK_FAST4, IK_TILE, IK_DIRECT, IK_DOWN, IK_SHEAR, IK_RESIZE2D };

struct ImageStep {
  int kernel = IK_NONE;
  const char *name = "";          // profile name
  unsigned grid[3] = {1, 1, 1}, block = 0;
  size_t lds = 0;                 // dynamic LDS bytes
  // template arguments: k_raster_fast<cplx, f32w, down, pw, out, vw, rec4, iqf>, k_raster_fast4<iqf, pw>, k_raster_tile<cplx, down>,
  // k_raster_direct<cplx>, k_down_fused<cplx, mode, sums, ld, iqf>, k_raster_shear<shear>
  int cplx = 0, f32w = 0, down = 0, pw = 0, out = 0, vw = 0, rec4 = 0, iqf = IQF_RT;
  int mode = DM_EXACT, sums = 0, ld = 4, shear = 0;
  bool to_images = false;         // the raster IS the image (sizes equal): it is written to the image buffer
  // the kernel's parameters: q (+ fa, fi) for the tile kernels, dq (+ lds_main) for k_down_fused, sq for k_raster_shear;
  // rs = {h_in, w_in, h_out, w_out} for k_resize2d
  TileParams q{};
  FastAx fa{};
  FastInc fi{};
  DownParams dq{};
  size_t lds_main = 0;
  ShearParams sq{};
  int rs[4] = {0, 0, 0, 0};
};

struct ImagePlan {
  int status = TSDR_OK;
  const char *err = "";           // message for set_err when status != TSDR_OK
  int nsteps = 0;
  ImageStep step[3];
  bool fallback = false;          // the last two steps (raster of ONE frame into WS_RASTER, k_resize2d) run once per frame
  size_t ws_raster = 0;           // ... and need this many bytes of WS_RASTER
  size_t in_stride = 0;
  int frames = 0;
  bool raster = false, images = false;   // what the steps produce
  ProjLayout sums{};              // projection partial sums formed by the image step (ncp == 0: none)
};

static inline int plan_fail(ImagePlan &pl, const char *msg) {
  pl.status = TSDR_EINVAL; pl.err = msg; pl.nsteps = 0; pl.fallback = false; pl.ws_raster = 0;
  pl.raster = pl.images = false; pl.sums = ProjLayout{};
  return TSDR_EINVAL;
}

static inline const char *geom_error(size_t S, int y_t, int x_t) {
  if (y_t <= 0 || x_t <= 0) return "y_t and x_t must be positive";
  const size_t P = (size_t)y_t * (size_t)x_t;
  if (S >= (size_t(1) << 31) || P >= (size_t(1) << 31)) return "frame larger than 2^31 samples/pixels";
  if (S != P && S < 2) return "imresize needs at least 2 input samples";
  return nullptr;
}

// Staging lanes per line: log2 of the power of two (4 .. 64) that wastes the fewest load slots of a W-sample line, ties to the
// larger.  A lane issues `unit` loads per trip, lpl samples apart, so a line costs ceil(W / (unit lpl)) * unit lpl slots;
// max_trips > 0 bounds the trips (k_raster_fast: one sample per trip, four trips at most).
static inline int stage_lanes(int W, long unit, long max_trips) {
  int best = -1; long best_slots = 1L << 60;
  for (int lg = 2; lg <= 6; ++lg) {
    const long chunk = unit << lg, trips = (long)ceil_div((size_t)W, (size_t)chunk);
    if (max_trips > 0 && trips > max_trips) continue;
    const long slots = trips * chunk;
    if (slots < best_slots || (slots == best_slots && lg > best)) { best = lg; best_slots = slots; }
  }
  return best;
}

// XCD-aware grid of the tile kernels: (8 XCD slots, line tiles, (frame, strip) units per slot).  false: too many tiles.
static inline bool xcd_grid(const TileParams &q, unsigned (&grid)[3]) {
  const size_t units = (size_t)q.frames * q.tiles_p;
  const size_t G = (size_t)q.xcd_group;
  const size_t upx = ceil_div(units, 8 * G) * G;  // units per XCD slot
  if (upx > 65535 || (size_t)q.tiles_l > 65535 || units >= (size_t(1) << 20)) return false;
  grid[0] = 8; grid[1] = (unsigned)q.tiles_l; grid[2] = (unsigned)upx;
  return true;
}
constexpr const char *kTooManyTiles = "raster: too many tiles for one launch (split the buffer)";

// ---- the tap kernel's tiling (k_down_fused, and through guard_image_plan the sync guard's exact tiles) ----------------------
struct DownPlan { bool fused; int mode; DownParams q; size_t lds; };

static inline DownPlan plan_down_tiles(size_t S, int y_t, int x_t, int h_out, int w_out, bool exact, bool wide_exact = false, bool guard_tiles = false) {
  DownPlan pl;
  pl.fused = false;
  pl.lds = 0;
  pl.mode = DM_EXACT;
  const double sf = (double)S / ((double)y_t * (double)x_t);
  const double sfy = (double)y_t / (double)h_out, sfx = (double)x_t / (double)w_out;
  const long NLd = (long)(63.0 * sfy) + 3;
  // FAST: above a vertical ratio of ~2 the lines between an output row's two tap lines are more than half of the tile's
  // span: stage just the 2 x 64 tap lines (C5: 128 instead of 239)
  const bool sparse = !exact && NLd > 128;
  const long NL = sparse ? 128 : NLd;
  // 64-column tiles (4096 pixels per 256-thread workgroup) with f32 staging: measured at C2 against the former preference
  // (32 columns at most, {a, slope} f64 pairs when they fit 32 KiB -- which held the tile to 16 columns): 50 vs 65 us for the
  // FAST kernel; 128 columns: 58 us.  The EXACT tiling is the sync guard's as well and stays as it was.
  static const int cand_fast[] = {64, 32, 16, 8, 4}, cand_exact[] = {32, 16, 8, 4, 0};
  const int *cand = (exact && !wide_exact) ? cand_exact : cand_fast;   // wide_exact: the EXACT frame path (not the sync guard's tiles)
  for (int pass = 1; pass < 3 && !pl.fused; ++pass) {
    const int sb = 4;
    // (the sync guard's kernel runs one workgroup per CU and opts in to a large LDS: the widest tile that fits 96 KiB -- at C3
    // 32 columns instead of 16, i.e. one round of image tiles per flagged frame instead of two)
    const size_t cap = guard_tiles ? 96 * 1024 : pass == 2 ? 60 * 1024 : 32 * 1024;
    for (int ci = 0; ci < 5 && cand[ci] > 0; ++ci) {
      const int TC = cand[ci];
      const long DPX = (long)((double)(TC - 1) * sfx) + 2;
      const long W = (long)((double)DPX * sf) + 4 + (exact ? 0 : (sf <= 0.5 ? 2 : 1));
      const size_t lds = (((size_t)NL * (size_t)(W | 1) * sb + 15) & ~(size_t)15) + (size_t)TC * 20 + (size_t)NL * 4;
      if (lds <= cap && W < (1 << 20)) {
        pl.fused = true;
        pl.lds = lds;
        // FAST: fixed-point taps where a raster pixel spans at most half a sample (the second tap of a line then lies in the
        // first one's three-sample window); one more staged sample for that window
        pl.mode = exact ? DM_EXACT : (sf <= 0.5 ? DM_FAST_FX : DM_FAST_F32);
        pl.q.S = (unsigned)S; pl.q.y_t = y_t; pl.q.x_t = x_t; pl.q.h_out = h_out; pl.q.w_out = w_out;
        pl.q.sparse = sparse ? 1 : 0;
        pl.q.TC = TC; pl.q.NL = (int)NL; pl.q.W = (int)W; pl.q.tiles_c = (int)ceil_div((size_t)w_out, (size_t)TC);
        // staging lanes per line: a lane issues its loads four at a time (round 4: the former rule counted ceil(W / lpl) * lpl
        // and, for W = 29, chose 32 lanes per line: three of every four loads were clamped duplicates);
        // wide rows (many samples per raster pixel): 16 loads in flight per lane, 8 lanes per line
        const long LD = (!exact && W >= 48) ? 16 : 4;
        pl.q.ld16 = LD == 16 ? 1 : 0;
        pl.q.lpl_log = stage_lanes((int)W, LD, 0);
        break;
      }
    }
  }
  return pl;
}

// ---- route 3: the tile walk ----------------------------------------------------------------------------------
// The instantiations of k_raster_fast<true, f32w, down, pw, out, vw, rec4, iqf> that plan_raster can name, for any request it
// accepts -- stated once: plan_raster refuses a step outside it, resample.hip:launch_fast builds exactly these kernels and
// refuses every other value, plan_dump --table prints them.  Each rule follows from a condition of plan_raster's FAST branch
// (quoted; NOTEBOOK.md, "kernel instantiations", says how to extend the set when a planner change needs a new kernel):
constexpr bool fast_instance(bool f32w, bool down, int pw, bool out, int vw, bool rec4, int iqf) {
  (void)f32w;   // either position advance at any tile: `w32 = 2 * P < 2^24 && q.tiles_l <= 128 && q.tiles_p <= 128`
  const bool pw_any = pw == 1 || pw == 2 || pw == 4 || pw == 8 || pw == 16 || pw == 32;   // `s.pw = max(q.TP / 4, 1)`, TP = 4 .. 128
  // `dn = want_down && q.TP >= 32 && ...`: the in-walk downgrade runs on tiles of 32 pixels and more
  if (down && pw < 8) return false;
  // `if (!dn && !out) return TSDR_OK`: a step that neither downgrades nor writes the raster is never made
  if (!down && !out) return false;
  // `want_down = ... && y_t >= 2 * 64 && ...` and `VW = v4 ? 1 : y_t >= 2 * 64 ? 2 : 1` (v4 is IK_FAST4's): the downgrade
  // runs two wavefronts high; a raster shorter than 128 lines gets one, and no downgrade
  if (down ? vw != 2 : (vw != 1 && vw != 2)) return false;
  // `s.rec4 = rec4 && dn`, and the format is a template argument exactly then: `if (s.rec4) s.iqf = ...`, else IQF_RT
  if (rec4 && !down) return false;
  const bool iqf_ok = rec4 ? (iqf == IQF_CF32 || iqf == IQF_SC16 || iqf == IQF_SC8 || iqf == IQF_UC8) : iqf == IQF_RT;
  return pw_any && iqf_ok;
}
constexpr const char *kNoFastInstance = "raster: the tile plan names a kernel that is not built";

// sig_to_image for `frames` consecutive frames (`out`: the raster is written) and, with `down`, the (h_out, w_out) image of each
// frame from the same launch where the tiling allows: did_down says so.  Appends at most one step.
static inline int plan_raster(const PlanOpts &o, const ImageReq &r, int frames, bool out, bool down, int h_out, int w_out, bool sums,
                              ImagePlan &pl, bool &did_down) {
  did_down = false;
  if (frames <= 0) return TSDR_OK;
  const size_t S = r.S;
  const int y_t = r.y_t, x_t = r.x_t, cplx = r.cplx;
  const size_t P = (size_t)y_t * x_t;
  const double sf = (double)S / (double)P;
  // TSDR_FAST exists for the steady-state frame loop (tsdr_frames*), whose input is IQ; the per-function entry
  // points (real input) always run the oracle's operation sequence
  const bool exact = r.precision == TSDR_EXACT || !cplx || P >= (size_t(1) << 30);
  // fused downgrade in the raster launch: only when both axes shrink (<= 66 x 130 candidates per tile)
  const bool want_down = down && !(y_t == h_out && x_t == w_out) && y_t >= 2 * 64 && x_t >= 2 * 128 &&
                         (double)y_t / h_out >= 1.0 && (double)x_t / w_out >= 1.0;
  ImageStep &s = pl.step[pl.nsteps];
  s = ImageStep{};
  TileParams &q = s.q;
  q.S = (unsigned)S; q.y_t = y_t; q.x_t = x_t; q.frames = frames;
  if (cplx) q.iqf = r.iqf;
  s.cplx = cplx ? 1 : 0;
  s.out = out ? 1 : 0;
  // pairs of strips.  Measured on C2 -- round 2 (16-byte sample records, 3 workgroups per CU): G=1 0.138 ms, G=4 0.132 ms, G=41 0.146 ms;
  // round 4 (f32 samples, 4 per CU), the launch alone on two boxes: G=1 115.3, G=2 110.9 / 114.9, G=4 113.7 / 117.4, G=8 118.4, G=16 120.5 us
  // (C3: no difference; C5: G=2 1 % behind G=4).  The EXACT tile kernel (two workgroups per CU fewer) keeps four: 146.5 against 148.3 us
  q.xcd_group_log = exact ? 2 : 1;
  q.xcd_group = 1 << q.xcd_group_log;
  q.ax = rs_axis(S, (size_t)y_t * x_t);
  if (h_out > 0 && w_out > 0) {
    q.ay = rs_axis((size_t)y_t, (size_t)h_out); q.axx = rs_axis((size_t)x_t, (size_t)w_out);
    q.inv_sfy = 1.0 / q.ay.sf; q.inv_sfx = 1.0 / q.axx.sf;
  }
  bool tiled = false;
  // EXACT with the downgrade fused in: 64-pixel tiles, because the raster tile kept in LDS then costs 16.6 KiB
  // instead of 33 KiB, which doubles the resident workgroups per CU.  FAST keeps no raster tile (k_raster_fast).
  int tp_max = (want_down && exact) ? 64 : 128;
  // staged-sample budget per tile: EXACT 4 B/sample (<= 48 KiB), FAST 16 B/sample (<= 47 samples per line = 47 KiB;
  // only down-sampling ratios get near it, up-sampling tiles stage ~11-18 samples per line)
  // (FAST with plain f32 samples -- REC4, k_raster_fast: the f32 walk with the in-walk downgrade -- 4 B/sample: <= 94 samples
  // per line, i.e. C3's 1.15 samples per raster pixel get 64-pixel tiles, and with them the in-walk projection sums)
  const bool rec4_ok = !exact && want_down && o.raster_rec4 != 0 && 2 * P < (size_t(1) << 32) && y_t > h_out && x_t > w_out;
  auto pick_tp = [&](long w_cap) {
    tiled = false;
    for (int TP = tp_max; TP >= 4; TP >>= 1) {
      const long W = (long)((double)(TP - 1) * sf) + 4;
      if (W <= w_cap) { tiled = true; q.TP = TP; q.W = (int)W; break; }
    }
  };
  pick_tp(exact ? 191 : rec4_ok ? 94 : 47);
  if (rec4_ok && tiled && q.W > 47) {
    // the wider budget only holds for the plan REC4 serves: the in-walk downgrade (TP >= 32)
    if (q.TP < 32) pick_tp(47);
  }
  if (tiled && !exact) {  // FAST: k_raster_fast
    // the in-walk downgrade needs ratios strictly above 1 (a line / pixel is then the top-left tap of at most one
    // output row / column); otherwise the raster is produced here and the caller downgrades separately
    const bool dn = want_down && q.TP >= 32 && y_t > h_out && x_t > w_out;
    // wavefronts stacked vertically per workgroup (see k_raster_fast).  Measured on C2: 1 -> 0.121 ms, 2 -> 0.118 ms,
    // 4 (1024 threads, 77 KiB LDS) -> 0.131 ms; again with f32 samples (REC4, 12 KiB): 130 / 124 / 138 us for the launch
    // round 6: four lines per lane (k_raster_fast4) wherever the f32-sample walk with the in-walk image writes rasters from
    // 128-pixel tiles -- C2's route: a quarter fewer write requests for the same bytes (option "raster_v4", default off)
    const bool v4 = o.raster_v4 > 0 && rec4_ok && dn && q.TP == 128 && out && 2 * P < (size_t(1) << 24) && y_t >= 512 &&
                    x_t <= 127 * 128 && o.raster_split == 0 &&
                    (q.iqf.kind == IQK_CF32 || q.iqf.kind == IQK_SC16);   // (k_raster_fast4 exists for those two formats only)
    const int VW = v4 ? 1 : y_t >= 2 * 64 ? 2 : 1;
    const int lstep = dn ? 63 : 64, NL = v4 ? 256 : lstep * (VW - 1) + 64;
    q.own_l = v4 ? 255 : lstep * VW;
    q.own_p = dn ? q.TP - 1 : q.TP;
    q.tiles_l = dn ? (y_t - 2) / q.own_l + 1 : (int)ceil_div((size_t)y_t, (size_t)q.own_l);
    q.tiles_p = dn ? (x_t - 2) / q.own_p + 1 : (int)ceil_div((size_t)x_t, (size_t)q.TP);
    q.inv_tiles_p = 1.0f / (float)q.tiles_p;
    if (!dn && !out) return TSDR_OK;  // nothing to do here; the caller falls back to k_down_fused
    // f32 walk and 32-bit position advance: D = 2P < 2^24 and few enough tiles that the advances stay below 2^32
    const bool w32 = 2 * P < (size_t(1) << 24) && q.tiles_l <= 128 && q.tiles_p <= 128;
    // Staged samples as plain f32 (REC4, k_raster_fast) instead of 16-byte records wherever the f32 walk with the in-walk
    // downgrade runs: C3's tiles (39 samples x 127 lines) were 79 KB of records, ONE 512-thread workgroup per CU with nothing
    // to cover its staging (357 -> 244 us per buffer with 20 KB of samples); C2's 42 KB -> 14 KB is worth 4-6 % of its
    // store-bound launch.  One more sample per line: a pixel reads (k, k + 1).
    const bool rec4 = rec4_ok && dn;
    if (!rec4 && q.W > 47) return plan_fail(pl, "raster: tile plan needs the f32-sample walk");  // (pick_tp above rules it out)
    if (rec4) q.W += 1;
    // staging lanes per line: the power of two that wastes the fewest lane slots with <= 4 samples per lane
    q.lpl_log = stage_lanes(q.W, 1, 4);
    q.cs = (int)ceil_div((size_t)q.W, (size_t)1 << q.lpl_log);
    size_t lds = rec4 ? (((size_t)NL * (size_t)(q.W | 1) * 4 + 15) & ~(size_t)15) + 16 : (size_t)NL * (size_t)(q.W | 1) * 16 + 16;
    const int v4pw = o.raster_v4 == 32 ? 32 : 16;
    if (v4) lds += (size_t)(128 / v4pw) * NL * 4;   // the wavefronts' image-row scratch (down_event4)
    // the images' projection partial sums come out of the same walk when the caller has room for them
    // (with narrower tiles -- down-sampling ratios such as C3's -- the per-workgroup part of the sums is spread over
    // four times as many workgroups and costs more than the separate pass over the images: 0.382 vs 0.354 ms)
    const bool pj = dn && q.TP >= 64 && sums;
    if (dn) {
      q.h_out = h_out; q.w_out = w_out;
      lds += (size_t)(NL + q.TP + 1) * 12 + 16;
      if (pj) {
        lds = std::max(lds, (size_t)2 * 256 * VW * 4);  // the sums reuse the sample region after the walk
        pl.sums.ncp = q.tiles_l;
        pl.sums.nrp = q.tiles_p;
        s.sums = 1;
        q.proj_stride = proj_floats(h_out, w_out, pl.sums);
      }
    }
    s.fa = fast_axis(S, P);
    s.fi = fast_inc(S, P, x_t, q.own_l, q.own_p);
    if (!xcd_grid(q, s.grid)) return plan_fail(pl, kTooManyTiles);
    s.lds = lds;
    s.down = dn ? 1 : 0;
    if (v4) {
      s.kernel = IK_FAST4; s.name = "raster_down_iq";
      s.pw = v4pw; s.block = 64 * (128 / v4pw);
      s.iqf = q.iqf.sc16() ? IQF_SC16 : IQF_CF32;
    } else {
      s.kernel = IK_FAST; s.name = !out ? "down_walk_iq" : dn ? "raster_down_iq" : "raster_iq";
      s.f32w = w32 ? 1 : 0; s.pw = std::max(q.TP / 4, 1); s.vw = VW; s.block = 256 * VW;
      // the f32-sample instantiations (the hot ones) exist once per input format, the others read it from the parameters
      s.rec4 = (rec4 && dn) ? 1 : 0;
      if (s.rec4) s.iqf = q.iqf.kind == IQK_SC16 ? IQF_SC16 : q.iqf.kind == IQK_SC8 ? IQF_SC8 : q.iqf.kind == IQK_UC8 ? IQF_UC8 : IQF_CF32;
      if (!fast_instance(s.f32w, s.down, s.pw, s.out, s.vw, s.rec4, s.iqf)) return plan_fail(pl, kNoFastInstance);  // (no input gets here)
    }
    ++pl.nsteps;
    did_down = dn;
    return TSDR_OK;
  }
  if (tiled) {  // EXACT: k_raster_tile
    const bool dn = want_down && q.TP >= 32;
    q.own_l = dn ? 63 : 64;
    q.own_p = dn ? q.TP - 1 : q.TP;
    q.tiles_l = dn ? (y_t - 2) / 63 + 1 : (int)ceil_div((size_t)y_t, 64);
    q.tiles_p = dn ? (x_t - 2) / q.own_p + 1 : (int)ceil_div((size_t)x_t, (size_t)q.TP);
    q.inv_tiles_p = 1.0f / (float)q.tiles_p;
    // staging lanes per line: a lane issues its loads four at a time, lpl samples apart (see plan_down_tiles)
    q.lpl_log = stage_lanes(q.W, 4, 0);
    size_t lds = (size_t)64 * (size_t)(q.W | 1) * 4 + 16 + 64 * 4 + 16;
    if (dn) {
      q.h_out = h_out; q.w_out = w_out;
      q.NR = (int)ceil(64.0 / ((double)y_t / h_out)) + 5;
      q.NC = (int)ceil((double)q.TP / ((double)x_t / w_out)) + 5;
      if (q.NR > 128 || q.NC > 192) return plan_fail(pl, "raster: candidate table overflow");
      lds += (size_t)q.TP * 65 * 4 + (size_t)(q.NR + q.NC + 4) * 4 + (size_t)(q.NR + q.NC) * 8;
    }
    if (!dn && !out) return TSDR_OK;  // nothing to do here; the caller falls back to k_down_fused
    if (!xcd_grid(q, s.grid)) return plan_fail(pl, kTooManyTiles);
    s.kernel = IK_TILE; s.block = 256; s.lds = lds; s.down = dn ? 1 : 0;
    s.name = dn ? (cplx ? "raster_down_iq_exact" : "raster_down_f32_exact") : (cplx ? "raster_iq_exact" : "raster_f32_exact");
    ++pl.nsteps;
    did_down = dn;
    return TSDR_OK;
  }
  if (!out) return TSDR_OK;
  // no tile fits: the direct kernel (no LDS, EXACT arithmetic); it reads S, y_t, x_t and the format, nothing else
  q = TileParams{};
  q.S = (unsigned)S; q.y_t = y_t; q.x_t = x_t;
  if (cplx) q.iqf = r.iqf;
  s.kernel = IK_DIRECT; s.block = 256; s.name = cplx ? "raster_direct_iq" : "raster_direct_f32";
  s.grid[0] = (unsigned)stream_blocks(o.cu_count, ceil_div((size_t)y_t, 64) * 64 * (size_t)x_t); s.grid[1] = (unsigned)frames;
  ++pl.nsteps;
  return TSDR_OK;
}

// ---- route 2's raster: k_raster_shear -----------------------------------------------------------------------
static inline void plan_shear(const ImageReq &r, bool shear, ImagePlan &pl, bool &did) {
  did = false;
  const int y_t = r.y_t, x_t = r.x_t, frames = r.frames;
  const double sf = (double)r.S / ((double)y_t * (double)x_t);
  if (sf > 0.5 || y_t < 64 || x_t < kShearTP || frames <= 0 || frames > 65535) return;
  if ((r.raster_addr & 3u) != 0) return;
  ImageStep &s = pl.step[pl.nsteps];
  s = ImageStep{};
  ShearParams &q = s.sq;
  q.S = (unsigned)r.S; q.y_t = y_t; q.x_t = x_t; q.frames = frames; q.sf = sf;
  q.c = y_t & 31;
  if (q.c == 0 && (r.raster_stride & 31) == 0 && (r.raster_addr & 127u) == 0) shear = false;   // already on the grid
  q.rows = shear ? 95 : 64;
  q.W = (int)((double)(kShearTP - 1) * sf) + 5;
  q.inv_W = 1.0f / (float)q.W;
  q.tiles_p = (int)ceil_div((size_t)x_t, (size_t)kShearTP);
  q.tiles_l = (int)ceil_div((size_t)y_t + (shear ? 31 : 0), 64);
  q.out_mis = (unsigned)((r.raster_addr >> 2) & 31u);
  const double xt = (double)x_t;
  q.XA = (long long)floor(sf * (1.0 - (shear ? (double)q.c * xt : 0.0)) * 4294967296.0);
  q.XB = (long long)floor(sf * (1.0 + (double)(32 - q.c) * xt) * 4294967296.0);
  const size_t lds = ((size_t)q.rows * (size_t)(q.W | 1) + (size_t)q.rows) * 4;
  if (lds > 60 * 1024 || q.tiles_l > 65535) return;
  s.kernel = IK_SHEAR; s.shear = shear ? 1 : 0; s.out = 1; s.cplx = 1; s.iqf = IQF_CF32;
  s.name = shear ? "raster_sheared_iq" : "raster_unsheared_iq";
  s.grid[0] = (unsigned)q.tiles_p; s.grid[1] = (unsigned)q.tiles_l; s.grid[2] = (unsigned)frames;
  s.block = 256; s.lds = lds;
  ++pl.nsteps;
  did = true;
}

// ---- route 4 (and the image half of routes 1, 2): sig_to_image |> downgradeImage straight from the signal -----------------
// dp: the tap kernel's tiling for this request (plan_down_tiles(..., exact, /*wide_exact=*/true)), evaluated once by plan_images
static inline int plan_down_frames(const PlanOpts &o, const ImageReq &r, const DownPlan &dp, bool sums, ImagePlan &pl) {
  const int y_t = r.y_t, x_t = r.x_t, h_out = r.h_out, w_out = r.w_out, frames = r.frames, cplx = r.cplx;
  const bool same2 = (y_t == h_out && x_t == w_out);
  if (!same2 && (y_t < 2 || x_t < 2)) return plan_fail(pl, "imresize needs at least a 2x2 raster");
  if (frames <= 0) return TSDR_OK;
  bool did = false;
  if (same2) {  // imresize returns a copy when the sizes already match: the raster IS the result
    const int n0 = pl.nsteps;
    const int rc = plan_raster(o, r, frames, true, false, 0, 0, false, pl, did);
    if (!rc && pl.nsteps > n0) pl.step[n0].to_images = true;
    return rc;
  }
  const bool exact = r.precision == TSDR_EXACT || !cplx;
  if (dp.fused) {
    ImageStep &s = pl.step[pl.nsteps];
    s = ImageStep{};
    s.kernel = IK_DOWN; s.block = kDownNT; s.cplx = cplx ? 1 : 0; s.mode = dp.mode; s.ld = dp.q.ld16 ? 16 : 4;
    s.dq = dp.q;
    if (cplx) s.dq.iqf = r.iqf;
    const bool psum = !exact && sums;
    s.grid[0] = (unsigned)(ceil_div((size_t)h_out, 64) * (size_t)s.dq.tiles_c); s.grid[1] = (unsigned)frames;
    if (o.down_xcd && !exact) {
      s.dq.xcd_tiles = (int)s.grid[0];
      s.dq.xcd_tpx = (int)ceil_div((size_t)s.grid[0], 8);
      s.grid[0] = (unsigned)(8 * s.dq.xcd_tpx * frames); s.grid[1] = 1;
    }
    s.lds_main = (dp.lds + 15) & ~(size_t)15;
    s.lds = dp.lds;
    // (the FAST kernels exist once per input format, the EXACT one reads it from the parameters)
    s.iqf = dp.mode == DM_EXACT ? IQF_RT
          : s.dq.iqf.kind == IQK_SC16 ? IQF_SC16 : s.dq.iqf.kind == IQK_SC8 ? IQF_SC8 : s.dq.iqf.kind == IQK_UC8 ? IQF_UC8 : IQF_CF32;
    if (!cplx) s.name = "down_fused_f32_exact";
    else if (dp.mode == DM_EXACT) s.name = "down_fused_iq_exact";
    else if (psum) {
      s.name = "down_fused_iq_sums";
      s.sums = DS_PSUM;
      s.lds = s.lds_main + (kDownNT + (size_t)s.dq.TC) * 4;
      pl.sums.ncp = (int)ceil_div((size_t)h_out, 64);
      pl.sums.nrp = s.dq.tiles_c;
      s.dq.proj_stride = proj_floats(h_out, w_out, pl.sums);
    } else s.name = "down_fused_iq";
    ++pl.nsteps;
    return TSDR_OK;
  }
  // fallback: materialise each raster in workspace, then the generic 2-D resize
  // (one raster per pipeline lane: two submissions of tsdr_frames_submit_d may be walking this loop side by side)
  const size_t P = (size_t)y_t * x_t;
  int rc = plan_raster(o, r, 1, true, false, 0, 0, false, pl, did);
  if (rc) return rc;
  ImageStep &s = pl.step[pl.nsteps];
  s = ImageStep{};
  s.kernel = IK_RESIZE2D; s.name = "resize2d"; s.block = 256;
  s.grid[0] = (unsigned)stream_blocks(o.cu_count, (size_t)h_out * w_out);
  s.rs[0] = y_t; s.rs[1] = x_t; s.rs[2] = h_out; s.rs[3] = w_out;
  ++pl.nsteps;
  pl.fallback = true;
  pl.ws_raster = 4 * P * 4;
  return TSDR_OK;
}

// raster (optional) + (h_out, w_out) image for every frame with as few passes over IQ as possible; or the rasters alone
static inline ImagePlan plan_images(const PlanOpts &o, const ImageReq &r) {
  ImagePlan pl{};
  pl.in_stride = r.in_stride;
  pl.frames = r.frames;
  if (const char *e = geom_error(r.S, r.y_t, r.x_t)) { plan_fail(pl, e); return pl; }
  bool did = false;
  if (!r.images) {  // sig_to_image alone
    if (r.raster && !plan_raster(o, r, r.frames, true, false, 0, 0, false, pl, did)) pl.raster = pl.nsteps > 0;
    return pl;
  }
  // (no entry point asks for an empty image; checked here, before any ratio is formed from the sizes)
  if (r.h_out <= 0 || r.w_out <= 0) { plan_fail(pl, "output size must be positive"); return pl; }
  const int y_t = r.y_t, x_t = r.x_t, h_out = r.h_out, w_out = r.w_out;
  const bool fast = r.precision == TSDR_FAST && r.cplx;
  const bool same2 = y_t == h_out && x_t == w_out;
  const DownPlan dp = plan_down_tiles(r.S, y_t, x_t, h_out, w_out, !fast, true);
  const double spp = (double)r.S / ((double)y_t * (double)x_t);   // samples per raster pixel
  auto finish = [&](int rc) {
    if (!rc) { pl.images = r.frames > 0; for (int i = 0; i < pl.nsteps; ++i) pl.raster |= pl.step[i].out && !pl.step[i].to_images && !(pl.fallback && i >= pl.nsteps - 2); }
    return pl;
  };
  // 1  FAST without a raster to write: k_down_fused re-derives the four taps of every output pixel from 64 x 64-pixel tiles of
  // staged samples and leaves the projection partial sums itself (round 3: 54 us at C2 against the walk's 77 us with
  // out == null -- the walk evaluates all 2.9 M raster pixels of a frame for the 1.8 M that are taps) ...
  // ... where a tile of at least 32 columns fits (C2: 0.115 samples per raster pixel, 64 columns, 0.102 vs 0.123 ms per buffer
  // in round 3; C5: 0.084, 0.138 vs 0.279 ms), or, above 0.5 samples per raster pixel, one of 16 (C3: 1.15 samples per pixel --
  // the walk won there, 0.420 vs 0.461 ms, while the tap kernel staged its 121-sample rows four loads at a time: a chain of
  // dependent round trips, 28 us per tile.  With 16 loads in flight per lane: 186 us against the walk's 323 + k_proj's 24,
  // 0.243 vs 0.403 ms per buffer).  Option "down_spp_max_pct" (default 200) bounds the ratio; the walk keeps the rest.
  if (!r.raster && fast && !o.fast_walk_only && dp.fused && dp.q.TC >= (spp > 0.5 ? 16 : 32) && spp <= (double)o.down_spp_max_pct * 0.01 &&
      !same2 && y_t >= 2 && x_t >= 2)
    return finish(plan_down_frames(o, r, dp, r.sums, pl));
  // 2  FAST with a raster (option "raster_split"; A/B of round 4): the rasters by the store-aligned ("sheared") raster-only
  // kernel of raster_shear.hip, the images + projection sums by the raster-free kernel -- two launches, IQ read twice,
  // instead of the one walk that produces raster, image and sums with misaligned column stores
  if (r.raster && fast && o.raster_split && r.iqf.kind == IQK_CF32 &&   // (the A/B kernel reads ComplexF32 only)
      dp.fused && dp.q.TC >= 32 && spp <= 0.5 && !same2 && y_t >= 64 && x_t >= 128) {
    plan_shear(r, o.raster_split == 1, pl, did);
    if (did) return finish(plan_down_frames(o, r, dp, r.sums, pl));
  }
  // 3  the tile walk: raster, and where the tiling allows the image and its sums, from one launch
  if (r.raster || fast) {
    if (plan_raster(o, r, r.frames, r.raster, true, h_out, w_out, r.sums, pl, did)) return pl;
    if (did) return finish(TSDR_OK);
  }
  // 4  the images are still missing
  return finish(plan_down_frames(o, r, dp, false, pl));
}

}  // namespace tsdr
