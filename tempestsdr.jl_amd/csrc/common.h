// common.h -- context, workspace and launch helpers shared by every translation unit
// of libtempest_hip.so.  gfx950 only; no CPU fallback anywhere in this library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tempest_hip.h"
#include "loop_policy.h"

namespace tsdr {

// workspace slots: one growable device buffer each, owned by the context
enum Slot {
  WS_IN = 0,      // host-API staging of inputs
  WS_OUT,         // host-API staging of outputs
  WS_AUX,         // host-API staging (second output / state)
  WS_ABS,         // |IQ| or power scratch
  WS_RASTER,      // fallback raster when the fused path cannot tile
  WS_IMG,         // per-frame 600x800 images of one buffer
  WS_PROJ,        // raw + filtered projections, sums
  WS_KEYS,        // packed argmax keys per frame
  WS_FFT_A,       // FFT ping
  WS_FFT_B,       // FFT pong
  WS_FFT_C,       // Bluestein / correlation scratch
  WS_FFT_D,
  WS_MISC,
  WS_GUARD,       // sync guard: flags + per-workgroup top-2 column maxima (guard.h)
  WS_F64_A,       // Float64 per-function entry points (*_f64): transform / staging buffers of their own, so that an f64
  WS_F64_B,       // call never moves a workspace the f32 paths hold
  WS_F64_C,
  WS_IQX,         // integer IQ expanded to ComplexF32 for the transform routes without a loader hook (tsdr_*_iq_d)
  WS_DISPLAY,     // display.hip: per group the finite minimum / maximum / count, the range, and the 4096 histogram counters
  WS_FOLD,        // raster_fold.hip: per (trial, tile) the f64 partial sums of a period scan's pictures
  WS_CFOLD,       // raster_cfold.hip: per (trial, tile) the f64 partial energies of a carrier scan's complex pictures
  WS_CSTACK,      // raster_cstack.hip: per tile the four f64 partial sums of a call, its rotation q, and (LOCK) the complex picture Z
  WS_CTRACK,      // raster_ctrack.hip: per (frame, tile) the f64 partial sums of a phase probe (Re rho_f, Im rho_f, E_f, the tile's E_s)
  WS_GRAM,        // raster_gram.hip: per (tile, accumulator in use) the f64 partial sums of a frame Gram matrix's 32 x 32 blocks
  WS_HIRES,       // tsdr_frames_hires_iq_d: the rasters of one chunk of frames (raster_accum.hip)
  WS_HIRES_IDX,   // ... and the buffer's sync indices when the caller passes none
  WS_HIRES_SHIFTS,  // ... and the raster-unit shifts its frames were averaged with (tsdr_frames_hires_shifts)
  WS_REG_PART,    // raster_register.hip: per-tile partial sums of the profiles (f64), column partials then row partials
  WS_REG_PROF,    // ... the profiles of a registration's frames and of its reference (f64)
  WS_REG_SCORES,  // ... its scores when the caller asks for none
  WS_COUNT
};

struct ProfRec {
  const char *name;
  hipEvent_t e0, e1;
};

// How the frame kernels' loaders read one IQ sample: interleaved ComplexF32 (the reference's recv! buffers), or interleaved
// int16 pairs as SDR hardware delivers them, turned into ComplexF32(re, im) * scale in the loader itself (tsdr_frames_sc16*:
// int16 slots are never expanded in HBM -- half the IQ bytes the image kernel reads), or 8-bit pairs (tsdr_frames_iq_d):
// int8 (sc8), or uint8 around the fixed offset 127.5 (uc8: the subtraction is exact in f32, so the product by scale is
// the only rounding of either format) -- a quarter of the bytes.  kind = TSDR_IQ_* of tempest_hip.h.
enum { IQK_CF32 = 0, IQK_SC16 = 1, IQK_SC8 = 2, IQK_UC8 = 3 };
struct IqFmt {
  int kind = IQK_CF32; float scale = 1.0f;
  __host__ __device__ bool sc16() const { return kind == IQK_SC16; }
};

struct TwTable {   // two-level table of W_N^e = exp(-2*pi*i*e/N), N = 2^logN
  int logN = 0, h = 0;
  float2 *lo = nullptr;  // W_N^j, j < 2^h
  float2 *hi = nullptr;  // W_N^(j*2^h), j < 2^(logN-h)
};

struct BluesteinPlan {
  size_t n = 0, L = 0;
  float2 *chirp = nullptr;  // exp(-i*pi*k^2/n), k < n
  float2 *bfft = nullptr;   // FFT_L of the wrapped conj chirp
};

// The frame loop pipelined across buffers (tsdr_frames_submit_d, frames.hip): successive buffers on internal HIP streams so that
// the latency-bound tail of one (vsync statistics, sync guard, shift + IIR) runs beside the image launch of the next.  WHICH
// streams, and in which arrangement, is the tuner's business (loop_policy.h); this is what of the pipeline needs HIP.
struct Pipeline {
  hipStream_t pool[kPoolN + kPoolH] = {};  // created at the first submission (frames.hip:pipe_init)
  hipStream_t lane[4] = {};         // the streams of the arrangement in use (members of pool): [0], [1], [3] equal lanes / [0] image lane, [2] tail lane
  hipEvent_t ev_img[kPipeSlots] = {}, ev_tail[kPipeSlots] = {};  // recorded behind a slot's image launch / its shift + IIR
  bool ev_tail_used[kPipeSlots] = {};
  hipEvent_t lane_in = nullptr;     // "inputs ready" point of the context's stream
  hipEvent_t tune_ev[kTrial] = {};  // timing events of a trial (two are recorded: PipeTuner::submitted)
  unsigned long long n = 0;         // submissions since the last flush point
  unsigned long long seq = 0;       // submissions since the lanes were last run empty (slot = seq % kPipeSlots)
  PipeKey key;                      // what the slot offsets of the submissions in flight were computed from
  int last_slot = -1;               // slot of the latest submission: its tail is behind everything submitted
  int cand_now = -1;                // arrangement (index into kCands) of the submissions in flight
  int cand_submit = -1;             // ... of the latest tsdr_frames_submit_* call: what tsdr_frames_pipeline_info reports when nothing is measured
  bool from_run = false;            // the lanes carry tsdr_frames_d / _sc16_d / _iq_d calls (frames.hip:frames_run), not submissions: the
                                    // caller was promised no flush point, so whatever the context's stream receives next drains first (run_fence)
  bool one_lane = false;            // ... is the one-stream arrangement (no event per buffer; pipe_drain records one when asked)
  LaneBusy busy;                    // which pool streams may still hold work (loop_policy.h): pipe_sync_lanes waits for these only
  PipeTuner tuner;
  void release() {                  // tsdr_destroy, with every lane idle
    for (auto &l : pool) if (l) (void)hipStreamDestroy(l);
    for (auto &e : tune_ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : ev_img) if (e) (void)hipEventDestroy(e);
    for (auto &e : ev_tail) if (e) (void)hipEventDestroy(e);
    if (lane_in) (void)hipEventDestroy(lane_in);
  }
};

}  // namespace tsdr

struct tsdr_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  hipStream_t launch_stream = nullptr;  // stream TSDR_LAUNCH targets (== stream)
  std::string err;
  int cu_count = 0;
  int precision = TSDR_FAST;  // tsdr_precision: written by tsdr_set_precision only (a buffer that has to run in TSDR_EXACT
                              // carries that in its frames.hip:FrameJob, as it carries its IQ format)
  // development switches (tsdr_set_option; environment variables of the same upper-case names are read ONCE, in tsdr_create)
  int opt_ac_mixed = 1;     // autocorrelation of n = 2*(2^a3^b5^c) samples: native mixed-radix route (0: zero-padded power of two)
  int opt_fft_no_mix2 = 0;  // 1: every mixed-radix factor through the generic LDS-stage kernel
  int opt_fft_big = 1;      // mixed-radix planner may use factors of 500 / 1000 / 2000 (three-register-step kernels)
  int opt_vsync_blank_dark = 0;  // 1: the blanking interval is the DARKEST band: findmin instead of findmax on both axes (FrameSynchronisation.jl:51-53)
  int opt_vsync_current_sy = 0;  // 1: vsync / the frame loop return s_y of the CURRENT image (the corrected ordering, off by default)
  int opt_hires_chunk_frames = 0; // tsdr_frames_hires_iq_d: frames per chunk (0: the whole buffer in one chunk, the measured optimum)
  int opt_hires_refine = 0;       // tsdr_frames_hires_iq_d: 0..8, the registration's search radius in cells of the 600x800 sync grid (0: off;
                                  // include/tempest_hip_register.h)
  int hires_shifts_n = 0;         // frames of the most recent tsdr_frames_hires_iq_d whose applied shifts WS_HIRES_SHIFTS holds
  int opt_display_hist_agg = 0;   // tsdr_display_u8*: 1 = a wave whose lanes all hold one histogram bin adds their number once (display.hip; A/B)
  int opt_fast_walk_only = 0;   // 1: the raster-free FAST frame path runs the raster walk with out == null (round 2's route; A/B)
  int opt_down_spp_max_pct = 200; // raster-free FAST route: k_down_fused up to this many samples per raster pixel (percent), the raster walk above
                                  // (round 4: 50 -> 200 once wide rows stage with 16 loads in flight: C3 0.40 -> 0.24 ms per buffer)
  int opt_down_xcd = 1;      // raster-free FAST kernel: XCD-aware tile order
  int opt_raster_rec4 = -1;  // FAST raster walk: staged |IQ| as plain f32 samples (4 bytes) instead of {a, slope hi, slope lo} records (16): 0 = never (the A/B), else wherever the f32 walk forms the images
  int opt_raster_v4 = 0;     // FAST frame loop with rasters at C2-like geometry: four lines per lane (k_raster_fast4: dwordx4 raster stores, compacted image
                             // rows) -- 32: four wavefronts of 32 pixel columns per tile, other > 0: eight of 16.  Round 6's A/B: loses by 12-20 %, off
  int opt_raster_split = 0;  // FAST frame loop with rasters: 1 = sheared raster-only kernel + raster-free image kernel, 2 = the same unsheared (A/B)
  int opt_ac_fuse_mid = 1;  // autocorrelation: last forward pass + power spectrum + first inverse pass as one launch
  // sync guard of the FAST frame loop (guard.h): relative top-2 margin below which a frame is re-evaluated exactly
  // (0: off); running totals {frames checked, frames re-evaluated} on the device
  float guard_thr = 2e-5f;
  unsigned *guard_sync[4] = {};             // work-queue words of the guard kernel (zero between launches), one set per pipeline lane
  unsigned long long *guard_stats = nullptr;
  // adaptive route (option "sync_guard_auto", loop_policy.h:GuardRoute).  Decided on the host, DETERMINISTICALLY (round 5):
  // every guarded call's guard launch writes ITS OWN {frames, flagged} into a pinned ring entry tagged with the call's
  // sequence number; the decision for call k folds the entries of calls <= k - kGuardLag, in submission order, waiting for
  // them if need be (call k - 3 is long complete in any steady state: it is the pipeline's own slot-reuse distance).  The same
  // sequence of buffers therefore takes the same route on every run, whatever the host / GPU timing.
  int opt_guard_auto = 1;
  tsdr::GuardRoute guard;
  int opt_guard_nowait = 0;                  // measurement switch (TSDR_GUARD_NOWAIT): the decision never waits for an entry
  static constexpr int kGuardRing = 16, kGuardLag = 3;
  unsigned long long *guard_ring = nullptr;  // pinned: GuardRoute::decode
  unsigned long long guard_seq = 0;          // guarded calls issued so far (the next one's sequence number)
  unsigned long long guard_consumed = 0;     // entries folded into the window so far
  int guard_last_dark = 0;                  // polarity ("vsync_blank_dark") of those records
  size_t guard_last_off = (size_t)-1;       // byte offset inside WS_GUARD of the most recent guarded call's top-2 records (tsdr_sync_guard_margins)
  int guard_last_frames = 0, guard_last_nbx = 0, guard_last_nby = 0;
  struct Buf { void *p = nullptr; size_t cap = 0; } ws[tsdr::WS_COUNT];
  // profiling
  bool prof_on = false;
  std::vector<tsdr::ProfRec> prof;
  std::vector<hipEvent_t> ev_pool;
  struct ProfAgg { std::string name; double ms; long long n; };
  std::vector<ProfAgg> prof_agg;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  // FFT state
  float2 *tw_small = nullptr;  // W_4096^e, e < 4096
  std::map<int, tsdr::TwTable> tw;
  std::map<unsigned, float2 *> twg;  // mixed-radix FFT: W_{R*Rn}^(col*k) tables of the last strided pass, key R << 16 | Rn
  std::map<size_t, tsdr::BluesteinPlan> blu;
  // Float64 segment / resampler transforms (spectra64.hip): W_n^e in f64, built once per length n -- e < n for n <= 4096, else
  // two levels (W_n^j, j < 4096, then W_n^(4096 h)); Bluestein chirp + transformed wrapped conj chirp per length
  std::map<size_t, double2 *> tw64;
  std::map<size_t, double2 *> blu64;
  // tsdr_argmax_d: two device key slots (each launch clears the other one) and a pinned host word for the readback
  unsigned long long *amax_keys = nullptr, *amax_host = nullptr, *amax_host_dev = nullptr;
  int amax_slot = 0;
  bool amax_dirty = false;   // a fused findmax may have left keys in the slot words (autocorr.hip:amax_begin clears them)
  unsigned long long amax_seq = 0;
  tsdr::Pipeline pipe;              // tsdr_frames_submit_d: the internal streams, their events, and the choice of arrangement
  int opt_pipe_mode = -1;           // -1: the measured choice; 0: image lane + tail lane; 1: whole buffers alternate between opt_pipe_lanes
                                    // equal lanes, only shift + IIR chained; 2: one internal stream (the sequential order)
  int opt_pipe_lanes = 2;           // equal lanes of the forced arrangement 1: 2 or 3
  int opt_pipe_priority = 1;        // forced arrangement 0: the tail lane is a stream of the highest priority
  int opt_pipe_ext_event = 1;       // 1: a buffer's tail event rides on its shift + IIR dispatch (hipExtLaunchKernelGGL's stop event) instead of
                                    // a marker packet of its own behind it (the event is an argument of sync.hip:shift_iir_d)
  int opt_pipe_dev_events = 1;      // the pipeline's hand-over events release to device scope (TSDR_PIPE_DEV_EVENTS=0: the default system scope; A/B)
  int opt_pipe_tune = 1;            // 0: "pipe_mode" -1 means arrangement 0 with rasters, 1 without (rounds 1-4), nothing is measured
  int opt_pipe_pin = -1;            // "pipe_pin" k >= 0: arrangement k of loop_policy.h:kCands, nothing measured; -1: not pinned
  int opt_frames_overlap = 1;       // "frames_overlap": tsdr_frames_d / _sc16_d / _iq_d leave a buffer's tail on the pipeline's tail lane, beside the
                                    // next call's image launch (frames.hip:frames_run); 0: every call on the context's stream, as before;
                                    // 1: while this is the device's only context; 2: whatever else lives on the device
  // Every host-side wait of this library is bounded (round 6): a stream that does not complete within opt_wait_ms returns
  // TSDR_EHIP with the waiting stage in tsdr_last_error instead of holding the caller's thread (a GUI task inside a ccall) for
  // good.  0: unbounded (plain hipStreamSynchronize).  Option "wait_ms" / TSDR_WAIT_MS.
  int opt_wait_ms = 30000;
  hipEvent_t wait_ev = nullptr;     // the marker a bounded wait polls (created on first use)
  unsigned long long wait_timeouts = 0;   // bounded waits that gave up (tsdr_wait_stats)
  unsigned long long guard_uncounted = 0; // guard ring entries that never arrived within their bound / were overwritten unread
  bool guard_late = false;          // the last awaited guard entry timed out: later ones get a short bound until one arrives
  // tsdr_frames_overlap_stats: which route the tsdr_frames_d / _sc16_d / _iq_d calls of this context took (frames.hip:frames_run).
  // Host-side counters; nothing reads them but that entry point.
  unsigned long long run_on_lanes = 0, run_sequential = 0;
  unsigned run_why = 0;             // why the latest sequential call was one: 1 option / contexts on the device, 2 profiling, 4 TSDR_EXACT, 8 adopted stream
  int hold_tail_ms = 0;             // tsdr_debug_hold_tail: one-shot host-side delay on the tail lane of the next call that takes the lanes (0: none)
  void *stage_small = nullptr;      // host_stage.h: the pinned block small results of the host forms land in (allocated on first use)
  std::vector<void *> stage_kept;   // ... and the temporaries of calls whose wait gave up: a copy may still touch them, so nothing frees them
                                    // before tsdr_destroy has seen the stream complete
  int opt_beta_waves = 4;           // wavefronts per k_beta workgroup (4 or 8): alone the two tie; beside the pipeline's image kernel a 256-thread
                                    // workgroup fits the holes its retiring workgroups leave (raster-free 357 k vs 309 k frames/s)

  void *scratch(int slot, size_t bytes);  // nullptr on failure (err set)
};

namespace tsdr {

int set_err(tsdr_ctx *ctx, int status, const char *fmt, ...);
int hip_fail(tsdr_ctx *ctx, hipError_t e, const char *what);
// A kernel that asks for more than 64 KiB of dynamic LDS has to be opted in -- once per (device, function): the attribute
// belongs to the device's function object, and one process may hold contexts on several devices (tsdr_group_*).
int lds_opt_in(tsdr_ctx *ctx, const void *fn, size_t bytes);
// frames.hip: order the context's stream behind every buffer submitted to the pipeline (tsdr_frames_submit_d)
int pipe_drain(tsdr_ctx *ctx);
int pipe_sync_lanes(tsdr_ctx *ctx);    // bounded host-side wait for the pipeline's internal streams (TSDR_EHIP when one is stuck)
// A tsdr_frames_d call that left its tail on the lanes promised its caller stream order, not a flush point: everything the
// context's stream is about to receive -- any launch (TSDR_LAUNCH), a copy, a timing event -- comes behind those tails.
int contexts_on_device(int device);   // ctx.hip: contexts alive on it (tsdr_create .. tsdr_destroy)
void hold_cb(void *ms);               // ctx.hip: the host function of tsdr_debug_hold_stream / tsdr_debug_hold_tail (sleeps (intptr_t)ms milliseconds)
static inline int run_fence(tsdr_ctx *c) { return c->pipe.n && c->pipe.from_run ? pipe_drain(c) : (int)TSDR_OK; }
static inline PipeOpts pipe_opts(const tsdr_ctx *c) {
  return PipeOpts{c->opt_pipe_mode, c->opt_pipe_lanes, c->opt_pipe_priority, c->opt_pipe_tune, c->opt_pipe_pin};
}
// bounded host-side waits (ctx.hip): poll a marker event, first spinning, then in short sleeps; TSDR_EHIP + message after
// ctx->opt_wait_ms.  `what` names the stage for tsdr_last_error.
int wait_stream(tsdr_ctx *ctx, hipStream_t s, const char *what);
int wait_event(tsdr_ctx *ctx, hipEvent_t e, const char *what);
// ring.hip: n samples of an integer format (one-sample aligned) -> ComplexF32 at `out` (8-byte aligned), the loaders' product
int iq_expand(tsdr_ctx *ctx, const void *iq, const IqFmt &f, size_t n, float2 *out);
void prof_begin(tsdr_ctx *ctx, const char *name);
void prof_end(tsdr_ctx *ctx);

#define TSDR_HIP(ctx, call)                                          \
  do {                                                               \
    hipError_t _e = (call);                                          \
    if (_e != hipSuccess) return tsdr::hip_fail((ctx), _e, #call);   \
  } while (0)

// Launch a kernel on the context's stream; when profiling is on the launch is
// bracketed by its own hipEvent pair so bench.py can read per-kernel durations live.  A launch that goes to the context's
// stream itself (not to a lane: LaneScope) first orders that stream behind what tsdr_frames_d left on the lanes (run_fence).
#define TSDR_LAUNCH(ctx, kname, kernel, grid, block, shmem, ...)                              \
  do {                                                                                        \
    if ((ctx)->launch_stream == (ctx)->stream) {                                              \
      int _rf = tsdr::run_fence((ctx));                                                       \
      if (_rf) return _rf;                                                                    \
    }                                                                                         \
    if ((ctx)->prof_on) tsdr::prof_begin((ctx), kname);                                       \
    hipLaunchKernelGGL(kernel, grid, block, shmem, (ctx)->launch_stream, __VA_ARGS__);               \
    if ((ctx)->prof_on) tsdr::prof_end((ctx));                                                \
    hipError_t _le = hipGetLastError();                                                       \
    if (_le != hipSuccess) return tsdr::hip_fail((ctx), _le, kname);                          \
  } while (0)

// The pointer rule of every device-pointer entry point (tempest_hip.h, Conventions): a pointer is aligned to one element of
// what it points to -- 4 bytes for float / int, 8 for ComplexF32 / double, 16 for ComplexF64 -- or the call is refused on the
// host, before anything is enqueued.  What a kernel may assume beyond that (16-byte vectors) it has to check for itself.
#define TSDR_PTR_ALIGNED(ctx, fn, p, elem)                                                                     \
  do {                                                                                                         \
    if (reinterpret_cast<uintptr_t>(p) & (uintptr_t)((elem) - 1))                                              \
      return tsdr::set_err((ctx), TSDR_EINVAL, "%s: %s is not aligned to one element (%d bytes)", fn, #p, (int)(elem)); \
  } while (0)

static inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// The `iq, iq_fmt, scale` arguments of the *_iq_d entry points (tempest_hip.h, TSDR_IQ_*): a known format, the pointer aligned
// to one sample of it (8 / 4 / 2 bytes) -- else TSDR_EINVAL with the argument's name, before anything is enqueued.  (The host-pointer
// forms check the format alone: TSDR_IQ_FMT_ARG.)
#define TSDR_IQ_FMT_ARG(ctx, fn, iq_fmt)                                                                                    \
  do {                                                                                                                       \
    if ((iq_fmt) < TSDR_IQ_CF32 || (iq_fmt) > TSDR_IQ_UC8)                                                                    \
      return tsdr::set_err((ctx), TSDR_EINVAL, "%s: iq_fmt %d is not a TSDR_IQ_* format", fn, (int)(iq_fmt));                \
  } while (0)
#define TSDR_IQ_ARG(ctx, fn, iq, iq_fmt, scale, f)                                                                          \
  do {                                                                                                                       \
    TSDR_IQ_FMT_ARG(ctx, fn, iq_fmt);                                                                                        \
    (f) = tsdr::IqFmt{(iq_fmt), (iq_fmt) == TSDR_IQ_CF32 ? 1.0f : (scale)};                                                  \
    if (reinterpret_cast<uintptr_t>(iq) % tsdr::iq_bytes(f))                                                                 \
      return tsdr::set_err((ctx), TSDR_EINVAL, "%s: iq is not aligned to one sample of its format (%d bytes)", fn, (int)tsdr::iq_bytes(f)); \
  } while (0)

// grid for a capped, grid-strided streaming kernel of 256-thread workgroups
static inline int stream_blocks(int cu_count, size_t work_items) {
  size_t blocks = ceil_div(work_items, 256);
  size_t cap = (size_t)(cu_count > 0 ? cu_count : 256) * 8;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}
static inline int stream_grid(tsdr_ctx *ctx, size_t work_items) { return stream_blocks(ctx->cu_count, work_items); }

static inline int ilog2(size_t v) { int l = 0; while ((size_t(1) << l) < v) ++l; return l; }
static inline bool is_pow2(size_t v) { return v && !(v & (v - 1)); }

// ---- imresize coordinate helpers (shared host/device; mirrors oracle resize_axis /
// resize_coord / lin_pos, i.e. ImageTransformations.imresize! + Interpolations Linear) ----
struct RsAxis { double sf, off, n_in; };

__host__ __device__ inline RsAxis rs_axis(size_t n_in, size_t n_out) {
  RsAxis a;
  a.sf = (double)n_in / (double)n_out;
  a.off = (1.0 - 0.5) - a.sf * (1.0 - 0.5);
  a.n_in = (double)n_in;
  return a;
}

#ifdef __HIPCC__
// x = sf*i + off with two roundings (no FMA), clamped to [1, n_in]; returns the 0-based
// left sample index and the f64 weight of the right sample.
__device__ inline unsigned rs_pos(const RsAxis &a, double i1, double &delta) {
  double x = __dadd_rn(__dmul_rn(a.sf, i1), a.off);
  x = fmax(x, 1.0);
  x = fmin(x, a.n_in);
  double xf = floor(x);
  if (xf > a.n_in - 1.0) xf -= 1.0;
  delta = x - xf;
  return (unsigned)xf - 1u;
}
// The same for positions known to lie strictly inside (1, n_in): no clamps, no end-of-signal case -- the identical x, floor and
// delta with four f64 instructions fewer.  Callers establish the precondition per tile (k_raster_tile: every pixel of a tile
// that does not hold the first or last few pixels of the frame).
__device__ inline unsigned rs_pos_inner(const RsAxis &a, double i1, double &delta) {
  const double x = __dadd_rn(__dmul_rn(a.sf, i1), a.off);
  const double xf = floor(x);
  delta = x - xf;
  return (unsigned)xf - 1u;
}
// (1-d)*a + d*b in f64 (two products, one sum, no FMA), rounded once to f32
__device__ inline float rs_blend(float a, float b, double d) {
  double v = __dadd_rn(__dmul_rn(1.0 - d, (double)a), __dmul_rn(d, (double)b));
  return (float)v;
}
// |re + i*im| = f32( sqrt_f64( re^2 + im^2 ) ), the squares exact in f64
__device__ inline float abs_c(float re, float im) {
  double s = __dadd_rn(__dmul_rn((double)re, (double)re), __dmul_rn((double)im, (double)im));
  float r = (float)sqrt(s);
  if (isinf(re) || isinf(im)) r = INFINITY;
  return r;
}
// one IQ sample of a frame's buffer (k in samples) from integer storage: the same product the ring's expansion kernels form.
// An 8-bit sample is one 2-byte load (a frame of an 8-bit buffer starts at byte 2*f*S: nothing wider is aligned).
constexpr float kUc8Offset = 127.5f;   // uc8: value = (f32(code) - 127.5) * scale; the subtraction is exact, the product the one rounding
__device__ inline float2 cvt_sc16(short2 v, float scale) { return make_float2(__fmul_rn((float)v.x, scale), __fmul_rn((float)v.y, scale)); }
__device__ inline float2 cvt_sc8(unsigned v, float scale) {   // v: the two bytes, I in the low one
  return make_float2(__fmul_rn((float)(signed char)(v & 0xFFu), scale), __fmul_rn((float)(signed char)((v >> 8) & 0xFFu), scale));
}
__device__ inline float2 cvt_uc8(unsigned v, float scale) {
  return make_float2(__fmul_rn(__fsub_rn((float)(v & 0xFFu), kUc8Offset), scale),
                     __fmul_rn(__fsub_rn((float)((v >> 8) & 0xFFu), kUc8Offset), scale));
}
__device__ inline float2 ld_iq(const float *__restrict__ src, unsigned k, const IqFmt &f) {
  if (f.kind == IQK_SC16) return cvt_sc16(reinterpret_cast<const short2 *>(src)[k], f.scale);
  if (f.kind >= IQK_SC8) {   // one load and one instruction stream for both 8-bit formats (sc8: f32(code) - 0 is f32(code))
    const unsigned v = reinterpret_cast<const unsigned short *>(src)[k];
    const bool uc = f.kind == IQK_UC8;
    const int i = uc ? (int)(v & 0xFFu) : (int)(signed char)(v & 0xFFu), q = uc ? (int)(v >> 8) : (int)(signed char)(v >> 8);
    const float off = uc ? kUc8Offset : 0.f;
    return make_float2(__fmul_rn(__fsub_rn((float)i, off), f.scale), __fmul_rn(__fsub_rn((float)q, off), f.scale));
  }
  return reinterpret_cast<const float2 *>(src)[k];
}
// The same with the format fixed at compile time (IQF_CF32 / IQF_SC16 / IQF_SC8 / IQF_UC8: the FAST image kernels, whose
// register allocation and instruction stream must not pay for the other formats) or read from the launch's parameters
// (IQF_RT: every other reader)
enum { IQF_CF32 = 0, IQF_SC16 = 1, IQF_RT = 2, IQF_SC8 = 3, IQF_UC8 = 4 };
// the compile-time twin of a run-time format (IqFmt::kind), and the one place a launch site of the per-function paths goes from
// the one to the other: fn(std::integral_constant<int, IQF_*>{}) is called for the integer format `iqf` holds (IQF_SC16 / _SC8 /
// _UC8: the kernels with a format argument there exist for those only)
constexpr int iqf_of(int iqk) { return iqk == IQK_SC16 ? IQF_SC16 : iqk == IQK_SC8 ? IQF_SC8 : iqk == IQK_UC8 ? IQF_UC8 : IQF_CF32; }
template <typename F>
inline int with_int_iqf(int iqf, F &&fn) {
  if (iqf == IQF_SC16) return fn(std::integral_constant<int, IQF_SC16>{});
  if (iqf == IQF_SC8) return fn(std::integral_constant<int, IQF_SC8>{});
  return fn(std::integral_constant<int, IQF_UC8>{});
}
enum { IQN_SC16 = 0, IQN_SC8 = 1, IQN_UC8 = 2 };   // index of an integer format's launch name in a {"..._sc16", "..._sc8", "..._uc8"} table
constexpr int iqf_name(int iqf) { return iqf == IQF_SC16 ? IQN_SC16 : iqf == IQF_SC8 ? IQN_SC8 : IQN_UC8; }
// one integer sample's bits (I in the low half: 32 bits of sc16, 16 of the 8-bit formats) -> ComplexF32
template <int IQF>
__device__ inline float2 cvt_iq(unsigned w, float scale) {
  if (IQF == IQF_SC16) return cvt_sc16(make_short2((short)(w & 0xFFFFu), (short)(w >> 16)), scale);
  return IQF == IQF_SC8 ? cvt_sc8(w, scale) : cvt_uc8(w, scale);
}
template <int IQF>
__device__ inline float2 ld_iq_as(const float *__restrict__ src, unsigned k, const IqFmt &f) {
  if (IQF == IQF_CF32) return reinterpret_cast<const float2 *>(src)[k];
  if (IQF == IQF_SC16) {
    const short2 v = reinterpret_cast<const short2 *>(src)[k];
    return make_float2(__fmul_rn((float)v.x, f.scale), __fmul_rn((float)v.y, f.scale));
  }
  if (IQF == IQF_SC8) return cvt_sc8(reinterpret_cast<const unsigned short *>(src)[k], f.scale);
  if (IQF == IQF_UC8) return cvt_uc8(reinterpret_cast<const unsigned short *>(src)[k], f.scale);
  return ld_iq(src, k, f);
}
// bytes per IQ sample in a buffer of that format (frame strides are counted in samples; an 8-bit sample is half a float, so
// a frame's base is offset in bytes)
__host__ __device__ inline size_t iq_bytes(const IqFmt &f) { return f.kind == IQK_CF32 ? 8 : f.kind == IQK_SC16 ? 4 : 2; }
template <int IQF>
__host__ __device__ inline size_t iq_bytes_as(const IqFmt &f) {
  return IQF == IQF_CF32 ? 8 : IQF == IQF_SC16 ? 4 : (IQF == IQF_SC8 || IQF == IQF_UC8) ? 2 : iq_bytes(f);
}
// base of the frame that starts `samples` samples into an IQ buffer (8-bit formats: 2-byte aligned, no more)
__host__ __device__ inline const float *iq_at(const float *in, size_t samples, size_t bytes_per_sample) {
  return reinterpret_cast<const float *>(reinterpret_cast<const char *>(in) + samples * bytes_per_sample);
}
__device__ inline float abs2_c(float re, float im) { return __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)); }
#endif

}  // namespace tsdr

// the staging path of the host-pointer entry points (HostStage, host_map, read_back), over the context declared above
#define TSDR_HOST_STAGE_WITH_CTX
#include "host_stage.h"
