// host_stage.h -- the one staging path of the host-pointer entry points.  A call declares which host arrays go up to which workspace
// slot and which come back; begin() enqueues the uploads, the device-pointer form runs, finish() enqueues the downloads and does the
// call's one bounded wait (run() is the three in a row):
//   HostStage st(ctx);
//   float *d_in = (float *)st.in(WS_IN, in, in_bytes), *d_out = (float *)st.out(WS_OUT, out, out_bytes);
//   return st.run(__func__, [&] { return entry_d(ctx, d_in, d_out); });
// The first part of this header is bookkeeping only -- the list of transfers, the NULL and zero-byte rules, the order, who owns a
// temporary -- over a back end B that grows slots, copies and waits.  It includes no HIP header: a stand-alone program drives it
// with a back end that records (tools/host_plan/host_stage_main.cpp, tests/test_host_stage_host.py).  The second part, compiled
// where common.h includes this header, is the back end of a tsdr_ctx, HostStage itself, host_map and read_back.
//
// A declaration returns the device pointer.  Slots grow at the declaration; nothing is enqueued before begin(), which returns
// TSDR_ENOMEM / TSDR_EINVAL if any declaration failed.
//   * A NULL host pointer is an optional array the caller did not pass: a NULL device pointer, no transfer.
//   * Zero bytes are legal: the slot exists (the device form gets a pointer), nothing is copied.
//   * in / out / inout take a whole slot, once per stage.  A slot that holds several arrays is reserve()d first; each declaration
//     on it then takes the next 8-byte aligned range, an absent optional array included (an array's place does not depend on
//     which of its neighbours the caller passed).  in_to / out_from name device memory that is no slot.
//   * At most kStageEntries declarations; one too many, or a range past its reservation, is TSDR_EINVAL.
// Host memory the LIBRARY owns for a transfer belongs to the stage, never to a stack frame: a wait that gives up (wait_stream:
// TSDR_EHIP after wait_ms) leaves the copy enqueued.
//   * small(bytes): results of at most kStageSmall bytes in all (the vsync index pair, the guard counters) land in a pinned block
//     of the context, allocated on first use, freed by tsdr_destroy, read only after a successful finish().  A copy that a
//     timed-out call left pending is ordered, on the same stream, before the copy and the wait of the block's next reader.
//   * temp(bytes): larger temporaries (the guard's margin records, table images).  The stage frees them when it goes out of scope
//     -- unless a copy may still be pending (something enqueued, no successful wait since): then they move to a list on the context
//     that tsdr_destroy releases only where the stream completed (it abandons a stuck context as a whole).
//
// Slots of the host forms (as before this header existed: memory use and aliasing are what the kernels were tested under):
//   host_map (36 entry points)   in WS_IN; out WS_OUT
//   tsdr_frames                  iq WS_IN; state WS_AUX (up, down); frames WS_OUT; raster WS_FFT_A (WS_RASTER is the fallback
//                                path's); sync_idx WS_MISC (with do_align only)
//   tsdr_vsync / _f64            img WS_IN / WS_F64_A; index pair WS_OUT / WS_F64_B -> small
//   tsdr_raster_accum            rasters WS_IN; shifts WS_MISC; state WS_AUX (up, down)
//   tsdr_raster_register         rasters WS_IN; ref WS_AUX; shifts WS_MISC; WS_OUT: shifts_out, then scores
//   tsdr_display_u8              images WS_IN; out WS_OUT; ranges WS_AUX
//   fold, cfold (fold_entry)     iq WS_IN; WS_OUT: the state (up if alpha != 0 and no scan, down) or a scan's scores
//   cstack (stack_entry)         iq WS_IN; zstate WS_OUT (up if alpha != 0, down); WS_AUX: mag, then info
//   ctrack stack                 iq WS_IN; zstate WS_OUT (up if alpha != 0, down); WS_AUX: mag, then info, then the track (up)
//   ctrack probe                 iq WS_IN; out WS_OUT; WS_AUX: zref, then the track (both up)
//   ctrack gram                  iq WS_IN; gram WS_OUT; the track WS_AUX (up)
//   tune (tune_entry)            iq WS_IN; out WS_OUT; WS_AUX: taps (up), then hist (up, down)
//   tsdr_resampler_lpf (f32)     the narrowed H WS_FFT_A
// (WS_MISC is also demod.hip's scratch: no host form above runs a demodulator.)
#pragma once
#include <cstddef>
#include <cstdlib>

#include "../../include/tempest_hip.h"

namespace tsdr {

constexpr int kStageEntries = 8, kStageTemps = 2;
constexpr size_t kStageSmall = 64;

// B: void *grow(int slot, size_t bytes) (nullptr: out of memory), int fence(), int upload(void *dev, const void *host, size_t),
// int download(void *host, const void *dev, size_t), int wait(const char *what), void *small_block() (kStageSmall pinned bytes or
// nullptr), void keep(void *temp) (takes a malloc'ed block over).  The int results are tsdr_status values.
template <class B>
class HostStageT {
 public:
  explicit HostStageT(B b) : b_(b) {}
  HostStageT(const HostStageT &) = delete;
  HostStageT &operator=(const HostStageT &) = delete;
  ~HostStageT() {
    for (int i = 0; i < n_temps_; ++i) {
      if (pending_) b_.keep(temps_[i]);
      else free(temps_[i]);
    }
  }
  // `bytes` of `slot` for the declarations on that slot that follow; the base of the slot
  void *reserve(int slot, size_t bytes) {
    if (find(slot, false) || find(slot, true)) return fail(TSDR_EINVAL);
    void *dev = b_.grow(slot, bytes);
    return dev ? push(Entry{slot, bytes, nullptr, dev, false, false, 0}) : fail(TSDR_ENOMEM);
  }
  void *in(int slot, const void *host, size_t bytes) { return add(slot, nullptr, const_cast<void *>(host), bytes, true, false); }
  void *out(int slot, void *host, size_t bytes) { return add(slot, nullptr, host, bytes, false, true); }
  void *inout(int slot, void *host, size_t bytes, bool upload_if) { return add(slot, nullptr, host, bytes, upload_if, true); }
  void in_to(void *dev, const void *host, size_t bytes) { (void)add(-1, dev, const_cast<void *>(host), bytes, true, false); }
  void out_from(const void *dev, void *host, size_t bytes) { (void)add(-1, const_cast<void *>(dev), host, bytes, false, true); }
  void *small(size_t bytes) {
    char *base = (char *)b_.small_block();
    if (!base) return fail(TSDR_ENOMEM);
    if (small_used_ + bytes > kStageSmall) return fail(TSDR_EINVAL);
    void *p = base + small_used_;
    small_used_ += (bytes + 7) & ~(size_t)7;
    return p;
  }
  void *temp(size_t bytes) {
    if (n_temps_ == kStageTemps) return fail(TSDR_EINVAL);
    void *p = malloc(bytes ? bytes : 1);
    return p ? temps_[n_temps_++] = p : fail(TSDR_ENOMEM);
  }
  int begin() {
    if (bad_) return bad_;
    if (int rc = b_.fence()) return rc;
    for (int i = 0; i < n_; ++i)
      if (e_[i].up && e_[i].bytes) {
        if (int rc = b_.upload(e_[i].dev, e_[i].host, e_[i].bytes)) return rc;
        pending_ = true;
      }
    return TSDR_OK;
  }
  int finish(const char *what) {
    for (int i = 0; i < n_; ++i)
      if (e_[i].down && e_[i].bytes) {
        if (int rc = b_.download(e_[i].host, e_[i].dev, e_[i].bytes)) return rc;
        pending_ = true;
      }
    const int rc = b_.wait(what);
    if (!rc) pending_ = false;
    return rc;
  }
  template <class F>
  int run(const char *what, F device_form) {
    if (int rc = begin()) return rc;
    if (int rc = device_form()) return rc;
    return finish(what);
  }
  int run(const char *what) { return run(what, [] { return (int)TSDR_OK; }); }
  // a copy this stage enqueued may not have completed: what it reads or writes has to stay
  bool pending() const { return pending_; }

 private:
  struct Entry {
    int slot;       // -1: `dev` is the caller's
    size_t bytes;
    void *host;     // nullptr: a reservation
    void *dev;
    bool up, down;
    size_t next;    // a reservation's first free byte
  };
  Entry *find(int slot, bool reservation) {
    for (int i = 0; i < n_; ++i)
      if (slot >= 0 && e_[i].slot == slot && !e_[i].host == reservation) return &e_[i];
    return nullptr;
  }
  void *fail(int status) {
    if (!bad_) bad_ = status;
    return nullptr;
  }
  void *push(const Entry &e) {
    if (n_ == kStageEntries) return fail(TSDR_EINVAL);
    e_[n_++] = e;
    return e.dev;
  }
  void *add(int slot, void *dev, void *host, size_t bytes, bool up, bool down) {
    if (Entry *r = find(slot, true)) {
      if (r->next + bytes > r->bytes) return fail(TSDR_EINVAL);
      dev = (char *)r->dev + r->next;
      r->next = (r->next + bytes + 7) & ~(size_t)7;
    } else if (slot >= 0 && host) {
      if (find(slot, false)) return fail(TSDR_EINVAL);
      if (!(dev = b_.grow(slot, bytes))) return fail(TSDR_ENOMEM);
    }
    return host ? push(Entry{slot, bytes, host, dev, up, down, 0}) : nullptr;
  }

  B b_;
  Entry e_[kStageEntries];
  int n_ = 0, n_temps_ = 0, bad_ = TSDR_OK;
  void *temps_[kStageTemps] = {};
  size_t small_used_ = 0;
  bool pending_ = false;
};

}  // namespace tsdr

#ifdef TSDR_HOST_STAGE_WITH_CTX   // common.h: tsdr_ctx, run_fence, wait_stream, TSDR_HIP are declared
namespace tsdr {

struct CtxStageBackend {
  tsdr_ctx *ctx;
  void *grow(int slot, size_t bytes) { return ctx->scratch(slot, bytes); }
  int fence() { return run_fence(ctx); }
  int upload(void *dev, const void *host, size_t bytes) {
    TSDR_HIP(ctx, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return TSDR_OK;
  }
  int download(void *host, const void *dev, size_t bytes) {
    TSDR_HIP(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return TSDR_OK;
  }
  int wait(const char *what) { return wait_stream(ctx, ctx->stream, what); }
  void *small_block() {
    if (!ctx->stage_small && hipHostMalloc(&ctx->stage_small, kStageSmall, hipHostMallocDefault) != hipSuccess) {
      ctx->stage_small = nullptr;
      set_err(ctx, TSDR_ENOMEM, "host staging: no pinned block for small results");
    }
    return ctx->stage_small;
  }
  void keep(void *temp) { ctx->stage_kept.push_back(temp); }
};

struct HostStage : HostStageT<CtxStageBackend> {
  explicit HostStage(tsdr_ctx *ctx) : HostStageT<CtxStageBackend>(CtxStageBackend{ctx}) {}
};

// Host-pointer wrapper of one input and one output: stage `in` to the device, run the device-pointer core on the context's
// stream, copy `out` back, wait.  run(din, dout) returns a tsdr_status.
template <typename F>
static inline int host_map(tsdr_ctx *ctx, const void *in, size_t in_bytes, void *out, size_t out_bytes, F run) {
  if (!ctx) return TSDR_EINVAL;
  if ((in_bytes && !in) || (out_bytes && !out)) return TSDR_EINVAL;
  HostStage st(ctx);
  void *din = in ? st.in(WS_IN, in, in_bytes) : st.reserve(WS_IN, 0);   // (run always gets two device pointers)
  void *dout = out ? st.out(WS_OUT, out, out_bytes) : st.reserve(WS_OUT, 0);
  return st.run("host wrapper: results", [&] { return run(din, dout); });
}

// Read device state back to the caller: first whatever still writes it -- every submitted buffer (drain: pipe_drain), or only the
// tails tsdr_frames_d left on the lanes (the stage's run_fence) --, then the copy and the bounded wait.
static inline int read_back(tsdr_ctx *ctx, bool drain, void *host, const void *dev, size_t bytes, const char *what) {
  if (drain)
    if (int rc = pipe_drain(ctx)) return rc;
  HostStage st(ctx);
  st.out_from(dev, host, bytes);
  return st.run(what);
}

}  // namespace tsdr
#endif
