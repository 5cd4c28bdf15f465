// loop_policy.h -- what the frame loop decides on the host between two launches, as plain state: which arrangement of streams
// a pipelined submission runs in (PipeTuner), and which route the sync guard's adaptive switch takes (GuardRoute).
//
// No HIP, no context: frames.hip does the waits, the timing events and the ring poll, and tells these two what happened; a
// host-only program replays whole histories of submissions through them (tools/host_plan/loop_policy_main.cpp, compared with
// tests/golden/loop_policy_v1.txt by tests/test_loop_policy_host.py).
//
// WHICH arrangement on WHICH streams is measured (round 5).  Rounds 3-4 chose by geometry -- an image lane and a high-priority
// tail lane with rasters (+6-8 % on the builder's boxes), two equal lanes without (+13 %) -- and the driver's box then measured
// the former 2 % BELOW one call per buffer.  The cause is not the box: how two streams of a process overlap depends on the
// hardware queues HIP mapped them to, i.e. on how many streams the process had created before (tools/r05_queue_probe.sh: the
// same code with 5 idle streams created first runs the image lane + tail lane at 0.269 instead of 0.151 ms per buffer, with 1
// runs two equal lanes at 0.095 instead of 0.076).  So, like the reference's own FFTW.PATIENT plans (Resampler.jl:31,39), the
// pipeline measures: the first submissions of a configuration run kTrial buffers through each candidate of kCands -- results
// are identical in every arrangement -- timing the interval between the tails of successive buffers, then settle on the
// fastest (the sequential order among them, so a process in which nothing overlaps falls back to it by itself).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

namespace tsdr {

constexpr int kPipeSlots = 3;            // image / key / projection / guard-record slots in rotation
constexpr int kPoolN = 6, kPoolH = 2;    // candidate streams: normal priority / highest priority
constexpr int kTuneCands = 8, kTrial = 15;

// what the slot offsets of the submissions in flight were computed from: frames per buffer (the image slots are that many
// frames apart), the tile plan of (S, y_t, x_t, raster or not, precision) for the projection sums, the SyncXY object's block
// counts for the guard records.  A change of any of them runs the pipeline empty first.
struct PipeKey {
  size_t nb = 0, S = 0; int y_t = 0, x_t = 0, raster = -1, prec = -1, align = -1, iq_kind = 0; const void *sync = nullptr;
  bool operator==(const PipeKey &o) const {
    return nb == o.nb && S == o.S && y_t == o.y_t && x_t == o.x_t && raster == o.raster && prec == o.prec && align == o.align && iq_kind == o.iq_kind && sync == o.sync;
  }
  // the same loop at a slightly different geometry (GUI.jl:492-506: the interactive y_t / x_t corrections move one line at a
  // time): same frames per buffer, raster or not, precision, alignment, input format; S and the raster size within 10 %.
  // What was measured for one holds for the other (the launches have the same shapes and durations within a few percent).
  bool near(const PipeKey &o) const {
    if (!(nb == o.nb && raster == o.raster && prec == o.prec && align == o.align && iq_kind == o.iq_kind)) return false;
    const double s = (double)S / (double)(o.S ? o.S : 1), p = ((double)y_t * x_t) / ((double)o.y_t * o.x_t > 0 ? (double)o.y_t * o.x_t : 1.0);
    return s > 0.9 && s < 1.1 && p > 0.9 && p < 1.1;
  }
};

struct PipeCand { const char *name; int sym, nl, s[3]; };
// sym: whole buffers rotate over nl equal lanes pool[s[0 .. nl)]; !sym: image lane pool[s[0]], tail lane pool[s[1]].
// pool[0 .. kPoolN) are normal-priority streams, pool[kPoolN ..) streams of the highest priority.
static const PipeCand kCands[kTuneCands] = {
    {"one stream (sequential order)", 1, 1, {0, 0, 0}},
    {"image lane + high-priority tail lane", 0, 2, {0, kPoolN, 0}},
    {"image lane + tail lane", 0, 2, {2, 3, 0}},
    {"image lane + high-priority tail lane (other streams)", 0, 2, {4, kPoolN + 1, 0}},
    {"two equal lanes", 1, 2, {0, 1, 0}},
    {"two equal lanes (other streams)", 1, 2, {2, 3, 0}},
    {"two equal lanes (third pair)", 1, 2, {4, 5, 0}},
    {"three equal lanes", 1, 3, {0, 1, 2}},
};

struct PipeOpts {   // the options the choice reads (tsdr_ctx::opt_pipe_*), by value
  int mode = -1, lanes = 2, priority = 1, tune = 1, pin = -1;
  bool measured() const { return pin < 0 && mode < 0 && tune; }
};

struct PipeTune {                 // the measured choice for one PipeKey
  PipeKey key; int state = 0;     // 0: nothing measured; 1: trials running; 2: settled
  int cand = 0, pos = 0, chosen = -1, round = 0;   // round 0: warm-up trial of candidate 0; 1, 2: the two measured passes
  int interrupts = 0;             // times another configuration cut into this one's trials (4: settle on the sequential order)
  bool inherited = false;         // settled by taking over a neighbouring configuration's choice (PipeKey::near), not by trials
  float ms[kTuneCands] = {};      // mean interval between the tails of successive buffers, per arrangement
};

struct PipeInfo {   // tsdr_frames_pipeline_info
  int trials_left = 0, chosen = -1;
  float ms[kTuneCands] = {};
  std::string text;
};

// The arrangement of every submission.  One submission is: select(); if trial_complete(), run the lanes empty, read the two
// timing events and record_trial(); launch in candidate(); submitted().
class PipeTuner {
 public:
  // forced ("pipe_pin", "pipe_mode" >= 0), the geometry rule of rounds 3-4 ("pipe_tune" = 0), or the measured choice -- then a
  // change of configuration is handled here: one measured before, a neighbour of one, or measure now
  void select(const PipeKey &key, const PipeOpts &o) {
    forced_ = o.pin >= 0 ? o.pin : o.mode == 0 ? (o.priority ? 1 : 2) : o.mode == 1 ? (o.lanes == 3 ? 7 : 4) : o.mode == 2 ? 0 : !o.tune ? (key.raster ? 1 : 4) : -1;
    if (forced_ >= 0 || (t_.state != 0 && t_.key == key)) return;
    // what is known about the previous one is kept -- settled or half-way through its trials (a caller that alternates between
    // two configurations resumes each one's trials where it left them instead of starting over on every change); the table
    // holds the 8 most recently used configurations
    if (t_.state != 0) {
      if (done_.size() >= 8) done_.erase(done_.begin());
      if (t_.state == 1) {                    // (the trial that was interrupted is run again from its first buffer)
        t_.pos = 0;
        // a caller that keeps cutting in (two configurations in strict alternation) would never settle and would run the lanes
        // empty at every change: after four interruptions the configuration keeps the sequential order
        if (++t_.interrupts >= 4) { t_.state = 2; t_.chosen = 0; }
      }
      done_.push_back(t_);
    }
    t_ = PipeTune{};
    bool found = false;
    if (force_) {   // "measure now": what the table holds for this configuration goes, neighbours are not consulted
      for (size_t i = done_.size(); i-- > 0;) if (done_[i].key == key) done_.erase(done_.begin() + (long)i);
      force_ = false;
      t_.key = key; t_.state = 1; ++runs_;
      found = true;
    }
    for (size_t i = 0; i < done_.size() && !found; ++i)
      if (done_[i].key == key) { t_ = done_[i]; done_.erase(done_.begin() + (long)i); found = true; }
    for (size_t i = done_.size(); i-- > 0 && !found;)   // (the most recent neighbour first)
      if (done_[i].state == 2 && done_[i].key.near(key)) { t_ = done_[i]; t_.key = key; t_.inherited = true; found = true; }
    if (!found) { t_.key = key; t_.state = 1; ++runs_; }
  }

  // the running trial has had its kTrial buffers: the caller runs the pipeline empty and reports the elapsed time.  A wait
  // that fails returns from the submission with nothing recorded, and the next submission finds the trial still complete.
  bool trial_complete() const { return forced_ < 0 && t_.state == 1 && t_.pos == kTrial; }

  // elapsed_ms: between the timing events of the trial's buffers 2 and kTrial - 1 -- the mean interval between the tails of
  // successive buffers over a whole number of lane rotations (12 intervals: with two or three lanes the tails complete in
  // bursts, so a median of single intervals says nothing), after 3 buffers of ramp-up
  void record_trial(bool timer_ok, float elapsed_ms) {
    t_.pos = 0;
    // the very first trial (the device's clocks and caches as the caller left them) only warms up: measured again, in turn
    if (t_.round == 0) { t_.round = 1; return; }
    const float v = timer_ok ? elapsed_ms / (float)(kTrial - 3) : 1e30f;
    t_.ms[t_.cand] = t_.round == 1 ? v : std::min(t_.ms[t_.cand], v);   // two passes over the candidates, the better of the two
    if (++t_.cand < kTuneCands) return;
    t_.cand = 0;
    if (++t_.round < 3) return;
    int best = 0;
    for (int c = 1; c < kTuneCands; ++c) if (t_.ms[c] < t_.ms[best]) best = c;
    // the sequential order unless something beats it by more than the measurement's noise
    t_.chosen = t_.ms[best] < 0.985f * t_.ms[0] ? best : 0;
    t_.state = 2;
  }

  int candidate() const { return forced_ >= 0 ? forced_ : t_.state == 2 ? t_.chosen : t_.cand; }   // index into kCands

  // the submission is enqueued.  Returns which timing event to record behind its tail: 2, kTrial - 1, or -1 for none -- two
  // per trial (a timed event is a marker packet that holds up the launches behind it for a few microseconds: one per buffer
  // made the one-stream candidate look 10 % slower than it is)
  int submitted(const PipeOpts &o) {
    if (!o.measured() || t_.state != 1 || t_.pos >= kTrial) return -1;
    const int pos = t_.pos++;
    return pos == 2 || pos == kTrial - 1 ? pos : -1;
  }

  // cand_now: the arrangement of the submissions in flight (-1: nothing submitted yet)
  PipeInfo info(const PipeOpts &o, int cand_now) const {
    const PipeTune &t = t_;
    const bool measured = o.measured();
    constexpr int kAll = 2 * kTuneCands + 1;   // the warm-up trial + two passes
    PipeInfo r;
    r.trials_left = !measured ? 0 : t.state == 2 ? 0 : t.state == 1 ? kAll - (t.round == 0 ? 0 : 1 + (t.round - 1) * kTuneCands + t.cand) : kAll;
    r.chosen = measured ? (t.state == 2 ? t.chosen : -1) : cand_now;
    for (int c = 0; c < kTuneCands; ++c) r.ms[c] = measured && (t.state == 2 || t.round == 2 || (t.round == 1 && c < t.cand)) ? t.ms[c] : 0.f;
    std::string &s = r.text;
    if (o.pin >= 0) s = std::string("pinned (\"pipe_pin\"): ") + kCands[o.pin].name;
    else if (!measured) s = std::string("forced: ") + (cand_now >= 0 ? kCands[cand_now].name : "nothing submitted yet");
    else if (t.state != 2) s = "measuring";
    else {
      s = std::string(t.inherited ? "taken over from a neighbouring configuration's measurement: " : "measured: ") + kCands[t.chosen].name + " |";
      char b[96];
      for (int c = 0; c < kTuneCands; ++c) { snprintf(b, sizeof b, " [%d] %s %.4f ms;", c, kCands[c].name, (double)t.ms[c]); s += b; }
    }
    s += " (measurements started on this context: " + std::to_string(runs_) + ")";
    return r;
  }

  void reset() { t_ = PipeTune{}; done_.clear(); }         // "pipe_tune": setting it also discards what was measured
  void measure_now() { t_ = PipeTune{}; force_ = true; }   // "pipe_measure": the next configuration is measured whatever is known
                                                           // about it or its neighbours

 private:
  PipeTune t_;                    // the configuration of the latest measured submission
  std::vector<PipeTune> done_;    // earlier configurations (a caller that goes back to one -- GUI.jl's y_t / x_t corrections, a
                                  // raster asked for now and then -- does not measure it again); <= 8, the oldest goes first
  bool force_ = false;
  unsigned long long runs_ = 0;   // measurements (full sets of trials) started so far
  int forced_ = -1;               // this submission's arrangement when nothing is measured (select)
};

// The sync guard's adaptive route (option "sync_guard_auto"): when more than `hi` of the recent frames were flagged,
// re-evaluating them one by one costs more than running whole buffers in the exact sequence, so the FAST frame loop does that
// until the share (still counted, on the exact statistics) falls below `lo`.  Decided over windows of at least kGuardAutoWindow
// frames, from the per-call counts of the guard's ring entries folded in submission order (frames.hip:guard_auto_update).
constexpr unsigned kGuardAutoWindow = 60;
struct GuardRoute {
  unsigned win_c = 0, win_f = 0;    // frames checked / flagged since the last decision
  bool exact_now = false;
  unsigned long long switches = 0, buffers_exact = 0;
  float hi = 0.15f, lo = 0.05f;

  struct Entry { unsigned tag, frames, flagged; };   // ring word: tag (seq + 1, 16 bits) << 48 | frames << 24 | flagged
  static Entry decode(unsigned long long w) { return Entry{(unsigned)(w >> 48), (unsigned)((w >> 24) & 0xFFFFFFull), (unsigned)(w & 0xFFFFFFull)}; }

  void fold(unsigned frames, unsigned flagged, bool auto_on) {
    if (!auto_on) return;   // (not counted)
    win_c += frames;
    win_f += flagged;
    if (win_c < kGuardAutoWindow) return;
    const float share = (float)win_f / (float)win_c;
    if (!exact_now && share > hi) { exact_now = true; ++switches; }
    else if (exact_now && share < lo) { exact_now = false; ++switches; }
    win_c = win_f = 0;
  }
  // "sync_guard_ppb": the history belongs to the old threshold -- start over on the fast route
  void restart() { exact_now = false; win_c = win_f = 0; }
  void set_auto(bool on) { if (!on) exact_now = false; }   // "sync_guard_auto"
};

// Which of the pipeline's pool streams may still hold work, as far as the host knows (bit i: pool[i]).  A host wait for the
// lanes (frames.hip:pipe_sync_lanes) touches only these: an idle stream can share a hardware queue with a stream that is held,
// and a marker on it would wait for that one.  Transitions, in the order frames.hip makes them:
//   submit(mask)       a submission is about to launch on the streams of its arrangement
//   failed()           ... and returned half-way: its launches are behind no event that a later drain would order
//   drain()            pipe_drain ordered the context's stream behind the latest complete submission's tail
//   host_saw_stream()  a host wait for the context's stream completed: after a drain with nothing submitted since, and no
//                      failed submission outstanding, every lane is idle
//   lane_idle(i)       a host wait for pool[i] completed; with the last one a failed submission's launches are done as well
struct LaneBusy {
  unsigned mask = 0;
  bool drained = false, unordered = false;
  void submit(unsigned m) { mask |= m; drained = false; }
  void failed() { unordered = true; }
  void drain() { drained = true; }
  void host_saw_stream() { if (drained && !unordered) mask = 0; }
  bool busy(int i) const { return (mask >> i & 1u) != 0; }
  void lane_idle(int i) { mask &= ~(1u << i); if (!mask) unordered = false; }
};

// Contexts alive per device: tsdr_frames_d takes the lanes only while its context is the device's only one (two contexts on one
// GPU fill each other's gaps already, and their lanes get in each other's way: NOTEBOOK "tsdr_frames_d on the lanes"), unless
// option "frames_overlap" is 2.  overlap_allowed: opt 0 never, 1 alone on the device, 2 always.
inline bool overlap_allowed(int opt, int contexts_on_device) { return opt >= 2 || (opt == 1 && contexts_on_device <= 1); }

}  // namespace tsdr
