// The scenario list of the loop-policy record (tests/golden/loop_policy_v1.txt), and the line format.
//
// A scenario is a history of one context: options set, buffers submitted, trial boundaries whose waits and elapsed times are
// scripted, guard ring entries arriving.  It is written against a Model, so that the same list drives the library's
// loop_policy.h (loop_policy_main.cpp) and -- when the record is made -- the code that decided all this before that header
// existed.  A Model has:
//   std::deque<Boundary> script     what the next trial boundaries find (empty: every wait succeeds, the timer reads 12 ms)
//   Sub submit(const PipeKey &)     one tsdr_frames_submit_*: status, arrangement, was the pipeline run empty for a trial
//                                   boundary, which timing event was recorded behind the tail (-1: none)
//   int option(name, value)         tsdr_set_option's "pipe_*" and "sync_guard_*" branches
//   Info info()                     tsdr_frames_pipeline_info
//   Decoded guard_entry(word)       one ring entry arrives and is folded (returns its fields);  bool guard_buffer(): a guarded
//                                   buffer is planned, true = it takes the exact route;  GuardNow guard_now(): the route's state
// One line per step:  <scenario>.<step> <event> | <what happened> | <state afterwards>, floats as their bits.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

namespace loop_scn {

struct Key {   // the fields of a PipeKey, so that this header needs no other
  size_t nb = 30, S = 10000; int y_t = 1000, x_t = 1000, raster = 0, prec = 1, align = 1, iq_kind = 0, sync = 1;
  Key with_nb(size_t v) const { Key k = *this; k.nb = v; return k; }
  Key with_S(size_t v) const { Key k = *this; k.S = v; return k; }
  Key with_yx(int y, int x) const { Key k = *this; k.y_t = y; k.x_t = x; return k; }
};
struct Boundary { int wait_rc; bool timer_ok; float elapsed_ms; };
struct Sub { int rc, cand; bool quiesce; int timed; };
struct Info { int trials_left, chosen; float ms[8]; std::string text; };
struct Decoded { unsigned tag, frames, flagged; };
struct GuardNow { unsigned win_c, win_f; int exact_now; unsigned long long switches, buffers_exact; };

static inline std::string fmt(const char *f, ...) {
  char b[2048];
  va_list ap;
  va_start(ap, f);
  vsnprintf(b, sizeof b, f, ap);
  va_end(ap);
  return b;
}
static inline unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }

template <class M>
struct Run {
  M m;
  std::string name;
  int step = 0;
  std::vector<std::string> *out;
  Run(const char *n, std::vector<std::string> *o) : name(n), out(o) {}

  void line(const std::string &event, const std::string &what, const std::string &state) {
    out->push_back(fmt("%s.%d %s | %s | %s", name.c_str(), ++step, event.c_str(), what.c_str(), state.c_str()));
  }
  std::string info_text() {
    const Info i = m.info();
    std::string s = fmt("info=%d,%d,[", i.trials_left, i.chosen);
    for (int c = 0; c < 8; ++c) s += fmt(c ? " %08x" : "%08x", bits(i.ms[c]));
    return s + "],\"" + i.text + "\"";
  }
  // n submissions of one configuration: arrangements run-length coded, the submissions (counted from 1) before which a trial
  // boundary ran the pipeline empty, the timing events recorded as submission:event, and every status that was not 0
  void submit(const char *label, const Key &k, int n) {
    std::string arr, q, ev, rcs;
    int run_c = -2, run_n = 0;
    auto flush = [&]() { if (run_n) arr += fmt(arr.empty() ? "%dx%d" : ",%dx%d", run_c, run_n); };
    for (int i = 1; i <= n; ++i) {
      const Sub s = m.submit(k);
      if (s.quiesce) q += fmt(q.empty() ? "%d" : ",%d", i);
      if (s.rc) { rcs += fmt(rcs.empty() ? "%d:%d" : ",%d:%d", i, s.rc); continue; }
      if (s.timed >= 0) ev += fmt(ev.empty() ? "%d:%d" : ",%d:%d", i, s.timed);
      if (s.cand != run_c) { flush(); run_c = s.cand; run_n = 0; }
      ++run_n;
    }
    flush();
    line(fmt("submit %s x%d", label, n), "arr=" + arr + " quiesce=" + q + " timed=" + ev + " failed=" + rcs, info_text());
  }
  void option(const char *opt, int v) {
    const int rc = m.option(opt, v);
    line(fmt("option %s %d", opt, v), fmt("rc=%d", rc), info_text() + " " + guard_text());
  }
  void boundary(int wait_rc, bool timer_ok, float elapsed_ms) { m.script.push_back(Boundary{wait_rc, timer_ok, elapsed_ms}); }
  // a whole measurement's 17 boundaries: the warm-up trial, then two passes of elapsed times (a negative one: the timer fails)
  void measurement(float warm, const float (&p1)[8], const float (&p2)[8]) {
    boundary(0, true, warm);
    for (float e : p1) boundary(0, e >= 0.f, e >= 0.f ? e : 0.f);
    for (float e : p2) boundary(0, e >= 0.f, e >= 0.f ? e : 0.f);
  }
  void settle(const char *label, const Key &k) { submit(label, k, 256); }   // 17 trials of 15 buffers, and the one that finds the last complete

  std::string guard_text() {
    const GuardNow g = m.guard_now();
    return fmt("guard=%u,%u,%d,%llu,%llu", g.win_c, g.win_f, g.exact_now, g.switches, g.buffers_exact);
  }
  void entry(unsigned tag, unsigned frames, unsigned flagged) {
    const unsigned long long w = (unsigned long long)tag << 48 | (unsigned long long)frames << 24 | flagged;
    const Decoded d = m.guard_entry(w);
    line(fmt("entry %016llx", w), fmt("tag=%u frames=%u flagged=%u", d.tag, d.frames, d.flagged), guard_text());
  }
  void buffers(int n) {
    std::string r;
    for (int i = 0; i < n; ++i) r += m.guard_buffer() ? 'E' : 'F';
    line(fmt("buffers x%d", n), "route=" + r, guard_text());
  }
};

// elapsed times are those of 12 intervals: 12 ms is 1 ms per buffer, and every value is a small binary fraction
constexpr float kE = 12.f;

template <class M>
std::vector<std::string> run_all() {
  std::vector<std::string> out;
  const Key K0, K1 = K0.with_nb(31);   // (another number of frames per buffer: never a neighbour)

  // ---- the tuner: a full measurement, trial by trial
  {
    Run<M> r("full", &out);
    // the warm-up's 8 ms per buffer appears nowhere; the second pass improves arrangement 3 (to the best), worsens 4 (the first
    // pass's value stays) and brings 7 level with 3: the tie goes to the lower index
    const float p1[8] = {kE, 11.25f, 11.625f, 10.5f, 10.875f, 11.25f, kE, 10.5f};
    const float p2[8] = {kE, 11.25f, 11.625f, 9.75f, kE, 11.25f, kE, 9.75f};
    r.measurement(96.f, p1, p2);
    r.submit("K0", K0, 1);
    r.submit("K0", K0, 14);
    for (int t = 0; t < 16; ++t) r.submit("K0", K0, 15);
    r.submit("K0", K0, 1);
    r.submit("K0", K0, 40);
  }
  // ---- both sides of the 1.5 % rule: 11.8125 / 12 = 0.984375 is chosen, 11.828125 / 12 = 0.98567... is not
  for (int side = 0; side < 2; ++side) {
    Run<M> r(side ? "rule-above" : "rule-below", &out);
    float p[8];
    for (int c = 0; c < 8; ++c) p[c] = kE;
    p[5] = side ? 11.828125f : 11.8125f;
    r.measurement(kE, p, p);
    r.submit("K0", K0, 255);
    r.submit("K0", K0, 3);
  }
  // ---- a failed timing event: in pass 1 only (2), in pass 2 only (3), in both (6: 1e30); then in every trial
  {
    Run<M> r("timer-some", &out);
    const float p1[8] = {kE, kE, -1.f, 11.f, kE, kE, -1.f, kE}, p2[8] = {kE, kE, 11.5f, -1.f, kE, kE, -1.f, kE};
    r.measurement(kE, p1, p2);
    r.submit("K0", K0, 135);
    r.submit("K0", K0, 120);
    r.submit("K0", K0, 3);
  }
  {
    Run<M> r("timer-all", &out);
    const float p[8] = {-1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f};
    r.measurement(kE, p, p);
    r.submit("K0", K0, 255);
    r.submit("K0", K0, 3);
  }
  // ---- a wait that fails once at a trial boundary: the status comes back, nothing is recorded, the next submission tries again
  {
    Run<M> r("wait-fails", &out);
    r.submit("K0", K0, 15);
    r.boundary(-4, true, kE);
    r.boundary(0, true, 6.f);
    r.submit("K0", K0, 1);
    r.submit("K0", K0, 1);
    r.submit("K0", K0, 14);
    r.boundary(-4, true, kE);     // ... and in a measured trial: its time is the one read after the wait that succeeded
    r.boundary(0, true, 9.f);
    r.submit("K0", K0, 3);
  }

  // ---- configuration changes
  {
    Run<M> r("leave-settled", &out);
    const float p[8] = {kE, kE, kE, kE, 9.f, kE, kE, kE};
    r.measurement(kE, p, p);
    r.settle("K0", K0);
    r.submit("K1", K1, 20);
    r.submit("K0", K0, 3);
    r.submit("K1", K1, 3);     // (resumes its trial from the first buffer)
  }
  {
    Run<M> r("leave-mid-trial", &out);
    r.submit("K0", K0, 52);    // warm-up, arrangements 0 and 1 timed, 7 buffers into arrangement 2's trial
    r.submit("K1", K1, 5);
    r.submit("K0", K0, 14);    // arrangement 2 again, from its first buffer
    r.submit("K0", K0, 2);
  }
  {
    Run<M> r("alternation", &out);
    for (int i = 0; i < 6; ++i) { r.submit("K0", K0, 1); r.submit("K1", K1, 1); }
    r.submit("K0", K0, 20);
  }
  {
    // ten configurations, each measured to the end: the table holds 8.  Going back to the first measures it again; going back
    // to the third does too, because the configuration that is left is pushed -- and the oldest evicted -- before the lookup;
    // the tenth is still known
    Run<M> r("eviction", &out);
    for (int k = 0; k < 10; ++k) r.settle(fmt("N%d", k).c_str(), K0.with_nb(40 + k));
    r.submit("N0", K0.with_nb(40), 1);
    r.submit("N2", K0.with_nb(42), 1);
    r.submit("N9", K0.with_nb(49), 1);
    r.submit("N3", K0.with_nb(43), 1);
  }
  {
    Run<M> r("neighbour", &out);
    const float pa[8] = {kE, kE, kE, 9.f, kE, kE, kE, kE};
    r.measurement(kE, pa, pa);
    r.settle("S10000", K0);
    r.submit("S10050", K0.with_S(10050), 2);           // taken over, no trials
    r.submit("S10000", K0, 2);                         // its own measurement is still there
    r.submit("S10050", K0.with_S(10050), 2);           // ... and so is what was taken over
    r.submit("S10900", K0.with_S(10900), 2);           // a neighbour of both: the most recent, which is S10000
  }
  {
    Run<M> r("two-neighbours", &out);
    const float pa[8] = {kE, kE, kE, 9.f, kE, kE, kE, kE}, pb[8] = {kE, kE, kE, kE, kE, 9.f, kE, kE};
    r.measurement(kE, pa, pa);
    r.settle("S10000", K0);
    r.option("pipe_measure", 1);
    r.measurement(kE, pb, pb);
    r.settle("S10100", K0.with_S(10100));              // measured although S10000 is a neighbour: "measure now"
    r.submit("K1", K1, 1);
    r.submit("S10050", K0.with_S(10050), 2);           // both are neighbours and settled: the most recent one's choice, 5
  }
  {
    Run<M> r("unsettled-neighbour", &out);
    r.submit("S10000", K0, 20);
    r.submit("S10050", K0.with_S(10050), 2);           // measured: the neighbour has settled on nothing
    r.submit("S10000", K0, 2);
  }
  {
    // the bounds of near(): strictly inside 0.9 .. 1.1 of S and of y_t * x_t (9000 / 10000 is the double 0.9, 11000 / 10000 the
    // double 1.1)
    Run<M> r("near-bounds", &out);
    r.settle("S9000", K0.with_S(9000));
    r.settle("S11000", K0.with_S(11000));
    r.submit("S10000", K0, 1);                         // 0.9 of one, 1.1 of the other: measured
    r.submit("S9999", K0.with_S(9999), 1);             // 0.90009: taken over from S9000
    r.submit("S10001", K0.with_S(10001), 1);           // 1.09989: taken over -- from the most recent neighbour, which is S9999
    r.settle("P900000", K0.with_nb(32).with_yx(900, 1000));
    r.settle("P1100000", K0.with_nb(32).with_yx(1100, 1000));
    r.submit("P1000000", K0.with_nb(32), 1);
    r.submit("P999000", K0.with_nb(32).with_yx(999, 1000), 1);
    r.submit("P1001000", K0.with_nb(32).with_yx(1001, 1000), 1);
  }
  {
    Run<M> r("not-near", &out);
    r.settle("K0", K0);
    Key k = K0.with_S(10010);
    k.raster = 1; r.submit("raster", k, 1); k.raster = 0;
    k.prec = 0; r.submit("precision", k, 1); k.prec = 1;
    k.align = 0; r.submit("alignment", k, 1); k.align = 1;
    k.iq_kind = 2; r.submit("iq-kind", k, 1); k.iq_kind = 0;
    r.submit("frames", k.with_nb(29), 1);
    k.sync = 2; r.submit("other-sync", k, 1); k.sync = 1;   // (another SyncXY object of the same size: a neighbour)
    r.submit("same", K0, 1);
  }

  // ---- options
  {
    Run<M> r("pin", &out);
    r.submit("K0", K0, 20);
    for (int p = 0; p < 8; ++p) { r.option("pipe_pin", p); r.submit("K0", K0, 2); }
    r.option("pipe_pin", 8);
    r.option("pipe_pin", -5);
    r.submit("K0", K0, 10);     // the trial goes on where it stood, to its last buffer
    r.option("pipe_pin", 3);
    r.submit("K0", K0, 2);      // no boundary while pinned, although the trial is complete
    r.option("pipe_pin", -1);
    r.submit("K0", K0, 2);
  }
  {
    Run<M> r("mode", &out);
    Key ras = K0; ras.raster = 1;
    r.option("pipe_mode", 0); r.submit("K0", K0, 2);
    r.option("pipe_priority", 0); r.submit("K0", K0, 2);
    r.option("pipe_priority", 7); r.submit("K0", K0, 2);
    r.option("pipe_mode", 1); r.submit("K0", K0, 2);
    r.option("pipe_lanes", 3); r.submit("K0", K0, 2);
    r.option("pipe_lanes", 4); r.submit("K0", K0, 2);
    r.option("pipe_mode", 2); r.submit("K0", K0, 2);
    r.option("pipe_mode", 9); r.submit("ras", ras, 2);
    r.option("pipe_mode", -3); r.submit("K0", K0, 2);
  }
  {
    Run<M> r("tune-off", &out);
    Key ras = K0; ras.raster = 1;
    r.settle("K0", K0);
    r.option("pipe_tune", 0);
    r.submit("ras", ras, 2);
    r.submit("K0", K0, 2);
    r.option("pipe_tune", 1);    // nothing is remembered; the count of measurements goes on
    r.submit("K0", K0, 2);
  }
  {
    Run<M> r("measure-now", &out);
    r.option("pipe_measure", 1);            // with nothing submitted
    r.submit("K0", K0, 20);                 // in mid-trial
    r.option("pipe_measure", 0);
    r.submit("K0", K0, 2);
    r.option("pipe_measure", 1);
    r.submit("K0", K0, 2);
    r.settle("K0", K0);                     // on a settled configuration
    r.submit("K0", K0, 2);
    r.option("pipe_measure", 1);
    r.submit("K0", K0, 2);
    r.submit("K1", K1, 2);
    r.option("pipe_measure", 1);            // what the table holds for the configuration goes too
    r.submit("K0", K0, 2);
  }

  // ---- the guard's adaptive route
  {
    Run<M> r("guard", &out);
    unsigned tag = 0;
    r.entry(++tag, 30, 4); r.entry(++tag, 30, 5);      // 9 of 60, closed at exactly 60: 9.f / 60.f is the float 0.15f -- stays
    r.buffers(2);
    r.entry(++tag, 25, 3); r.entry(++tag, 25, 3); r.entry(++tag, 15, 4);   // 10 of 65, closed beyond 60: switches
    r.buffers(3);
    r.entry(++tag, 60, 3);                             // 3 of 60 is 0.05f: stays on the exact route
    r.buffers(1);
    r.entry(++tag, 59, 2); r.entry(++tag, 1, 0);       // 2 of 60: back
    r.buffers(1);
    r.entry(++tag, 30, 5); r.entry(++tag, 30, 5);      // 10 of 60: switches
    r.entry(++tag, 30, 30);
    r.option("sync_guard_auto", 0);                    // off in mid-window: the fast route, entries are not counted
    r.buffers(1);
    r.entry(++tag, 100, 100);
    r.option("sync_guard_auto", 1);                    // (the half window is still there)
    r.entry(++tag, 30, 0);
    r.entry(++tag, 70, 70);
    r.buffers(2);
    r.entry(++tag, 40, 40);
    r.option("sync_guard_ppb", 20);                    // restart in mid-window, on the exact route
    r.buffers(1);
    r.entry(++tag, 59, 59);
    r.option("sync_guard_ppb", 0);                     // ... and on the fast route
    r.entry(++tag, 59, 59); r.entry(++tag, 1, 0);
    r.buffers(1);
    r.entry(0xFFFF, 0xFFFFFF, 0);                      // the fields' widths
    r.entry(++tag, 1, 0);
  }
  return out;
}

}  // namespace loop_scn
