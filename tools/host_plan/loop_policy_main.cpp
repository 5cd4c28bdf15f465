// Stand-alone host program (no GPU needed or touched, no HIP header): replays the scenario list of loop_policy_scenarios.h
// through csrc/loop_policy.h -- PipeTuner called in the order frames.hip:frames_submit calls it, GuardRoute as
// frames.hip:guard_auto_update and guard_plan do -- and prints one line per step.
//   loop_policy              every scenario (tests/test_loop_policy_host.py compares this with tests/golden/loop_policy_v1.txt)
//   loop_policy NAME         the steps of one scenario
// Build:  c++ -std=c++17 tools/host_plan/loop_policy_main.cpp -o loop_policy
//    or:  hipcc --cuda-host-only -x hip -std=c++17 tools/host_plan/loop_policy_main.cpp -o loop_policy
#include "../../tempestsdr.jl_amd/csrc/loop_policy.h"
#include "loop_policy_scenarios.h"

using namespace tsdr;
using namespace loop_scn;

struct Model {
  std::deque<Boundary> script;
  PipeOpts o;
  PipeTuner tuner;
  int cand_now = -1;
  GuardRoute guard;
  bool guard_auto = true;

  Sub submit(const Key &k) {
    PipeKey key;
    key.nb = k.nb; key.S = k.S; key.y_t = k.y_t; key.x_t = k.x_t; key.raster = k.raster; key.prec = k.prec; key.align = k.align;
    key.iq_kind = k.iq_kind; key.sync = (const void *)(size_t)(0x1000 * k.sync);
    tuner.select(key, o);
    const bool quiesce = tuner.trial_complete();
    if (quiesce) {
      Boundary b{0, true, 12.f};
      if (!script.empty()) { b = script.front(); script.pop_front(); }
      if (b.wait_rc) return Sub{b.wait_rc, -1, true, -1};
      tuner.record_trial(b.timer_ok, b.elapsed_ms);
    }
    cand_now = tuner.candidate();
    return Sub{0, cand_now, quiesce, tuner.submitted(o)};
  }

  // (the normalisation of each value is tsdr_set_option's)
  int option(const char *name, int v) {
    if (!std::strcmp(name, "pipe_mode")) o.mode = v < 0 ? -1 : v > 2 ? 2 : v;
    else if (!std::strcmp(name, "pipe_lanes")) o.lanes = v == 3 ? 3 : 2;
    else if (!std::strcmp(name, "pipe_priority")) o.priority = v != 0;
    else if (!std::strcmp(name, "pipe_tune")) { o.tune = v != 0; tuner.reset(); }
    else if (!std::strcmp(name, "pipe_pin")) { if (v >= kTuneCands) return -1; o.pin = v < 0 ? -1 : v; }
    else if (!std::strcmp(name, "pipe_measure")) { if (v) tuner.measure_now(); }
    else if (!std::strcmp(name, "sync_guard_ppb")) guard.restart();
    else if (!std::strcmp(name, "sync_guard_auto")) { guard_auto = v != 0; guard.set_auto(guard_auto); }
    else return -1;
    return 0;
  }

  Info info() const {
    const PipeInfo p = tuner.info(o, cand_now);
    Info i{p.trials_left, p.chosen, {}, p.text};
    for (int c = 0; c < kTuneCands; ++c) i.ms[c] = p.ms[c];
    return i;
  }

  Decoded guard_entry(unsigned long long w) {
    const GuardRoute::Entry e = GuardRoute::decode(w);
    guard.fold(e.frames, e.flagged, guard_auto);
    return Decoded{e.tag, e.frames, e.flagged};
  }
  bool guard_buffer() {
    if (!(guard_auto && guard.exact_now)) return false;
    ++guard.buffers_exact;
    return true;
  }
  GuardNow guard_now() const { return GuardNow{guard.win_c, guard.win_f, guard.exact_now ? 1 : 0, guard.switches, guard.buffers_exact}; }
};

int main(int argc, char **argv) {
  if (argc > 2) { std::fprintf(stderr, "usage: %s [SCENARIO]\n", argv[0]); return 2; }
  const std::string want = argc == 2 ? std::string(argv[1]) + "." : "";
  bool found = false;
  for (const std::string &l : run_all<Model>()) {
    if (l.compare(0, want.size(), want)) continue;
    found = true;
    std::puts(l.c_str());
  }
  if (!found) { std::fprintf(stderr, "no scenario %s\n", argv[1]); return 1; }
  return 0;
}
