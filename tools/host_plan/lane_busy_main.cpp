// Stand-alone host program (no GPU needed or touched, no HIP header): the lane bookkeeping of the frame loop's pipeline
// (csrc/loop_policy.h: LaneBusy, overlap_allowed) through the transitions frames.hip and ctx.hip make, one scenario per block.
// Prints one line per scenario and returns non-zero at the first expectation that does not hold
// (tests/test_lane_busy_host.py builds and runs it; under ASan + UBSan: tools/asan_host_loop_policy.sh's flags).
// Build:  c++ -std=c++17 tools/host_plan/lane_busy_main.cpp -o lane_busy
#include "../../tempestsdr.jl_amd/csrc/loop_policy.h"

using namespace tsdr;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("  FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// frames.hip:pipe_sync_lanes over the pool; `stuck`: streams whose bounded wait gives up.  Returns the streams it waited for.
static unsigned sync_lanes(LaneBusy &b, unsigned stuck, bool *ok) {
  unsigned waited = 0;
  *ok = true;
  for (int i = 0; i < kPoolN + kPoolH; ++i) {
    if (!b.busy(i)) continue;
    waited |= 1u << i;
    if (stuck >> i & 1u) { *ok = false; return waited; }
    b.lane_idle(i);
  }
  return waited;
}

int main() {
  const unsigned run_lanes = 1u << kCands[2].s[0] | 1u << kCands[2].s[1];   // image lane + tail lane of tsdr_frames_d
  bool ok = false;

  std::puts("fresh: nothing to wait for");
  { LaneBusy b; EXPECT(sync_lanes(b, 0, &ok) == 0 && ok); b.host_saw_stream(); EXPECT(b.mask == 0); }

  std::puts("submit, synchronize: the next change of configuration waits for no lane");
  { LaneBusy b; b.submit(run_lanes); b.submit(run_lanes); b.drain(); b.host_saw_stream();
    EXPECT(b.mask == 0); EXPECT(sync_lanes(b, ~0u, &ok) == 0 && ok); }

  std::puts("submit, change of configuration with buffers in flight: only the arrangement's lanes are waited for");
  { LaneBusy b; b.submit(run_lanes); EXPECT(sync_lanes(b, 0, &ok) == run_lanes && ok); EXPECT(b.mask == 0); }

  std::puts("a wait for the context's stream without a drain says nothing about the lanes");
  { LaneBusy b; b.submit(run_lanes); b.host_saw_stream(); EXPECT(b.mask == run_lanes); }

  std::puts("drain, then another submission: the earlier drain does not cover it");
  { LaneBusy b; b.submit(run_lanes); b.drain(); b.submit(run_lanes); b.host_saw_stream(); EXPECT(b.mask == run_lanes);
    b.drain(); b.host_saw_stream(); EXPECT(b.mask == 0); }

  std::puts("a drain with nothing new submitted stays valid (pipe_drain returns early)");
  { LaneBusy b; b.submit(run_lanes); b.drain(); b.host_saw_stream(); b.host_saw_stream(); EXPECT(b.mask == 0 && b.drained); }

  std::puts("two arrangements in turn: both sets stay marked until seen idle");
  { LaneBusy b; b.submit(1u << 0); b.submit(run_lanes); EXPECT(b.mask == (run_lanes | 1u));
    EXPECT(sync_lanes(b, 0, &ok) == (run_lanes | 1u) && ok); EXPECT(b.mask == 0); }

  std::puts("a submission fails half-way and its lane wait gives up: a later drain + wait on the stream must NOT clear the lanes");
  { LaneBusy b; b.submit(run_lanes); b.drain();            // an earlier, complete submission, drained
    b.submit(run_lanes); b.failed();                        // the failed one: launches on the image lane behind no tail event
    EXPECT(sync_lanes(b, 1u << kCands[2].s[0], &ok) != 0 && !ok);   // SubmitGuard's wait: the image lane is stuck
    b.drain(); b.host_saw_stream();                         // tsdr_synchronize later on: orders the stream behind the EARLIER tail only
    EXPECT(b.busy(kCands[2].s[0]));
    EXPECT(sync_lanes(b, 0, &ok) != 0 && ok); EXPECT(b.mask == 0 && !b.unordered);   // the lanes seen idle one by one: clean again
    b.submit(run_lanes); b.drain(); b.host_saw_stream(); EXPECT(b.mask == 0); }

  std::puts("a submission fails and its lane wait succeeds: clean at once");
  { LaneBusy b; b.submit(run_lanes); b.failed(); EXPECT(sync_lanes(b, 0, &ok) == run_lanes && ok); EXPECT(b.mask == 0 && !b.unordered); }

  std::puts("\"frames_overlap\": 0 never, 1 while the context is alone on its device, 2 always");
  { EXPECT(!overlap_allowed(0, 1) && !overlap_allowed(0, 2));
    EXPECT(overlap_allowed(1, 1) && !overlap_allowed(1, 2) && !overlap_allowed(1, 3));
    EXPECT(overlap_allowed(2, 1) && overlap_allowed(2, 2)); }

  std::printf("%d expectation(s) failed\n", failures);
  return failures ? 1 : 0;
}
