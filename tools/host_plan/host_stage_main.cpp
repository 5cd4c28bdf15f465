// Stand-alone host program (no GPU needed or touched, no HIP header): the bookkeeping of the host-pointer entry points' staging
// path (csrc/host_stage.h: HostStageT) over a back end that records what it is asked to do and carries the copies out as memcpy --
// at the wait when it succeeds, or LATER (land()) when the wait gives up, as a copy left on a stuck stream would.
// Prints one line per scenario and returns non-zero at the first expectation that does not hold
// (tests/test_host_stage_host.py builds and runs it; under ASan + UBSan: tools/asan_host_loop_policy.sh).
// Build:  c++ -std=c++17 tools/host_plan/host_stage_main.cpp -o host_stage
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../tempestsdr.jl_amd/csrc/host_stage.h"

using namespace tsdr;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("  FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

enum { kSlots = 6, kSlotBytes = 1 << 12 };

struct World {
  struct Copy { bool up; void *dst; const void *src; size_t bytes; };
  std::string log;            // one letter per call: g(row) f(ence) u(pload) d(ownload) w(ait) W(ait that gave up)
  std::vector<Copy> queue;    // enqueued, not carried out yet
  std::vector<Copy> done;     // every copy ever enqueued, in order
  std::vector<void *> kept;   // temporaries handed over
  alignas(16) char slot[kSlots][kSlotBytes];
  size_t grown[kSlots] = {};
  alignas(16) char small[kStageSmall];
  int fail_slot = -1;
  bool stuck = false;
  void land() {
    for (const Copy &c : queue) std::memcpy(c.dst, c.src, c.bytes);
    queue.clear();
  }
  ~World() { for (void *p : kept) free(p); }
};

struct Recorder {
  World *w;
  void *grow(int s, size_t bytes) {
    w->log += 'g';
    if (s == w->fail_slot || bytes > kSlotBytes) return nullptr;
    w->grown[s] = bytes;
    return w->slot[s];
  }
  int fence() { w->log += 'f'; return TSDR_OK; }
  int upload(void *dev, const void *host, size_t bytes) { return copy(true, dev, host, bytes); }
  int download(void *host, const void *dev, size_t bytes) { return copy(false, host, dev, bytes); }
  int copy(bool up, void *dst, const void *src, size_t bytes) {
    w->log += up ? 'u' : 'd';
    w->queue.push_back({up, dst, src, bytes});
    w->done.push_back({up, dst, src, bytes});
    return TSDR_OK;
  }
  int wait(const char *) {
    w->log += w->stuck ? 'W' : 'w';
    if (w->stuck) return TSDR_EHIP;
    w->land();
    return TSDR_OK;
  }
  void *small_block() { return w->small; }
  void keep(void *p) { w->kept.push_back(p); }
};
using Stage = HostStageT<Recorder>;

int main() {
  std::puts("declaration order is enqueue order, every upload before every download, one fence, one wait");
  {
    World w;
    float a[4] = {1, 2, 3, 4}, b[4] = {}, c[2] = {5, 6}, d[2] = {};
    Stage st(Recorder{&w});
    void *da = st.in(0, a, sizeof a);
    void *db = st.out(1, b, sizeof b);
    void *dc = st.inout(2, c, sizeof c, true);
    void *dd = st.inout(3, d, sizeof d, false);
    EXPECT(da == w.slot[0] && db == w.slot[1] && dc == w.slot[2] && dd == w.slot[3]);
    EXPECT(w.log == "gggg");                                   // slots grown at the declaration, nothing enqueued
    EXPECT(st.begin() == TSDR_OK && w.log == "ggggfuu" && st.pending());
    w.land();                                                  // the stream runs the uploads, then "the device form"
    std::memcpy(db, da, sizeof a);
    std::memcpy(dd, dc, sizeof c);
    EXPECT(st.finish("t") == TSDR_OK && w.log == "ggggfuudddw" && !st.pending());
    EXPECT(w.done.size() == 5 && w.done[0].src == a && w.done[1].src == c && w.done[2].dst == b && w.done[3].dst == c && w.done[4].dst == d);
    EXPECT(b[3] == 4 && d[1] == 6);
  }

  std::puts("a NULL host pointer: a NULL device pointer, no slot, no record");
  {
    World w;
    float a[2] = {};
    Stage st(Recorder{&w});
    EXPECT(st.in(0, nullptr, 8) == nullptr && st.out(1, nullptr, 8) == nullptr && st.inout(2, nullptr, 8, true) == nullptr);
    st.in_to(w.slot[5], nullptr, 8);
    st.out_from(w.slot[5], nullptr, 8);
    EXPECT(st.out(3, a, sizeof a) == w.slot[3]);
    EXPECT(st.run("t") == TSDR_OK && w.log == "gfdw" && w.done.size() == 1);
  }

  std::puts("zero bytes are legal: the slot exists, nothing is copied");
  {
    World w;
    float a[1] = {};
    Stage st(Recorder{&w});
    EXPECT(st.in(0, a, 0) == w.slot[0] && st.out(1, a, 0) == w.slot[1] && st.reserve(2, 0) == w.slot[2]);
    EXPECT(st.begin() == TSDR_OK && st.finish("t") == TSDR_OK && w.log == "gggfw" && w.done.empty());
  }

  std::puts("a failed slot growth: TSDR_ENOMEM from begin(), nothing enqueued, not even the fence");
  {
    World w;
    w.fail_slot = 1;
    float a[2] = {}, b[2] = {};
    Stage st(Recorder{&w});
    EXPECT(st.in(0, a, sizeof a) != nullptr && st.out(1, b, sizeof b) == nullptr);
    EXPECT(st.begin() == TSDR_ENOMEM && w.log == "gg" && w.done.empty() && !st.pending());
    bool ran = false;   // ... and run() does not reach the device form; a device form that fails is not waited for
    EXPECT(st.run("t", [&] { ran = true; return (int)TSDR_OK; }) == TSDR_ENOMEM && !ran && w.log == "gg");
    Stage st2(Recorder{&w});
    EXPECT(st2.out(2, b, sizeof b) != nullptr && st2.run("t", [] { return (int)TSDR_EBOUNDS; }) == TSDR_EBOUNDS && w.log == "gggf");
  }

  std::puts("sub-ranges of a reserved slot follow each other, 8-byte aligned; an absent array keeps its place");
  {
    World w;
    float mag[3] = {};
    double info[2] = {};
    for (int have_mag = 0; have_mag < 2; ++have_mag) {
      Stage st(Recorder{&w});
      char *base = (char *)st.reserve(0, 16 + sizeof info);
      char *dm = (char *)st.out(0, have_mag ? mag : nullptr, sizeof mag);   // 12 bytes: the next range starts at 16
      char *di = (char *)st.out(0, info, sizeof info);
      EXPECT(base == w.slot[0] && dm == (have_mag ? base : nullptr) && di == base + 16);
      EXPECT(!dm || dm + sizeof mag <= di);
      EXPECT(st.begin() == TSDR_OK);
      for (int i = 0; i < 3; ++i) ((float *)base)[i] = 7.f;
      ((double *)(base + 16))[1] = 9.0;
      EXPECT(st.finish("t") == TSDR_OK && info[1] == 9.0 && (mag[2] == 7.f) == (have_mag == 1));
    }
    Stage st(Recorder{&w});   // past the reservation, a slot declared twice, a reservation of a declared slot: refused
    (void)st.reserve(0, 16);
    EXPECT(st.out(0, mag, 12) != nullptr && st.out(0, info, 16) == nullptr && st.begin() == TSDR_EINVAL);
    Stage st2(Recorder{&w});
    EXPECT(st2.in(1, mag, 12) != nullptr && st2.out(1, mag, 12) == nullptr && st2.begin() == TSDR_EINVAL);
    Stage st3(Recorder{&w});
    EXPECT(st3.in(1, mag, 12) != nullptr && st3.reserve(1, 64) == nullptr && st3.begin() == TSDR_EINVAL);
  }

  std::puts("a ninth entry is refused, the eight before it stay as they were");
  {
    World w;
    char h[kStageEntries + 1][8] = {};
    Stage st(Recorder{&w});
    for (int i = 0; i < kStageEntries; ++i) st.out_from(w.slot[0] + 8 * i, h[i], 8);
    EXPECT(st.begin() == TSDR_OK);
    st.out_from(w.slot[0] + 8 * kStageEntries, h[kStageEntries], 8);
    EXPECT(st.begin() == TSDR_EINVAL);
    std::memset(w.slot[0], 3, 8 * (kStageEntries + 1));
    EXPECT(st.finish("t") == TSDR_OK && w.done.size() == (size_t)kStageEntries && h[kStageEntries - 1][7] == 3 && h[kStageEntries][0] == 0);
  }

  std::puts("small results: one pinned block, 8-byte aligned pieces, 64 bytes in all");
  {
    World w;
    Stage st(Recorder{&w});
    EXPECT(st.small(8) == w.small && st.small(12) == w.small + 8 && st.small(40) == w.small + 24 && st.small(1) == nullptr);
    EXPECT(st.begin() == TSDR_EINVAL);
    Stage st2(Recorder{&w});   // the next call has the block from its start again
    EXPECT(st2.small(kStageSmall) == w.small && st2.begin() == TSDR_OK);
  }

  std::puts("temporaries: freed with the stage after a wait that succeeded ...");
  {
    World w;
    {
      Stage st(Recorder{&w});
      char *t = (char *)st.temp(4096);
      st.out_from(w.slot[0], t, 4096);
      std::memset(w.slot[0], 5, 4096);
      EXPECT(t && st.begin() == TSDR_OK && st.finish("t") == TSDR_OK && t[4095] == 5);
      EXPECT(st.temp(1) != nullptr && st.temp(1) == nullptr);   // kStageTemps of them
    }
    EXPECT(w.kept.empty());
  }

  std::puts("... and alive, on the context's list, after one that gave up: the copies land when the stage is long gone");
  {
    World w;
    char *t_down = nullptr, *t_up = nullptr;
    {
      Stage st(Recorder{&w});
      t_down = (char *)st.temp(4096);
      t_up = (char *)st.temp(100);
      std::memset(t_up, 1, 100);
      st.in_to(w.slot[1], t_up, 100);
      st.out_from(w.slot[0], t_down, 4096);
      w.stuck = true;
      EXPECT(st.begin() == TSDR_OK && st.finish("t") == TSDR_EHIP && st.pending() && w.log == "fudW" && w.queue.size() == 2);
      w.land();                 // behind finish(), the stage still in scope
    }
    EXPECT(w.kept.size() == 2 && w.kept[0] == t_down && w.kept[1] == t_up);
    w.queue = w.done;
    std::memset(w.slot[0], 9, 4096);
    w.land();                   // behind the whole call: reads t_up, writes t_down
    EXPECT(t_down[0] == 9 && t_down[4095] == 9 && w.slot[1][99] == 1);
  }

  std::puts("uploads enqueued, the call fails before finish(): the temporaries are kept as well");
  {
    World w;
    {
      Stage st(Recorder{&w});
      void *t = st.temp(64);
      std::memset(t, 2, 64);
      st.in_to(w.slot[0], t, 64);
      EXPECT(st.begin() == TSDR_OK && st.pending());
    }
    EXPECT(w.kept.size() == 1);
    w.land();
    EXPECT(w.slot[0][63] == 2);
  }

  std::printf("%d expectation(s) failed\n", failures);
  return failures ? 1 : 0;
}
