// Stand-alone host program (no GPU needed or touched): prints what fft_plan.h decides for every case of the built-in list of
// fft_plan_dump.h -- one line per case: status (or the error text), the WS_FFT_B bytes, and per step the profile name, the kernel
// instantiation, grid, block, dynamic LDS bytes, the buffers read and written as roles, the tables needed, and a 64-bit FNV-1a
// hash over the canonical dump of the step's kernel parameters.
//   fft_plan_dump              every case (tests/test_fft_plan_host.py compares this with tests/golden/fft_plans_v1.txt)
//   fft_plan_dump --full ID    the canonical parameter dump of one case
//   fft_plan_dump --rows WHAT KIND N ROWS CUS    one whole-row request (WHAT: welch | store | wfall; KIND: SIG_* as a number) on a device of
//                              CUS compute units: the step's profile name, kernel, grid, and the tiles its workgroups walk
//                              (tests/test_grid_cap_host.py: ntiles > grid is a tile loop that takes a second trip)
// Build, host only:  hipcc --cuda-host-only -std=c++17 -ffp-contract=off -Iinclude tools/host_plan/fft_plan_dump_main.hip -o fft_plan_dump
#include <cstdlib>
#include <cstring>

#include "../../tempestsdr.jl_amd/csrc/fft_plan.h"
#include "fft_plan_dump.h"

using namespace tsdr;

// kernel<template arguments> of a step, spelled as a demangler prints the instantiation: the same entry lists as the
// geometry tables and the kernel-pointer tables, so index i names entry i
#define TSDR_X(...) #__VA_ARGS__,
static const char *const kMix2Args[] = {TSDR_MIX2_LIST(TSDR_X)};
static const char *const kMix3Args[] = {TSDR_MIX3_LIST(TSDR_X) TSDR_WELCH3_LIST(TSDR_X)};
static const char *const kMidArgs[] = {TSDR_MID_LIST(TSDR_X) TSDR_MID3_LIST(TSDR_X)};
#undef TSDR_X
static std::string squeeze(const char *s) { std::string o; for (; *s; ++s) if (*s != ' ') o += *s; return o; }
static std::string kernel_text(const FftStep &s) {
  fft_plan_dump::Txt t;
  switch (s.kernel) {
    case FK_PASS: t.f("k_fft_pass<%d,%d>", s.inst, s.mode); break;
    case FK_MIX: t.f("k_fft_mix"); break;
    case FK_MIX2: t.f("k_fft_mix2<%s,%d>", squeeze(kMix2Args[s.inst]).c_str(), s.mode); break;
    case FK_MIX3: t.f("k_fft_mix3<%s,%d>", squeeze(kMix3Args[s.inst]).c_str(), s.mode); break;
    case FK_MID: t.f("k_fft_mid<%s>", squeeze(kMidArgs[s.inst]).c_str()); break;
    case FK_MID3: t.f("k_fft_mid3<%s>", squeeze(kMidArgs[s.inst]).c_str()); break;
    default: break;
  }
  return t.s;
}
static const char *role(int b) { return b == FB_IN ? "in" : b == FB_OUT ? "out" : b == FB_WORK ? "work" : b == FB_MID ? "mid" : "-"; }

static fft_plan_dump::Outcome run(const fft_plan_dump::Case &c) {
  using namespace fft_plan_dump;
  FftOpts o;
  o.no_mix2 = c.no_mix2; o.big = c.big; o.cu_count = c.cu_count;
  const FftEpilogue e = epilogue(c);
  FftReq q;   // (pointers: any non-null value)
  q.in = reinterpret_cast<const float2 *>(0x10000000ull); q.out = reinterpret_cast<float2 *>(0x20000000ull);
  q.n = (size_t)c.n; q.batch = (size_t)c.batch; q.dir = c.dir; q.scale = c.scale;
  q.src_mode = c.src_mode; q.src_n = (size_t)c.src_n; q.src_scale = c.src_scale; q.keep = (size_t)c.keep;
  if (c.aux) q.src_aux = reinterpret_cast<const float2 *>(0x48000000ull);
  if (c.epi) q.epi = &e;
  FftPlan pl;
  if (c.what == W_FFT) plan_fft(pl, q, o);
  else if (c.what == W_AUTOCORR) plan_autocorr(pl, q, o);
  else {
    RowsReq r;
    r.what = c.what == W_WELCH ? ROWS_TO_WELCH : c.what == W_STORE ? ROWS_TO_STORE : ROWS_TO_WATERFALL;
    r.kind = c.sig_kind; r.sig_scale = c.src_scale; r.N = (size_t)c.n; r.rows = (size_t)c.batch; r.dir = c.dir; r.scale = c.scale;
    if (c.what == W_WELCH) r.acc = reinterpret_cast<float *>(0x52000000ull);
    if (c.what == W_STORE) r.rows_out = q.out;
    if (c.what == W_WATERFALL) r.wf = reinterpret_cast<double *>(0x54000000ull);
    plan_rows(pl, r, o);
  }
  Outcome out;
  out.status = pl.status; out.err = pl.err; out.copy = pl.copy_bytes != 0; out.work_bytes = pl.work_bytes;
  for (int i = 0; i < pl.nsteps; ++i) {
    const FftStep &s = pl.step[i];
    Launch l;
    l.name = s.name; l.kernel = kernel_text(s); l.grid = s.grid; l.block = s.block; l.lds = s.lds;
    l.bufs = std::string(role(s.src)) + ">" + role(s.dst);
    Txt tb;
    if (s.kernel == FK_PASS) tb.f("tw4096");
    if (s.twg_R) tb.f("%stwg(%u,%u)", tb.s.empty() ? "" : "+", s.twg_R, s.twg_Rn);
    if (s.opt_in) tb.f("%soptin", tb.s.empty() ? "" : "+");
    l.tables = tb.s.empty() ? "-" : tb.s;
    Txt t;
    if (s.kernel == FK_PASS) dump(t, s.p.pass);
    else if (s.kernel == FK_MID || s.kernel == FK_MID3) dump(t, s.p.mid);
    else {
      MixDesc d = s.p.mix;   // as launched: the table pointer is set exactly when the step names the table
      d.twg = s.twg_R ? reinterpret_cast<const float2 *>(0x70000000ull) : nullptr;
      dump(t, d);
    }
    l.params = t.s;
    out.steps.push_back(l);
  }
  return out;
}

// plan_rows for one request given on the command line
static int rows_query(char **a) {
  using namespace fft_plan_dump;
  Case c;
  c.what = !std::strcmp(a[0], "welch") ? W_WELCH : !std::strcmp(a[0], "store") ? W_STORE : !std::strcmp(a[0], "wfall") ? W_WATERFALL : -1;
  if (c.what < 0) { std::fprintf(stderr, "--rows: WHAT is welch, store or wfall\n"); return 2; }
  c.sig_kind = std::atoi(a[1]); c.n = std::strtoull(a[2], nullptr, 10); c.batch = std::strtoull(a[3], nullptr, 10); c.cu_count = std::atoi(a[4]);
  c.src_scale = c.sig_kind >= 2 ? 1.0f / 128.0f : 1.0f;
  FftOpts o;
  o.cu_count = c.cu_count;
  RowsReq r;
  r.what = c.what == W_WELCH ? ROWS_TO_WELCH : c.what == W_STORE ? ROWS_TO_STORE : ROWS_TO_WATERFALL;
  r.kind = c.sig_kind; r.sig_scale = c.src_scale; r.N = (size_t)c.n; r.rows = (size_t)c.batch;
  r.acc = reinterpret_cast<float *>(0x52000000ull); r.rows_out = reinterpret_cast<float2 *>(0x20000000ull); r.wf = reinterpret_cast<double *>(0x54000000ull);
  FftPlan pl;
  plan_rows(pl, r, o);
  if (pl.status) { std::printf("status=%d err=\"%s\"\n", pl.status, pl.err); return 0; }
  if (pl.nsteps != 1) { std::printf("declined\n"); return 0; }
  const FftStep &s = pl.step[0];
  const unsigned long long per_tile = 1ull << s.p.mix.logT;
  std::printf("%s %s grid=%u block=%u rows_per_tile=%llu ntiles=%llu\n", s.name, kernel_text(s).c_str(), s.grid, s.block, per_tile,
              (c.batch + per_tile - 1) / per_tile);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 7 && !std::strcmp(argv[1], "--rows")) return rows_query(argv + 2);
  const char *want = (argc == 3 && !std::strcmp(argv[1], "--full")) ? argv[2] : nullptr;
  if (argc != 1 && !want) { std::fprintf(stderr, "usage: %s [--full ID | --rows WHAT KIND N ROWS CUS]\n", argv[0]); return 2; }
  bool found = false;
  for (const fft_plan_dump::Case &c : fft_plan_dump::cases()) {
    if (want && c.id != want) continue;
    found = true;
    const fft_plan_dump::Outcome o = run(c);
    if (want) std::fputs(fft_plan_dump::full(c.id.c_str(), o).c_str(), stdout);
    else std::puts(fft_plan_dump::line(c.id.c_str(), o).c_str());
  }
  if (want && !found) { std::fprintf(stderr, "no case %s\n", want); return 1; }
  return 0;
}
