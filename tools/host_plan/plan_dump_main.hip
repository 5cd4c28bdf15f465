// Stand-alone host program (no GPU needed or touched): prints what image_plan.h:plan_images decides for every case of the
// built-in list of plan_dump.h -- one line per case: status, what is produced, and per step the profile name, grid, block, dynamic
// LDS bytes and a 64-bit FNV-1a hash over the canonical dump of the step's kernel parameters.
//   plan_dump              every case (tests/test_image_plan_host.py compares this with tests/golden/image_plans_v1.txt)
//   plan_dump --full ID    the canonical parameter dump of one case
//   plan_dump --one FMT EXACT S Y_T X_T FRAMES RASTER IMAGES CUS    the line of one IQ request given on the command line (FMT: 0 cf32,
//                          1 sc16, 2 sc8, 3 uc8; tests/test_grid_cap_host.py: the direct raster kernel's grid against its work)
//   plan_dump --table      every k_raster_fast instantiation image_plan.h:fast_instance admits (what resample.hip builds), one per line
//   plan_dump --reach      the distinct kernel instantiations a built-in sweep over plan_images met, sorted (tests/test_image_plan_host.py:
//                          for k_raster_fast the two lists are equal)
// Build, host only:  hipcc --cuda-host-only -std=c++17 -ffp-contract=off -Iinclude tools/host_plan/plan_dump_main.hip -o plan_dump
#include <cstdlib>
#include <cstring>
#include <set>

#include "../../tempestsdr.jl_amd/csrc/image_plan.h"
#include "plan_dump.h"

using namespace tsdr;

// kernel<template arguments> of a step, spelled as a demangler prints the instantiation
static const char *b(int v) { return v ? "true" : "false"; }
static std::string fast_text(int f32w, int down, int pw, int out, int vw, int rec4, int iqf) {
  plan_dump::Txt t;
  t.f("k_raster_fast<true,%s,%s,%d,%s,%d,%s,%d>", b(f32w), b(down), pw, b(out), vw, b(rec4), iqf);
  return t.s;
}
static std::string kernel_text(const ImageStep &s) {
  plan_dump::Txt t;
  switch (s.kernel) {
    case IK_FAST: return fast_text(s.f32w, s.down, s.pw, s.out, s.vw, s.rec4, s.iqf);
    case IK_FAST4: t.f("k_raster_fast4<%d,%d>", s.iqf, s.pw); break;
    case IK_TILE: t.f("k_raster_tile<%s,%s>", b(s.cplx), b(s.down)); break;
    case IK_DIRECT: t.f("k_raster_direct<%s>", b(s.cplx)); break;
    case IK_DOWN: t.f("k_down_fused<%s,%d,%d,%d,%d>", b(s.cplx), s.mode, s.sums, s.ld, s.iqf); break;
    case IK_SHEAR: t.f("k_raster_shear<%s>", b(s.shear)); break;
    case IK_RESIZE2D: t.f("k_resize2d"); break;
    default: break;
  }
  return t.s;
}

static ImagePlan plan_of(const plan_dump::Case &c) {
  PlanOpts o;
  o.raster_rec4 = c.raster_rec4; o.raster_v4 = c.raster_v4; o.raster_split = c.raster_split; o.fast_walk_only = c.fast_walk_only;
  o.down_spp_max_pct = c.down_spp_max_pct; o.down_xcd = c.down_xcd; o.cu_count = c.cu_count;
  ImageReq r;
  r.cplx = c.cplx; r.iqf = IqFmt{c.fmt, c.scale}; r.precision = c.exact ? TSDR_EXACT : TSDR_FAST;
  r.S = r.in_stride = (size_t)c.S; r.y_t = c.y_t; r.x_t = c.x_t; r.h_out = c.h_out; r.w_out = c.w_out; r.frames = c.frames;
  r.raster = c.raster != 0; r.images = c.images != 0; r.sums = c.sums != 0;
  r.raster_addr = c.raster ? (uintptr_t)0x7f0010000000ull + c.raster_addr_low : 0;
  r.raster_stride = (size_t)c.y_t * (size_t)c.x_t;
  return plan_images(o, r);
}

static plan_dump::Outcome run(const plan_dump::Case &c) {
  const ImagePlan pl = plan_of(c);
  plan_dump::Outcome out;
  out.status = pl.status; out.err = pl.err;
  out.raster = pl.raster; out.images = pl.images; out.fallback = pl.fallback; out.ws_raster = pl.ws_raster;
  out.ncp = pl.sums.ncp; out.nrp = pl.sums.nrp;
  for (int i = 0; i < pl.nsteps; ++i) {
    const ImageStep &s = pl.step[i];
    plan_dump::Launch l;
    l.name = s.name; l.kernel = kernel_text(s); l.block = s.block; l.lds = s.lds;
    if (s.kernel == IK_FAST || s.kernel == IK_FAST4 || s.kernel == IK_TILE) l.note = plan_dump::note(s.q);
    if (s.kernel == IK_DOWN) l.note = plan_dump::note(s.dq);
    for (int k = 0; k < 3; ++k) l.grid[k] = s.grid[k];
    plan_dump::Txt t;
    const bool sums = s.sums != 0;   // the launch sets the parameters' proj / keys pointers exactly then
    switch (s.kernel) {
      case IK_FAST: case IK_FAST4: plan_dump::dump(t, s.q, sums, sums); plan_dump::dump(t, s.fa); plan_dump::dump(t, s.fi); break;
      case IK_TILE: case IK_DIRECT: plan_dump::dump(t, s.q, sums, sums); break;
      case IK_DOWN: plan_dump::dump(t, s.dq, sums, sums, s.lds_main); break;
      case IK_SHEAR: plan_dump::dump(t, s.sq); break;
      case IK_RESIZE2D: plan_dump::dump_resize(t, s.rs[0], s.rs[1], s.rs[2], s.rs[3]); break;
      default: break;
    }
    l.params = t.s;
    out.steps.push_back(l);
  }
  return out;
}

// --table: fast_instance over a box that holds every value a template argument can take (and some it cannot)
static void print_table() {
  std::set<std::string> names;
  for (int f32w = 0; f32w < 2; ++f32w) for (int down = 0; down < 2; ++down) for (int pw = 0; pw <= 64; ++pw) for (int out = 0; out < 2; ++out)
    for (int vw = 0; vw <= 4; ++vw) for (int rec4 = 0; rec4 < 2; ++rec4) for (int iqf = 0; iqf <= IQF_UC8; ++iqf)
      if (fast_instance(f32w, down, pw, out, vw, rec4, iqf)) names.insert(fast_text(f32w, down, pw, out, vw, rec4, iqf));
  for (const std::string &n : names) std::puts(n.c_str());
}

// --reach: raster sizes around every threshold of the planner (2, 64 / 128 lines, 128 / 256 pixels, 128 tiles, 2P = 2^24), sample
// ratios across every tile width of the three staging budgets, five output sizes, and every value of the request (the four IQ
// formats and real input, both precisions, raster / images / sums wanted) and of the options that plan_images reads
static void print_reach() {
  static const int ys[] = {2, 20, 100, 127, 128, 200, 640, 1125, 2300, 17000}, xs[] = {2, 30, 255, 256, 300, 832, 2576, 4500, 17000};
  static const double ratios[] = {0.05, 0.115, 0.3, 0.45, 0.6, 0.7, 1.0, 1.15, 1.4, 2.0, 2.8, 4.0, 6.0, 10.0, 14.0, 20.0, 80.0};
  static const int outs[][2] = {{600, 800}, {100, 150}, {64, 64}, {1125, 2576}, {1200, 1600}};
  struct Opt { int rec4, v4, split, walk; };
  static const Opt opts[] = {{-1, 0, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 0}, {-1, 0, 0, 1}, {0, 0, 0, 1}, {-1, 1, 0, 0}, {-1, 32, 0, 0}, {-1, 0, 1, 0}, {-1, 0, 2, 0}};
  std::set<std::string> names;
  for (int y : ys) for (int x : xs) for (double ratio : ratios) for (const auto &hw : outs) for (const Opt &op : opts)
    for (int fmt = 0; fmt < 5; ++fmt) for (int bits = 0; bits < 16; ++bits) {   // (fmt 4: real samples)
      plan_dump::Case c;
      c.y_t = y; c.x_t = x; c.S = (unsigned long long)(ratio * (double)y * (double)x); c.h_out = hw[0]; c.w_out = hw[1];
      c.raster_rec4 = op.rec4; c.raster_v4 = op.v4; c.raster_split = op.split; c.fast_walk_only = op.walk;
      c.cplx = fmt < 4; c.fmt = c.cplx ? fmt : 0; c.scale = c.cplx ? plan_dump::fmt_scale(fmt) : 1.0f;
      c.exact = bits & 1; c.raster = (bits >> 1) & 1; c.images = (bits >> 2) & 1; c.sums = (bits >> 3) & 1;
      if ((!c.images && !c.raster) || (!c.cplx && !c.exact)) continue;
      const ImagePlan pl = plan_of(c);
      for (int i = 0; i < pl.nsteps; ++i) names.insert(kernel_text(pl.step[i]));
    }
  for (const std::string &n : names) std::puts(n.c_str());
}

int main(int argc, char **argv) {
  if (argc == 2 && !std::strcmp(argv[1], "--table")) { print_table(); return 0; }
  if (argc == 2 && !std::strcmp(argv[1], "--reach")) { print_reach(); return 0; }
  if (argc == 11 && !std::strcmp(argv[1], "--one")) {
    plan_dump::Case c;
    c.id = "one"; c.cplx = 1; c.fmt = std::atoi(argv[2]); c.scale = c.fmt ? 1.0f / 128.0f : 1.0f; c.exact = std::atoi(argv[3]);
    c.S = std::strtoull(argv[4], nullptr, 10); c.y_t = std::atoi(argv[5]); c.x_t = std::atoi(argv[6]); c.frames = std::atoi(argv[7]);
    c.raster = std::atoi(argv[8]); c.images = std::atoi(argv[9]); c.cu_count = std::atoi(argv[10]);
    std::puts(plan_dump::line(c.id.c_str(), run(c)).c_str());
    return 0;
  }
  const char *want = (argc == 3 && !std::strcmp(argv[1], "--full")) ? argv[2] : nullptr;
  if (argc != 1 && !want) { std::fprintf(stderr, "usage: %s [--table | --reach | --full ID | --one FMT EXACT S Y_T X_T FRAMES RASTER IMAGES CUS]\n", argv[0]); return 2; }
  bool found = false;
  for (const plan_dump::Case &c : plan_dump::cases()) {
    if (want && c.id != want) continue;
    found = true;
    const plan_dump::Outcome o = run(c);
    if (want) std::fputs(plan_dump::full(c.id.c_str(), o).c_str(), stdout);
    else std::puts(plan_dump::line(c.id.c_str(), o).c_str());
  }
  if (want && !found) { std::fprintf(stderr, "no case %s\n", want); return 1; }
  return 0;
}
