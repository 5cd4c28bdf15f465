// Stand-alone host program (no GPU needed or touched): prints what image_plan.h:plan_images decides for every case of the
// built-in list of plan_dump.h -- one line per case: status, what is produced, and per step the profile name, grid, block, dynamic
// LDS bytes and a 64-bit FNV-1a hash over the canonical dump of the step's kernel parameters.
//   plan_dump              every case (tests/test_image_plan_host.py compares this with tests/golden/image_plans_v1.txt)
//   plan_dump --full ID    the canonical parameter dump of one case
//   plan_dump --one FMT EXACT S Y_T X_T FRAMES RASTER IMAGES CUS    the line of one IQ request given on the command line (FMT: 0 cf32,
//                          1 sc16, 2 sc8, 3 uc8; tests/test_grid_cap_host.py: the direct raster kernel's grid against its work)
// Build, host only:  hipcc --cuda-host-only -std=c++17 -ffp-contract=off -Iinclude tools/host_plan/plan_dump_main.hip -o plan_dump
#include <cstdlib>
#include <cstring>

#include "../../tempestsdr.jl_amd/csrc/image_plan.h"
#include "plan_dump.h"

using namespace tsdr;

// kernel<template arguments> of a step, spelled as a demangler prints the instantiation
static std::string kernel_text(const ImageStep &s) {
  plan_dump::Txt t;
  auto b = [](int v) { return v ? "true" : "false"; };
  switch (s.kernel) {
    case IK_FAST: t.f("k_raster_fast<true,%s,%s,%d,%s,%d,%s,%d>", b(s.f32w), b(s.down), s.pw, b(s.out), s.vw, b(s.rec4), s.iqf); break;
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

static plan_dump::Outcome run(const plan_dump::Case &c) {
  PlanOpts o;
  o.raster_rec4 = c.raster_rec4; o.raster_v4 = c.raster_v4; o.raster_split = c.raster_split; o.fast_walk_only = c.fast_walk_only;
  o.down_spp_max_pct = c.down_spp_max_pct; o.down_xcd = c.down_xcd; o.cu_count = c.cu_count;
  ImageReq r;
  r.cplx = c.cplx; r.iqf = IqFmt{c.fmt, c.scale}; r.precision = c.exact ? TSDR_EXACT : TSDR_FAST;
  r.S = r.in_stride = (size_t)c.S; r.y_t = c.y_t; r.x_t = c.x_t; r.h_out = c.h_out; r.w_out = c.w_out; r.frames = c.frames;
  r.raster = c.raster != 0; r.images = c.images != 0; r.sums = c.sums != 0;
  r.raster_addr = c.raster ? (uintptr_t)0x7f0010000000ull + c.raster_addr_low : 0;
  r.raster_stride = (size_t)c.y_t * (size_t)c.x_t;
  const ImagePlan pl = plan_images(o, r);
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

int main(int argc, char **argv) {
  if (argc == 11 && !std::strcmp(argv[1], "--one")) {
    plan_dump::Case c;
    c.id = "one"; c.cplx = 1; c.fmt = std::atoi(argv[2]); c.scale = c.fmt ? 1.0f / 128.0f : 1.0f; c.exact = std::atoi(argv[3]);
    c.S = std::strtoull(argv[4], nullptr, 10); c.y_t = std::atoi(argv[5]); c.x_t = std::atoi(argv[6]); c.frames = std::atoi(argv[7]);
    c.raster = std::atoi(argv[8]); c.images = std::atoi(argv[9]); c.cu_count = std::atoi(argv[10]);
    std::puts(plan_dump::line(c.id.c_str(), run(c)).c_str());
    return 0;
  }
  const char *want = (argc == 3 && !std::strcmp(argv[1], "--full")) ? argv[2] : nullptr;
  if (argc != 1 && !want) { std::fprintf(stderr, "usage: %s [--full ID | --one FMT EXACT S Y_T X_T FRAMES RASTER IMAGES CUS]\n", argv[0]); return 2; }
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
