// plan_dump.h -- the case list and the canonical text of tools/host_plan/plan_dump_main.hip.
//
// Everything here is plain host C++ over the parameter structs of the image kernels (TileParams, FastAx, FastInc, DownParams,
// ShearParams: they must be declared before this file is included).  It knows nothing of how a plan is made, so the same file
// formats the launches of an older revision whose launch macro was replaced by a recorder: that is how the fixture
// tests/golden/image_plans_v1.txt was made (NOTEBOOK.md, "image plans").
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace plan_dump {

// ---- canonical dumps: every field in declaration order; integers in decimal, floats / doubles as %a, pointers as 0 / 1 ("will be set")
struct Txt {
  std::string s;
  void f(const char *fmt, ...) {
    char b[256];
    va_list ap; va_start(ap, fmt); std::vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    s += b;
  }
};
inline void dump(Txt &t, const tsdr::RsAxis &a, const char *n) { t.f("%s.sf=%a %s.off=%a %s.n_in=%a\n", n, a.sf, n, a.off, n, a.n_in); }
inline void dump(Txt &t, const tsdr::IqFmt &q) { t.f("iqf.kind=%d iqf.scale=%a\n", q.kind, (double)q.scale); }
inline void dump(Txt &t, const tsdr::TileParams &q, bool proj, bool keys) {
  t.f("S=%u y_t=%d x_t=%d TP=%d W=%d tiles_l=%d tiles_p=%d frames=%d own_l=%d own_p=%d h_out=%d w_out=%d NR=%d NC=%d\n", q.S, q.y_t, q.x_t,
      q.TP, q.W, q.tiles_l, q.tiles_p, q.frames, q.own_l, q.own_p, q.h_out, q.w_out, q.NR, q.NC);
  t.f("lpl_log=%d cs=%d xcd_group=%d xcd_group_log=%d inv_tiles_p=%a\n", q.lpl_log, q.cs, q.xcd_group, q.xcd_group_log, (double)q.inv_tiles_p);
  dump(t, q.ax, "ax"); dump(t, q.ay, "ay"); dump(t, q.axx, "axx");
  t.f("inv_sfy=%a inv_sfx=%a proj=%d proj_stride=%zu keys=%d\n", q.inv_sfy, q.inv_sfx, proj ? 1 : 0, q.proj_stride, keys ? 1 : 0);
  dump(t, q.iqf);
}
inline void dump(Txt &t, const tsdr::FastAx &f) {
  t.f("fa.S=%u fa.P=%u fa.D=%u fa.qstep=%u fa.rstep=%u fa.invDd=%a\n", f.S, f.P, f.D, f.qstep, f.rstep, f.invDd);
}
inline void dump(Txt &t, const tsdr::FastInc &n) {
  t.f("fi.qL=%u fi.rL=%u fi.qTL=%u fi.rTL=%u fi.qTP=%u fi.rTP=%u fi.k00=%d fi.r00=%u fi.invD=%a\n", n.qL, n.rL, n.qTL, n.rTL, n.qTP, n.rTP,
      n.k00, n.r00, (double)n.invD);
}
inline void dump(Txt &t, const tsdr::DownParams &q, bool proj, bool keys, size_t lds_main) {
  t.f("S=%u y_t=%d x_t=%d h_out=%d w_out=%d TC=%d NL=%d W=%d tiles_c=%d lpl_log=%d ld16=%d sparse=%d xcd_tpx=%d xcd_tiles=%d\n", q.S, q.y_t,
      q.x_t, q.h_out, q.w_out, q.TC, q.NL, q.W, q.tiles_c, q.lpl_log, q.ld16, q.sparse, q.xcd_tpx, q.xcd_tiles);
  t.f("proj=%d proj_stride=%zu keys=%d\n", proj ? 1 : 0, q.proj_stride, keys ? 1 : 0);
  dump(t, q.iqf);
  t.f("lds_main=%zu\n", lds_main);
}
inline void dump(Txt &t, const tsdr::ShearParams &q) {
  t.f("S=%u y_t=%d x_t=%d frames=%d W=%d rows=%d tiles_p=%d tiles_l=%d c=%d out_mis=%u sf=%a XA=%lld XB=%lld inv_W=%a\n", q.S, q.y_t, q.x_t,
      q.frames, q.W, q.rows, q.tiles_p, q.tiles_l, q.c, q.out_mis, q.sf, q.XA, q.XB, (double)q.inv_W);
}
inline void dump_resize(Txt &t, int h_in, int w_in, int h_out, int w_out) { t.f("h_in=%d w_in=%d h_out=%d w_out=%d\n", h_in, w_in, h_out, w_out); }

// what the one-line form shows of the parameters: the tile width of the walk kernels, the tap kernel's tile and staging
inline std::string note(const tsdr::TileParams &q) { Txt t; t.f("TP=%d ", q.TP); return t.s; }
inline std::string note(const tsdr::DownParams &q) { Txt t; t.f("TC=%d sparse=%d ld16=%d ", q.TC, q.sparse, q.ld16); return t.s; }

inline unsigned long long fnv1a(const std::string &s) {
  unsigned long long h = 0xcbf29ce484222325ull;
  for (unsigned char c : s) { h ^= c; h *= 0x100000001b3ull; }
  return h;
}

// ---- one launch and one case, as text ------------------------------------------------------------------------
struct Launch {
  std::string name, kernel, note, params;   // profile name, kernel<template arguments>, a few telling parameters, canonical dump of all of them
  unsigned grid[3], block;
  size_t lds;
};
struct Outcome {
  int status = 0;
  std::string err;
  std::vector<Launch> steps;    // with `fallback`: the last two are what ONE frame launches
  bool raster = false, images = false, fallback = false;
  size_t ws_raster = 0;
  int ncp = 0, nrp = 0;
};

inline std::string line(const char *id, const Outcome &o) {
  Txt t;
  t.f("%s status=%d", id, o.status);
  if (o.status) { t.f(" err=\"%s\"", o.err.c_str()); return t.s; }
  t.f(" raster=%d images=%d ncp=%d nrp=%d", o.raster ? 1 : 0, o.images ? 1 : 0, o.ncp, o.nrp);
  if (o.fallback) t.f(" fallback ws_raster=%zu", o.ws_raster);
  for (const Launch &l : o.steps)
    t.f(" | %s %s %sgrid=%u,%u,%u block=%u lds=%zu hash=%016llx", l.name.c_str(), l.kernel.c_str(), l.note.c_str(), l.grid[0], l.grid[1], l.grid[2],
        l.block, l.lds, fnv1a(l.params));
  return t.s;
}
inline std::string full(const char *id, const Outcome &o) {
  std::string s = line(id, o) + "\n";
  for (const Launch &l : o.steps) s += "--- " + l.name + " " + l.kernel + "\n" + l.params;
  return s;
}

// ---- the case list ----------------------------------------------------------------------------------------------
enum { FMT_CF32 = 0, FMT_SC16 = 1, FMT_SC8 = 2, FMT_UC8 = 3 };   // = TSDR_IQ_* / IQK_*
struct Case {
  std::string id;
  // options (tsdr_set_option names), at their defaults
  int raster_rec4 = -1, raster_v4 = 0, raster_split = 0, fast_walk_only = 0, down_spp_max_pct = 200, down_xcd = 1, cu_count = 256;
  // request
  int cplx = 1, fmt = FMT_CF32;
  float scale = 1.0f;
  int exact = 0;
  unsigned long long S = 0;
  int y_t = 0, x_t = 0, h_out = 600, w_out = 800, frames = 2;
  int raster = 0, images = 1, sums = 1;
  unsigned raster_addr_low = 0;   // low bits of the raster pointer (route "raster_split" reads them)
};

inline const char *fmt_name(int f) { return f == FMT_SC16 ? "sc16" : f == FMT_SC8 ? "sc8" : f == FMT_UC8 ? "uc8" : "cf32"; }
inline float fmt_scale(int f) { return f == FMT_SC16 ? 1.0f / 32768.0f : f == FMT_CF32 ? 1.0f : 1.0f / 128.0f; }

struct Lcg {   // (Knuth's MMIX constants; the high bits are the random ones)
  unsigned long long x;
  unsigned next(unsigned n) { x = x * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)((x >> 33) % n); }
};

inline std::vector<Case> cases() {
  std::vector<Case> v;
  auto add = [&](Case c, const std::string &id) { c.id = id; c.scale = c.cplx ? fmt_scale(c.fmt) : 1.0f; v.push_back(c); };
  auto geo = [](unsigned long long S, int y, int x, int frames) { Case c; c.S = S; c.y_t = y; c.x_t = x; c.frames = frames; return c; };
  struct Wl { const char *n; unsigned long long S; int y, x; };
  const Wl wl[] = {{"C2", 333333, 1125, 2576}, {"C3", 3333333, 1125, 2576}, {"C5", 833333, 2250, 4400}, {"C2A", 333333, 1152, 2576}};   // synth.WORKLOADS, S = round(Fs / fv)
  char b[128];
  // 1  the workloads: raster or not, FAST or EXACT, every IQ format, sums wanted or not
  for (const Wl &w : wl)
    for (int ras = 0; ras < 2; ++ras)
      for (int ex = 0; ex < 2; ++ex)
        for (int f = 0; f < 4; ++f)
          for (int sm = 0; sm < 2; ++sm) {
            Case c = geo(w.S, w.y, w.x, 30);
            c.raster = ras; c.exact = ex; c.fmt = f; c.sums = sm; c.raster_addr_low = 0;
            std::snprintf(b, sizeof b, "wl-%s-%s-%s-%s-%s", w.n, ras ? "ras" : "nor", ex ? "exact" : "fast", fmt_name(f), sm ? "sums" : "nos");
            add(c, b);
          }
  // 2  each non-default option value
  struct Opt { const char *n; int Case::*p; int val; };
  const Opt opts[] = {{"rec4=0", &Case::raster_rec4, 0}, {"v4=1", &Case::raster_v4, 1}, {"v4=32", &Case::raster_v4, 32}, {"split=1", &Case::raster_split, 1},
                      {"split=2", &Case::raster_split, 2}, {"walk=1", &Case::fast_walk_only, 1}, {"xcd=0", &Case::down_xcd, 0}, {"spp=50", &Case::down_spp_max_pct, 50}};
  for (const Opt &o : opts)
    for (const Wl &w : wl)
      for (int ras = 0; ras < 2; ++ras)
        for (int f = 0; f < 2; ++f)
          for (unsigned mis = 0; mis < 2; ++mis) {
            if (mis && !(ras && o.p == &Case::raster_split)) continue;   // a second raster address only where it is read
            Case c = geo(w.S, w.y, w.x, 30);
            c.*(o.p) = o.val; c.raster = ras; c.fmt = f; c.raster_addr_low = mis ? 0x44 : 0;
            std::snprintf(b, sizeof b, "opt-%s-%s-%s-%s%s", o.n, w.n, ras ? "ras" : "nor", fmt_name(f), mis ? "-mis" : "");
            add(c, b);
          }
  // 3  real input: tsdr_sig_to_image (rasters alone, EXACT)
  const Wl real[] = {{"c2", 333333, 1125, 2576}, {"small", 6000, 200, 300}, {"direct", 40000, 20, 30}, {"same", 600, 20, 30}, {"up", 100, 64, 128},
                     {"line", 5000, 1, 3000}, {"odd", 77777, 333, 777}, {"wide", 9000000, 300, 400}};
  for (const Wl &w : real) {
    Case c = geo(w.S, w.y, w.x, 1);
    c.cplx = 0; c.exact = 1; c.raster = 1; c.images = 0; c.sums = 0; c.h_out = c.w_out = 0;
    add(c, std::string("real-") + w.n);
  }
  for (int ras = 0; ras < 2; ++ras) {   // ... and with images: no entry point asks for them, the planner serves them
    Case c = geo(333333, 1125, 2576, 2);
    c.cplx = 0; c.exact = 1; c.raster = ras; c.sums = 0;
    add(c, ras ? "real-images-ras" : "real-images-nor");
  }
  // 4  the geometries of tests/test_image_plan_gpu.py (two frames each; the smallest shapes that still choose each route)
  {
    Case c = geo(53248, 640, 832, 2); c.raster = 1; add(c, "gpu-walk-raster");            // S = 0.1 P: the fused walk
    c.raster = 0; add(c, "gpu-taps-sums");                                                 // ... the tap kernel with sums
    c.sums = 0; add(c, "gpu-taps");
    c = geo(612352, 640, 832, 2); add(c, "gpu-taps-ld16");                                 // S = 1.15 P (C3's ratio): 16 loads in flight
    c = geo(6000, 200, 300, 2); c.raster = 1; add(c, "gpu-walk-nonfused");
    c = geo(40000, 20, 30, 2); c.raster = 1; add(c, "gpu-direct");                         // S / P = 66.7
    c = geo(53248, 640, 832, 2); c.raster = 1; c.exact = 1; add(c, "gpu-exact-raster");
    c.raster = 0; add(c, "gpu-exact-taps");
    c = geo(53248, 640, 832, 2); c.fast_walk_only = 1; add(c, "gpu-walk-only");            // the walk without a raster to write
    c = geo(54080, 650, 832, 2); c.raster = 1; c.raster_split = 1; add(c, "gpu-shear");    // y_t mod 32 != 0: sheared at any address
    c = geo(1000000, 20, 30, 2); c.sums = 0; add(c, "gpu-fallback");                       // 1667 samples per pixel: no tap tile fits
    c = geo(6000, 200, 300, 1); c.cplx = 0; c.exact = 1; c.raster = 1; c.images = 0; c.sums = 0; c.h_out = c.w_out = 0; add(c, "gpu-real-tile");
  }
  // 5  the error texts
  {
    Case c = geo(1000, 0, 30, 2); add(c, "err-geom-positive");
    c = geo(1ull << 31, 1125, 2576, 2); add(c, "err-geom-2^31");
    c = geo(1, 20, 30, 2); add(c, "err-geom-2-samples");
    c = geo(1000, 20, 30, 2); c.exact = 1; c.h_out = 0; add(c, "err-output-size");
    c = geo(1000, 1, 300, 2); add(c, "err-2x2");
    c = geo(333333, 1125, 2576, 30000); c.raster = 1; add(c, "err-too-many-tiles");
    c.exact = 1; add(c, "err-too-many-tiles-exact");
  }
  // 6  a seeded sweep: y_t in 2..2300, x_t in 2..4500, S / P log-uniform over 0.02..80 (0.02 * 2^(k/16), k < 192: the sixteen
  //    steps of an octave from a table, so that no library function decides a sample count)
  static const double step16[16] = {1.0, 1.0442737824274138, 1.0905077326652577, 1.1387886347566916, 1.189207115002721, 1.2418578120734840,
                                    1.2968395546510096, 1.3542555469368927, 1.4142135623730951, 1.4768261459394993, 1.5422108254079407,
                                    1.6104903319492543, 1.6817928305074290, 1.7562521603732995, 1.8340080864093424, 1.9152065613971474};
  Lcg g{20261018ull};
  const int total = 590;
  for (int i = 0; (int)v.size() < total; ++i) {
    Case c;
    c.y_t = 2 + (int)g.next(2299); c.x_t = 2 + (int)g.next(4499);
    if (i == 0) { c.y_t = 2300; c.x_t = 4500; }   // 2P >= 2^24: the 64-bit walk advance
    const unsigned k = g.next(192);
    double ratio = 0.02 * step16[k & 15];
    for (unsigned o2 = 0; o2 < (k >> 4); ++o2) ratio *= 2.0;
    const double P = (double)c.y_t * (double)c.x_t;
    c.S = (unsigned long long)(ratio * P);
    if (c.S < 2) c.S = 2;
    c.frames = 1 + (int)g.next(4);
    c.raster = (int)g.next(2); c.exact = g.next(4) == 0; c.fmt = (int)g.next(4); c.sums = g.next(4) != 0;
    const unsigned sp = g.next(8);
    c.raster_split = sp == 0 ? 1 : sp == 1 ? 2 : 0;
    c.raster_addr_low = 4u * g.next(32);             // misaligned raster addresses (multiples of one float)
    if (i == 1) { c.raster = 1; c.exact = 0; c.fmt = FMT_CF32; c.raster_split = 1; c.raster_addr_low = 0x24; c.y_t = 1125; c.x_t = 2576; c.S = 333333; }
    std::snprintf(b, sizeof b, "sweep-%03d", i);
    add(c, b);
  }
  // 7  the geometries of tests/test_raster_instances_gpu.py: one per class of k_raster_fast instantiation (image_plan.h:
  //    fast_instance), two frames each, the smallest rasters that produce the class
  {
    // the raster-only walk (200 x 300 is smaller than the 600 x 800 image: nothing to downgrade) at each tile width: TP = 4 .. 128
    // from 10 .. 0.1 samples per raster pixel; one of them less than 128 lines high (one wavefront per workgroup column)
    const Wl ras[] = {{"pw1", 600000, 200, 300}, {"pw2", 240000, 200, 300}, {"pw4", 120000, 200, 300}, {"pw8", 66000, 200, 300},
                      {"pw16", 30000, 200, 300}, {"pw32-vw1", 3000, 100, 300}, {"pw1-w64", 676000, 130, 520}};   // (w64: 130 strips, the 64-bit advance)
    for (const Wl &w : ras) { Case c = geo(w.S, w.y, w.x, 2); c.raster = 1; add(c, std::string("gpu-inst-ras-") + w.n); }
    // the f32-sample walk with the in-walk downgrade (640 x 832) at TP = 32, 64, 128 (2.5, 1.15, 0.5 samples per raster pixel),
    // with and without a raster to write (below 2 samples per pixel the tap kernel would take the second: "fast_walk_only")
    const Wl dn[] = {{"pw8", 1331200, 640, 832}, {"pw16", 612352, 640, 832}, {"pw32", 266240, 640, 832}};
    for (const Wl &w : dn)
      for (int ras1 = 1; ras1 >= 0; --ras1) {
        Case c = geo(w.S, w.y, w.x, 2); c.raster = ras1; c.fast_walk_only = !ras1 && w.S < 2 * 640 * 832;
        add(c, std::string("gpu-inst-rec4-") + w.n + (ras1 ? "-ras" : "-nor"));
      }
    for (int f = FMT_SC16; f <= FMT_UC8; ++f) { Case c = geo(266240, 640, 832, 2); c.raster = 1; c.fmt = f; add(c, std::string("gpu-inst-rec4-pw32-ras-") + fmt_name(f)); }
    // the record walk with the downgrade ("raster_rec4" 0; its 47-sample lines hold 128 pixels up to 0.33 samples per pixel)
    Case c = geo(53248, 640, 832, 2); c.raster_rec4 = 0; c.raster = 1; add(c, "gpu-inst-rec-pw32-ras");
    c.raster = 0; c.fast_walk_only = 1; add(c, "gpu-inst-rec-pw32-nor");
    c = geo(12000, 200, 300, 2); c.raster = 1; add(c, "gpu-inst-ras-pw32");   // the 128-pixel raster-only tile two wavefronts high
  }
  return v;
}

}  // namespace plan_dump
