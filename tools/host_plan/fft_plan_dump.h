// fft_plan_dump.h -- the case list and the canonical text of tools/host_plan/fft_plan_dump_main.hip.
//
// Everything here is plain host C++ over the parameter structs of the FFT pass kernels (PassDesc, MixDesc, MidDesc, FftEpilogue)
// and the SRC_* / EPI_* / SIG_* names of fft_dev.h: they must be declared before this file is included.  It knows nothing of how
// a plan is made, so the same file formats the launches of an older revision whose launch macro was replaced by a recorder: that
// is how the fixture tests/golden/fft_plans_v1.txt was made (NOTEBOOK.md, "FFT plans").
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace fft_plan_dump {

// ---- canonical dumps: every field in declaration order; integers in decimal, floats / doubles as %a, pointers as 0 / 1 ("set")
struct Txt {
  std::string s;
  void f(const char *fmt, ...) {
    char b[512];
    va_list ap; va_start(ap, fmt); std::vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    s += b;
  }
};
inline void dump(Txt &t, const tsdr::FftEpilogue &e) {
  t.f("epi.out=%d epi.k0=%llu epi.cnt=%llu epi.log_scale=%d epi.kind=%d epi.gain=%a epi.amax_keys=%d epi.amax_lo=%llu epi.amax_cnt=%llu\n", e.out ? 1 : 0, e.k0,
      e.cnt, e.log_scale, e.kind, (double)e.gain, e.amax_keys ? 1 : 0, e.amax_lo, e.amax_cnt);
}
inline void dump(Txt &t, const tsdr::PassDesc &d) {
  t.f("mode=%d logR=%d logT=%d dir=%d scale=%a N=%llu A=%u B=%u tiles=%u logNtw=%d logBnext=%d logPprev=%d nprev=%d\n", d.mode, d.logR, d.logT, d.dir,
      (double)d.scale, d.N, d.A, d.B, d.tiles, d.logNtw, d.logBnext, d.logPprev, d.nprev);
  t.f("logRprev=%d,%d,%d,%d logR1=%d Aprime=%u k1tiles=%u rows=%u src_mode=%d src_n=%llu keep=%llu src_aux=%d src_w8=%a\n", d.logRprev[0], d.logRprev[1],
      d.logRprev[2], d.logRprev[3], d.logR1, d.Aprime, d.k1tiles, d.rows, d.src_mode, d.src_n, d.keep, d.src_aux ? 1 : 0, d.src_w8);
  dump(t, d.epi);
}
inline void dump(Txt &t, const tsdr::MixDesc &d) {
  t.f("mode=%d dir=%d logT=%d nst=%d scale=%a R=%u rad=%d,%d,%d,%d,%d,%d,%d,%d N=%llu A=%u B=%u tiles=%u Bnext=%u Pprev=%u\n", d.mode, d.dir, d.logT, d.nst,
      (double)d.scale, d.R, d.rad[0], d.rad[1], d.rad[2], d.rad[3], d.rad[4], d.rad[5], d.rad[6], d.rad[7], d.N, d.A, d.B, d.tiles, d.Bnext, d.Pprev);
  t.f("ntw_hi=%u ntw_lo=%u r_hi=%u r_lo=%u nprev=%d Rprev=%u,%u,%u,%u,%u,%u Wprev=%u,%u,%u,%u,%u,%u R1=%u Aprime=%u k1tiles=%u rows=%u\n", d.ntw_hi, d.ntw_lo,
      d.r_hi, d.r_lo, d.nprev, d.Rprev[0], d.Rprev[1], d.Rprev[2], d.Rprev[3], d.Rprev[4], d.Rprev[5], d.Wprev[0], d.Wprev[1], d.Wprev[2], d.Wprev[3],
      d.Wprev[4], d.Wprev[5], d.R1, d.Aprime, d.k1tiles, d.rows);
  // (twg: read by the strided two-step kernels alone; what another pass's descriptor holds there is not part of the record)
  t.f("src_mode=%d src_n=%llu keep=%llu tw_sets=%d twg=%d src_aux=%d src_w8=%a acc=%d rows_real=%d wf=%d rows_out=%d\n", d.src_mode, d.src_n, d.keep, d.tw_sets,
      d.mode == 0 && d.twg ? 1 : 0, d.src_aux ? 1 : 0, d.src_w8, d.acc ? 1 : 0, d.rows_real, d.wf ? 1 : 0, d.rows_out ? 1 : 0);
  dump(t, d.epi);
}
inline void dump(Txt &t, const tsdr::MidDesc &d) {
  t.f("R=%u Bc=%u ndir=%u logT=%d nprev=%d Rprev=%u,%u,%u,%u,%u,%u r_hi=%u r_lo=%u Bnext=%u ntw_hi=%u ntw_lo=%u tw_sets=%d w8=%a\n", d.R, d.Bc, d.ndir, d.logT,
      d.nprev, d.Rprev[0], d.Rprev[1], d.Rprev[2], d.Rprev[3], d.Rprev[4], d.Rprev[5], d.r_hi, d.r_lo, d.Bnext, d.ntw_hi, d.ntw_lo, d.tw_sets, d.w8);
}

inline unsigned long long fnv1a(const std::string &s) {
  unsigned long long h = 0xcbf29ce484222325ull;
  for (unsigned char c : s) { h ^= c; h *= 0x100000001b3ull; }
  return h;
}

// ---- one launch and one case, as text ------------------------------------------------------------------------
// bufs: "reads>writes" in roles (in, out, work = WS_FFT_B, mid = the fused autocorrelation's second buffer, - = none);
// tables: what has to exist before the launch -- "tw4096" (tw_small), "twg(R,Rn)", "optin" (dynamic LDS above 64 KiB), "-" (nothing)
struct Launch {
  std::string name, kernel, bufs, tables, params;
  unsigned grid, block;
  size_t lds;
};
struct Outcome {
  int status = 0;
  std::string err;
  bool copy = false;          // a one-point transform: a device copy, no launch
  size_t work_bytes = 0;      // WS_FFT_B asked for
  std::vector<Launch> steps;
};

inline std::string line(const char *id, const Outcome &o) {
  Txt t;
  t.f("%s status=%d", id, o.status);
  if (o.status) { t.f(" err=\"%s\"", o.err.c_str()); return t.s; }
  t.f(" work=%zu", o.work_bytes);
  if (o.copy) t.f(" copy");
  for (const Launch &l : o.steps)
    t.f(" | %s %s grid=%u block=%u lds=%zu %s %s hash=%016llx", l.name.c_str(), l.kernel.c_str(), l.grid, l.block, l.lds, l.bufs.c_str(), l.tables.c_str(),
        fnv1a(l.params));
  return t.s;
}
inline std::string full(const char *id, const Outcome &o) {
  std::string s = line(id, o) + "\n";
  for (const Launch &l : o.steps) s += "--- " + l.name + " " + l.kernel + "\n" + l.params;
  return s;
}

// ---- the case list ----------------------------------------------------------------------------------------------
enum What { W_FFT = 0, W_AUTOCORR = 1, W_WELCH = 2, W_STORE = 3, W_WATERFALL = 4 };   // fft_run | the fused autocorrelation | the three whole-row launches
struct Case {
  std::string id;
  int what = W_FFT;
  int no_mix2 = 0, big = 1, cu_count = 256;   // options ("fft_no_mix2", "fft_big") and the device's CU count
  unsigned long long n = 0, batch = 1;        // transform length (W_AUTOCORR: Mc) and count (rows: segments)
  int dir = -1;
  float scale = 1.0f;
  int src_mode = 0;                           // SRC_*
  unsigned long long src_n = 0, keep = 0;
  int aux = 0;                                // a loader factor array is handed in
  float src_scale = 1.0f;
  int epi = 0, amax = 0, log_scale = 0;       // EPI_* (0: none), with the fused findmax
  unsigned long long k0 = 0, cnt = 0;
  int sig_kind = 1;                           // rows: SIG_* of the samples
};

inline tsdr::FftEpilogue epilogue(const Case &c) {   // (pointers: any non-null value)
  tsdr::FftEpilogue e;
  e.out = reinterpret_cast<float *>(0x50000000ull);
  e.k0 = c.k0; e.cnt = c.cnt; e.log_scale = c.log_scale; e.kind = c.epi;
  if (c.epi == tsdr::EPI_REAL) e.gain = 6.0f;
  if (c.amax) { e.amax_keys = reinterpret_cast<unsigned long long *>(0x60000000ull); e.amax_lo = c.cnt / 8; e.amax_cnt = c.cnt / 2; }
  return e;
}

inline std::vector<Case> cases() {
  using namespace tsdr;
  std::vector<Case> v;
  char b[128];
  auto add = [&](Case c, const std::string &id) { c.id = id; v.push_back(c); };
  auto fft = [](unsigned long long n, unsigned long long batch, int dir) {
    Case c; c.n = n; c.batch = batch; c.dir = dir; c.scale = dir > 0 ? (float)(1.0 / (double)n) : 1.0f; return c;
  };
  // 1  plain transforms: the lengths and batches of tests/test_fft_path_gpu.py and tests/sample_routes.py that are 2^a 3^b 5^c
  //    (the others go through Bluestein's power-of-two transforms, which are in the list too); every third one inverse as well
  const unsigned long long lens[] = {1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 1 << 16, 1 << 17, 1 << 18, 1 << 20, 1 << 22, 1 << 24,
                                     6, 10, 15, 25, 45, 100, 120, 125, 200, 243, 250, 300, 625, 1000, 1536, 3000, 15625, 30000, 62500, 65610, 80000,
                                     100000, 250000, 390625, 500000, 1000000, 1080000, 2000000, 2400000, 3000000, 3600000, 4000000, 20000000};
  int li = 0;
  for (unsigned long long n : lens)
    for (int dir = -1; dir <= 1; dir += 2) {
      if (dir > 0 && li++ % 3) continue;   // (the direction moves `dir` and `scale` alone)
      std::snprintf(b, sizeof b, "c2c-%llu-%s", n, dir < 0 ? "fwd" : "inv");
      add(fft(n, 1, dir), b);
    }
  const unsigned long long rows[][2] = {{8, 1000}, {64, 33}, {256, 17}, {1024, 9}, {4096, 3}, {8192, 2}, {512, 41}, {1024, 37}, {2048, 11}, {4096, 5}, {500, 33},
                                        {1000, 19}, {2000, 6}, {4000, 3}, {768, 9}, {1280, 7}, {2500, 2}, {3200, 3}, {128, 300}, {512, 2}, {10, 777},
                                        {100, 41}, {250, 300}, {1000, 7}, {6000, 5}, {160000, 2}, {1024, 5}, {1000, 5}, {64, 5}};
  for (const auto &r : rows) {
    std::snprintf(b, sizeof b, "rows-%llux%llu", r[0], r[1]);
    add(fft(r[0], r[1], -1), b);
    if (r[0] > 256 && r[0] <= 4096 && r[0] != 1024) {   // fft_any hands these to the whole-row launch first
      Case c = fft(r[0], r[1], r[1] & 1 ? +1 : -1);
      c.what = W_STORE;
      std::snprintf(b, sizeof b, "store-%llux%llu", r[0], r[1]);
      add(c, b);
    }
  }
  // 2  the search windows (Mc = n / 2 of 4e6, 1e7, 4e7 samples, and of the windows the tests use): forward with each packing loader,
  //    inverse with SRC_POWER + EPI_AC (with and without the fused findmax), and the fused-middle sequence of the same call
  const unsigned long long mcs[] = {2000000, 5000000, 20000000, 750, 1500, 2500, 30000, 40000, 90000, 100000, 500000, 1000, 6000};
  const int packers[] = {SRC_REAL, SRC_IQPOW, SRC_IQPOW_SC16, SRC_IQPOW_SC8, SRC_IQPOW_UC8};
  const char *packer_name[] = {"real", "iqpow", "iqpow_sc16", "iqpow_sc8", "iqpow_uc8"};
  for (unsigned long long Mc : mcs) {
    for (int k = 0; k < 5; ++k) {
      if (k >= 2 && Mc != 2000000 && Mc != 40000 && Mc != 6000) continue;
      Case c = fft(Mc, 1, -1);
      c.src_mode = packers[k]; c.src_n = 2 * Mc - (k == 0 ? 1 : 0); c.src_scale = k >= 2 ? 1.0f / 128.0f : 1.0f;
      std::snprintf(b, sizeof b, "ac-fwd-%llu-%s", Mc, packer_name[k]);
      add(c, b);
    }
    for (int am = 0; am < 2; ++am) {
      Case c = fft(Mc, 1, +1);
      c.scale = (float)(0.5 / (double)Mc); c.src_mode = SRC_POWER; c.src_n = Mc;
      c.epi = EPI_AC; c.amax = am; c.k0 = Mc / 10; c.cnt = Mc / 2; c.log_scale = am; c.keep = (c.k0 + c.cnt + 1) / 2;
      std::snprintf(b, sizeof b, "ac-inv-%llu%s", Mc, am ? "-amax" : "");
      add(c, b);
      c.what = W_AUTOCORR; c.src_mode = am ? SRC_IQPOW : SRC_REAL; c.src_n = 2 * Mc;
      std::snprintf(b, sizeof b, "ac-mid-%llu%s", Mc, am ? "-iqpow-amax" : "-real");
      add(c, b);
    }
  }
  {   // the fused middle from integer IQ; a length without one (3^9 has no fused kernel); options off
    Case c = fft(2000000, 1, +1);
    c.what = W_AUTOCORR; c.scale = (float)(0.5 / 2e6); c.src_mode = SRC_IQPOW_SC8; c.src_n = 4000000; c.src_scale = 1.0f / 128.0f;
    c.epi = EPI_AC; c.amax = 1; c.k0 = 200000; c.cnt = 1000000; c.keep = 600001;
    add(c, "ac-mid-2000000-sc8");
    c.src_mode = SRC_IQPOW_SC16; c.src_scale = 1.0f / 32768.0f; add(c, "ac-mid-2000000-sc16");
    c.src_mode = SRC_IQPOW_UC8; c.src_scale = 1.0f / 128.0f; add(c, "ac-mid-2000000-uc8");
    c.src_mode = SRC_REAL; c.src_scale = 1.0f;
    c.no_mix2 = 1; add(c, "ac-mid-2000000-nomix2"); c.no_mix2 = 0;
    c.big = 0; add(c, "ac-mid-2000000-nobig"); c.big = 1;
    const unsigned long long nomid[] = {19683, 177147, 243, 59049, 6561 * 7, 3000000000ull};
    for (unsigned long long Mc : nomid) {
      c.n = Mc; c.src_n = 2 * Mc;
      std::snprintf(b, sizeof b, "ac-mid-%llu-none", Mc);
      add(c, b);
    }
  }
  // 3  the power-of-two search's forward transform, inverse with SRC_POWER (zero-padded route) and with SRC_C2C + src_n (n = 2 * 2^k)
  for (int logMc : {9, 11, 12, 17, 22}) {
    const unsigned long long Mc = 1ull << logMc;
    for (int k = 0; k < 5; ++k) {
      Case c = fft(Mc, 1, -1);
      c.src_mode = packers[k]; c.src_n = Mc + Mc / 3; c.src_scale = k >= 2 ? 1.0f / 32768.0f : 1.0f;
      std::snprintf(b, sizeof b, "acp2-fwd-%d-%s", logMc, packer_name[k]);
      add(c, b);
    }
    Case c = fft(Mc, 1, +1);
    c.scale = (float)(0.5 / (double)Mc); c.src_mode = SRC_POWER; c.src_n = Mc; c.keep = Mc / 3 + 1;
    std::snprintf(b, sizeof b, "acp2-inv-%d-power", logMc);
    add(c, b);
    c.src_mode = SRC_C2C; c.src_n = 2 * Mc; c.keep = Mc / 2;
    std::snprintf(b, sizeof b, "acp2-inv-%d-c2c", logMc);
    add(c, b);
  }
  // 4  the complex search: integer or ComplexF32 samples in, SRC_ABS2 + EPI_CAC back (with and without findmax)
  const unsigned long long cls[] = {4000000, 10000000, 40000000, 1000, 4096, 65536, 100000};
  const int iqs[] = {SRC_C2C, SRC_IQ_SC16, SRC_IQ_SC8, SRC_IQ_UC8};
  const char *iq_name[] = {"cf32", "sc16", "sc8", "uc8"};
  for (unsigned long long n : cls) {
    for (int k = 0; k < 4; ++k) {
      Case c = fft(n, 1, -1);
      c.src_mode = iqs[k]; c.src_scale = k == 1 ? 1.0f / 32768.0f : k ? 1.0f / 128.0f : 1.0f;
      std::snprintf(b, sizeof b, "cac-fwd-%llu-%s", n, iq_name[k]);
      add(c, b);
    }
    for (int am = 0; am < 2; ++am) {
      Case c = fft(n, 1, +1);
      c.src_mode = SRC_ABS2; c.epi = EPI_CAC; c.amax = am; c.log_scale = am; c.k0 = n / 20; c.cnt = n / 4; c.keep = c.k0 + c.cnt;
      std::snprintf(b, sizeof b, "cac-inv-%llu%s", n, am ? "-amax" : "");
      add(c, b);
    }
  }
  // 5  getSpectrum (EPI_SPEC from every kind of samples), batched integer IQ through the first pass, and the resampler's two
  //    transforms (SRC_STUFF, then SRC_MULH + EPI_REAL)
  const unsigned long long sls[] = {1024, 1000, 6000, 80000, 65536, 1048576, 3000000};
  const int elw[] = {SRC_RE0, SRC_C2C, SRC_IQ_SC16, SRC_IQ_SC8, SRC_IQ_UC8};
  const char *elw_name[] = {"real", "cf32", "sc16", "sc8", "uc8"};
  for (unsigned long long n : sls)
    for (int k = 0; k < 5; ++k)
      for (int lg = 0; lg < 2; ++lg) {
        if (lg && k != 1) continue;
        Case c = fft(n, 1, -1);
        c.src_mode = elw[k]; c.src_scale = k >= 2 ? 1.0f / 128.0f : 1.0f; c.epi = EPI_SPEC; c.cnt = n; c.k0 = n / 2; c.log_scale = lg;
        std::snprintf(b, sizeof b, "spec-%llu-%s%s", n, elw_name[k], lg ? "-db" : "");
        add(c, b);
      }
  for (unsigned long long n : {512ull, 6000ull, 8192ull, 10000ull})
    for (int k = 2; k < 5; ++k) {
      Case c = fft(n, 30, -1);
      c.src_mode = elw[k]; c.src_scale = 1.0f / 128.0f;
      std::snprintf(b, sizeof b, "rowsiq-%llux30-%s", n, elw_name[k]);
      add(c, b);
    }
  for (unsigned long long n : {512ull, 1000ull, 4096ull, 6000ull, 12000ull, 65536ull, 1000000ull, 1048576ull}) {
    Case c = fft(n, 1, -1);
    c.src_mode = SRC_STUFF; c.src_n = 3;
    std::snprintf(b, sizeof b, "rs-stuff-%llu", n);
    add(c, b);
    c = fft(n, 1, +1);
    c.src_mode = SRC_MULH; c.aux = 1; c.epi = EPI_REAL; c.cnt = n;
    std::snprintf(b, sizeof b, "rs-mulh-%llu", n);
    add(c, b);
  }
  // 6  options and sizes that move the split: "fft_no_mix2" on, "fft_big" off, total points above 2^22, another CU count
  for (unsigned long long n : {1000ull, 6000ull, 100000ull, 1000000ull, 2000000ull, 4000000ull}) {
    Case c = fft(n, 1, -1);
    c.no_mix2 = 1; std::snprintf(b, sizeof b, "opt-nomix2-%llu", n); add(c, b); c.no_mix2 = 0;
    c.big = 0; std::snprintf(b, sizeof b, "opt-nobig-%llu", n); add(c, b); c.big = 1;
    c.cu_count = 64; std::snprintf(b, sizeof b, "opt-cu64-%llu", n); add(c, b);
  }
  for (unsigned long long bt : {2ull, 5ull, 42ull}) { std::snprintf(b, sizeof b, "big-100000x%llu", bt); add(fft(100000, bt, -1), b); }   // 42: above 2^22
  add(fft(4194304 + 2097152, 1, -1), "big-6291456");
  add(fft(1000000, 5, +1), "big-1000000x5");
  add(fft(1ull << 25, 1, -1), "big-33554432");   // four power-of-two passes
  // 7  the whole-row launches: getWelch's accumulator, tsdr_fft_c2c's batched rows, getWaterfall's writer -- every kernel of the
  //    row table, the generic kernel, each kind of samples, two CU counts, the options, lengths they decline
  const unsigned long long rls[] = {2, 64, 100, 128, 256, 300, 500, 512, 768, 960, 1000, 1200, 1280, 1600, 2000, 2048, 2500, 3000, 3200, 6,
                                    4000, 4096, 1024, 4095, 4100, 8192};
  for (int w = W_WELCH; w <= W_WATERFALL; ++w)
    for (unsigned long long n : rls)
      for (int kind = 0; kind < 5; ++kind) {
        if (kind != 1 && n != 1000 && n != 2048 && n != (w == W_WELCH ? 960u : 2000u)) continue;   // (960: the generic kernel; 2000: a pass-kernel tile)
        if (w == W_STORE && kind == 0) continue;
        Case c = fft(n, 325, w == W_STORE ? +1 : -1);
        c.what = w; c.sig_kind = kind; c.src_scale = kind >= 2 ? 1.0f / 128.0f : 1.0f;
        if (w != W_STORE || kind >= 2) { c.dir = -1; c.scale = 1.0f; }
        std::snprintf(b, sizeof b, "%s-%llu-%s", w == W_WELCH ? "welch" : w == W_STORE ? "store" : "wfall", n, elw_name[kind]);
        add(c, b);
      }
  for (int w = W_WELCH; w <= W_WATERFALL; ++w)
    for (unsigned long long n : {1000ull, 2048ull, 3000ull}) {
      const char *wn = w == W_WELCH ? "welch" : w == W_STORE ? "store" : "wfall";
      Case c = fft(n, 20000, -1);
      c.what = w;
      std::snprintf(b, sizeof b, "%s-%llu-many", wn, n); add(c, b);
      c.cu_count = 64; std::snprintf(b, sizeof b, "%s-%llu-many-cu64", wn, n); add(c, b); c.cu_count = 256;
      c.cu_count = 0; std::snprintf(b, sizeof b, "%s-%llu-many-cu0", wn, n); add(c, b); c.cu_count = 256;
      c.no_mix2 = 1; std::snprintf(b, sizeof b, "%s-%llu-nomix2", wn, n); add(c, b); c.no_mix2 = 0;
      c.batch = 1; std::snprintf(b, sizeof b, "%s-%llu-one", wn, n); add(c, b);
      c.batch = 0; std::snprintf(b, sizeof b, "%s-%llu-zero", wn, n); add(c, b);
    }
  // 8  the calls of tests/test_fft_plan_gpu.py: the smallest length that reaches each kind of step
  {
    add(fft(64, 5, -1), "gpu-pow2-rows");
    add(fft(512, 1, -1), "gpu-pow2-two-pass");
    add(fft(1 << 17, 1, +1), "gpu-pow2-three-pass");
    add(fft(100, 4, -1), "gpu-generic-one-pass");
    add(fft(300, 4, -1), "gpu-generic-last");                                       // 25 x 12: the last factor has no register-step kernel
    add(fft(6000, 1, -1), "gpu-two-step");                                          // 75 x 80, the column table
    add(fft(80000, 1, -1), "gpu-three-step");                                       // 500 x 160
    Case c = fft(5000, 1, +1);                                                      // calculate_autocorrelation(x[1:10000], 1, 100, 5000)
    c.what = W_AUTOCORR; c.scale = (float)(0.5 / 5000.0); c.src_mode = SRC_REAL; c.src_n = 10000; c.epi = EPI_AC; c.log_scale = 1; c.k0 = 100; c.cnt = 4900; c.keep = 2500;
    add(c, "gpu-mid-two-step");
    c.n = 90000; c.scale = (float)(0.5 / 9e4); c.src_n = 180000; c.k0 = 1000; c.cnt = 89000; c.keep = 45000;   // ... (x[1:180000], 1, 1000, 90000)
    add(c, "gpu-mid-three-step");
    c = fft(1000, 7, -1); c.what = W_STORE; add(c, "gpu-rows-store");
    c = fft(2000, 7, -1); c.what = W_WELCH; add(c, "gpu-rows-welch");
    c = fft(960, 7, -1); c.what = W_WELCH; add(c, "gpu-rows-welch-generic");
    c = fft(500, 7, -1); c.what = W_WATERFALL; add(c, "gpu-rows-waterfall");
  }
  // 9  a batch of 0, and each error text
  {
    add(fft(4096, 0, -1), "zero-batch-pow2");
    add(fft(6000, 0, -1), "zero-batch-mixed");
    add(fft(1ull << 32, 1, -1), "err-pow2-length");
    add(fft(7000, 1, -1), "err-mixed-length");
    add(fft(3ull << 31, 1, -1), "err-mixed-length-2^31");
    add(fft(1ull << 20, 1ull << 20, -1), "err-batch-pow2");
    add(fft(1000000, 1ull << 21, -1), "err-batch-mixed");
    Case c = fft(256, 1, -1); c.src_mode = SRC_REAL; c.src_n = 300; add(c, "err-loader-pow2-one-pass");
    c = fft(4096, 3, -1); c.src_mode = SRC_REAL; c.src_n = 300; add(c, "err-loader-pow2-batch");
    c = fft(4096, 3, -1); c.epi = EPI_SPEC; c.cnt = 4096; c.src_mode = SRC_IQ_SC8; add(c, "err-epilogue-pow2-batch");
    c = fft(200, 1, -1); c.src_mode = SRC_RE0; add(c, "err-loader-mixed-one-pass");
    c = fft(6000, 3, -1); c.src_mode = SRC_RE0; add(c, "err-loader-mixed-batch");
    c = fft(200, 1, -1); c.epi = EPI_SPEC; c.cnt = 200; add(c, "err-epilogue-mixed-one-pass");
    c = fft(6000, 3, -1); c.epi = EPI_SPEC; c.cnt = 6000; c.src_mode = SRC_IQ_SC8; add(c, "err-epilogue-mixed-batch");
    add(fft(2, 1ull << 33, -1), "err-rows-pow2");
    add(fft(3, 1ull << 33, -1), "err-rows-mixed");
    add(fft(270, 1ull << 31, -1), "err-grid-mixed");
  }
  // 10  the smallest length that reaches each table entry (and each profile name) the sections above do not: found by planning
  //     every 2^a 3^b 5^c length below 2^31 (NOTEBOOK.md, "FFT plans")
  for (unsigned long long n : {729ull, 1152ull, 3125ull, 5120ull, 9600ull, 11520ull, 16875ull, 18750ull, 20250ull, 20736ull, 40960ull, 512000ull, 9765625ull,
                               244140625ull}) {
    std::snprintf(b, sizeof b, "reach-%llu", n);
    add(fft(n, 1, -1), b);
  }
  for (unsigned long long Mc : {288ull, 384ull, 4608ull, 5760ull, 9600ull, 10240ull, 19200ull}) {
    Case c = fft(Mc, 1, +1);
    c.what = W_AUTOCORR; c.scale = (float)(0.5 / (double)Mc); c.src_mode = SRC_REAL; c.src_n = 2 * Mc; c.epi = EPI_AC; c.cnt = Mc; c.keep = (Mc + 1) / 2;
    std::snprintf(b, sizeof b, "reach-mid-%llu", Mc);
    add(c, b);
  }
  return v;
}

}  // namespace fft_plan_dump
