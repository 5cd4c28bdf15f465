// resampler_state.h -- the init_resampler closure behind tsdr_resampler (spectrum.hip; the Float64 twin's kernels live in
// spectra64.hip).
#pragma once

#include "common.h"

struct tsdr_resampler {
  tsdr_ctx *ctx;
  size_t bufferSize, sizeFFT;
  int up;
  double2 *H = nullptr;    // initLPF's H: ComplexF64 as in the reference (the Float64 window promotes it, Resampler.jl:93-97)
  double2 *Hs = nullptr;   // (H[k] + conj H[N-k]) / 2 for k <= N/2: the filter of the real part (half-size route), or null
  float2 *work = nullptr;  // containerFFT / inFFT / outFFT, device
  double2 *tw = nullptr;   // half-size route: {cos, sin}(2 pi e / N) for e < 1024, then for e = 1024 h (h <= N / 2048 + 1)
  // init_resampler(Float64, ...) (tsdr_resampler_init_f64): the same H; containerFFT in ComplexF64, ping / pong of sizeFFT
  // values each.  The f32 fields work / Hs / tw stay unallocated and tsdr_resampler_run[_d] refuses the object (TSDR_EINVAL),
  // as tsdr_resampler_run_f64[_d] refuses an f32 one.
  bool f64 = false;
  double2 *A64 = nullptr, *B64 = nullptr;
};
