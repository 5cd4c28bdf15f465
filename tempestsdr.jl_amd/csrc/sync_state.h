// sync_state.h -- the SyncXY state behind tsdr_sync (sync.hip; the Float64 twin's kernels live in sync64.hip).
#pragma once

#include "common.h"

struct tsdr_sync {
  tsdr_ctx *ctx;
  int y_t, x_t;
  int wmin_y, wmax_y, wmin_x, wmax_x;
  float h[5];
  float *beta_x = nullptr;  // device, (1+wmax_x-wmin_x) x x_t   (the current set: one of bset[])
  float *beta_y = nullptr;  // device, (1+wmax_y-wmin_y) x y_t
  float *bset[4][2] = {};   // [pipeline lane][x / y]: sync_use_lane
  int *pending = nullptr;   // device: [cur] = s_y the next vsync call will return (argmax of beta_y); double-buffered
  int cur = 0;
  // SyncXY{Float64} (tsdr_sync_create_f64, sync64.hip): taps and beta fields in f64; the f32 fields above stay unallocated and
  // every f32 entry point refuses the object (TSDR_EINVAL), as the f64 ones refuse an f32 state
  bool f64 = false;
  double h64[5] = {};
  double *beta64_x = nullptr, *beta64_y = nullptr;
  int *blk64 = nullptr;     // device: per-workgroup argmax records of the f64 beta scan
  size_t blk64_cap = 0;
};

