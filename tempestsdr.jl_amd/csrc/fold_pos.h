// fold_pos.h -- the coordinates of frame folding, shared by raster_fold.hip (the envelope fold, include/tempest_hip_fold.h) and
// raster_cfold.hip (the phase-coherent fold, include/tempest_hip_cfold.h): both sample frame f of a buffer at the same positions.
//
// B = t0 + f*T is split once per frame into bi = floor(B) and bf = B - bi (exact); a pixel's position relative to bi is
// s = bf + ((m + 1/2)*(T/P) - 1/2), so the f64 rounding happens at the magnitude of one frame, not of the buffer.  The buffer
// clamps act on s as [-bi, n-1-bi].
#pragma once
#include "common.h"

namespace tsdr {

struct FramePos {   // one frame's origin: integer part, and the clamps relative to it
  double bf, lo, hi, hik;
  long long bi;
};

// A: a launch's arguments with t0 (double) and n (long long, samples of the buffer)
template <typename Args>
__device__ inline FramePos frame_pos(const Args &A, double T, int f) {
  const double B = A.t0 + (double)f * T;
  const double bi = floor(B);
  return FramePos{B - bi, -bi, (double)(A.n - 1) - bi, (double)(A.n - 2) - bi, (long long)bi};
}

// position of pixel m of the frame at `fp`, relative to fp.bi, before the buffer clamps
__device__ inline double fold_s(const FramePos &fp, double spp, unsigned m) { return fp.bf + (((double)m + 0.5) * spp - 0.5); }
// ... its left tap (relative to fp.bi) and the weight of the right one
__device__ inline int fold_tap(const FramePos &fp, double s, double &d) {
  s = fmin(fmax(s, fp.lo), fp.hi);
  const double k = fmin(floor(s), fp.hik);
  d = s - k;
  return (int)k;
}

}  // namespace tsdr
