// amax.h -- findmax behind the autocorrelations (autocorr.hip owns the code; autocorr_cplx.hip shares it): one request per search,
// delivered to pinned host memory by the kernel itself and polled for by the host.
#pragma once
#include "common.h"

namespace tsdr {

// findmax fused into the autocorrelation's last pass: the window and where the result goes (see amax_begin / amax_wait)
struct AmaxReq {
  size_t lo = 0, cnt = 0;  // window out[lo .. lo + cnt)
  unsigned long long *key = nullptr, *clear = nullptr, *slots = nullptr;
  unsigned *arrived = nullptr;
  unsigned long long *host = nullptr;
  unsigned long long seq = 0;
  bool fused = false;      // out: the last pass delivered the maximum (else the caller runs k_argmax)
};

int amax_begin(tsdr_ctx *ctx, AmaxReq *r);
int amax_wait(tsdr_ctx *ctx, unsigned long long seq, size_t *idx, float *val);
int argmax_launch(tsdr_ctx *ctx, const float *v, size_t n, const AmaxReq &r);   // k_argmax over v[0 .. n)
int amax_publish(tsdr_ctx *ctx, const AmaxReq &r);                              // k_amax_publish behind a fused last pass

}  // namespace tsdr
