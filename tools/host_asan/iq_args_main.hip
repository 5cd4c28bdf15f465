// Stand-alone host program for tools/asan_host_iq.sh: the argument checks of the integer IQ entry points (tsdr_*_iq, tsdr_*_iq_d,
// tsdr_iq_expand_d) under AddressSanitizer + UBSan.  Every call here must be answered on the host, before anything is enqueued:
// a NULL context, an unknown format, a pointer at half a sample, a misaligned output, and the n == 0 / N == 0 cases.  No GPU is
// needed or touched: the context is a bare tsdr_ctx object, never one from tsdr_create.
#include <cstdio>
#include <cstring>

#include "../../tempestsdr.jl_amd/csrc/common.h"

static int fails = 0;
#define EXPECT(call, want)                                                                    \
  do {                                                                                        \
    const int rc_ = (call);                                                                   \
    if (rc_ != (want)) { std::printf("FAIL %s -> %d, expected %d\n", #call, rc_, (want)); ++fails; } \
  } while (0)
#define EXPECT_ERR(call, word)                                                                \
  do {                                                                                        \
    c.err.clear();                                                                            \
    const int rc_ = (call);                                                                   \
    if (rc_ != TSDR_EINVAL || c.err.find(word) == std::string::npos) {                        \
      std::printf("FAIL %s -> %d [%s], expected TSDR_EINVAL naming %s\n", #call, rc_, c.err.c_str(), word); ++fails; } \
  } while (0)

int main() {
  alignas(16) static unsigned char in[64];
  alignas(16) static float out[16];
  static double m[8];
  const void *iq = in;
  // NULL context: every entry point, before anything else
  EXPECT(tsdr_spectrum_iq_d(nullptr, iq, TSDR_IQ_SC8, 1.f, 4, 0, out), TSDR_EINVAL);
  EXPECT(tsdr_spectrum_iq(nullptr, iq, TSDR_IQ_SC8, 1.f, 4, 0, out), TSDR_EINVAL);
  EXPECT(tsdr_welch_iq_d(nullptr, iq, TSDR_IQ_SC16, 1.f, 4, 2, 0, out), TSDR_EINVAL);
  EXPECT(tsdr_welch_iq(nullptr, iq, TSDR_IQ_SC16, 1.f, 4, 2, 0, out), TSDR_EINVAL);
  EXPECT(tsdr_waterfall_iq_d(nullptr, iq, TSDR_IQ_UC8, 1.f, 4, 2, m), TSDR_EINVAL);
  EXPECT(tsdr_waterfall_iq(nullptr, iq, TSDR_IQ_UC8, 1.f, 4, 2, m), TSDR_EINVAL);
  EXPECT(tsdr_am_demod_iq_d(nullptr, iq, TSDR_IQ_SC8, 1.f, 4, out), TSDR_EINVAL);
  EXPECT(tsdr_abs2_iq_d(nullptr, iq, TSDR_IQ_SC8, 1.f, 4, out), TSDR_EINVAL);
  EXPECT(tsdr_invert_am_iq_d(nullptr, iq, TSDR_IQ_SC8, 1.f, 4, out), TSDR_EINVAL);
  EXPECT(tsdr_fm_demod_iq_d(nullptr, iq, TSDR_IQ_SC8, 1.f, 4, out), TSDR_EINVAL);
  EXPECT(tsdr_iq_expand_d(nullptr, iq, TSDR_IQ_SC8, 1.f, 4, out), TSDR_EINVAL);
  tsdr_ctx c;
  for (int fmt : {-1, 4, 1000, -2147483647 - 1}) {   // unknown formats
    EXPECT_ERR(tsdr_spectrum_iq_d(&c, iq, fmt, 1.f, 4, 0, out), "iq_fmt");
    EXPECT_ERR(tsdr_spectrum_iq(&c, iq, fmt, 1.f, 4, 0, out), "iq_fmt");
    EXPECT_ERR(tsdr_welch_iq_d(&c, iq, fmt, 1.f, 4, 2, 0, out), "iq_fmt");
    EXPECT_ERR(tsdr_welch_iq(&c, iq, fmt, 1.f, 4, 2, 0, out), "iq_fmt");
    EXPECT_ERR(tsdr_waterfall_iq_d(&c, iq, fmt, 1.f, 4, 2, m), "iq_fmt");
    EXPECT_ERR(tsdr_waterfall_iq(&c, iq, fmt, 1.f, 4, 2, m), "iq_fmt");
    EXPECT_ERR(tsdr_am_demod_iq_d(&c, iq, fmt, 1.f, 4, out), "iq_fmt");
    EXPECT_ERR(tsdr_abs2_iq_d(&c, iq, fmt, 1.f, 4, out), "iq_fmt");
    EXPECT_ERR(tsdr_invert_am_iq_d(&c, iq, fmt, 1.f, 4, out), "iq_fmt");
    EXPECT_ERR(tsdr_fm_demod_iq_d(&c, iq, fmt, 1.f, 4, out), "iq_fmt");
    EXPECT_ERR(tsdr_iq_expand_d(&c, iq, fmt, 1.f, 4, out), "iq_fmt");
  }
  // half a sample: an odd byte (8-bit), 2 mod 4 (sc16), 4 mod 8 (cf32)
  const struct { int fmt, shift; } half[] = {{TSDR_IQ_SC8, 1}, {TSDR_IQ_UC8, 1}, {TSDR_IQ_SC16, 2}, {TSDR_IQ_CF32, 4}};
  for (const auto &h : half) {
    const void *p = in + h.shift;
    EXPECT_ERR(tsdr_spectrum_iq_d(&c, p, h.fmt, 1.f, 4, 0, out), " iq ");
    EXPECT_ERR(tsdr_welch_iq_d(&c, p, h.fmt, 1.f, 4, 2, 0, out), " iq ");
    EXPECT_ERR(tsdr_waterfall_iq_d(&c, p, h.fmt, 1.f, 4, 2, m), " iq ");
    EXPECT_ERR(tsdr_am_demod_iq_d(&c, p, h.fmt, 1.f, 4, out), " iq ");
    EXPECT_ERR(tsdr_abs2_iq_d(&c, p, h.fmt, 1.f, 4, out), " iq ");
    EXPECT_ERR(tsdr_invert_am_iq_d(&c, p, h.fmt, 1.f, 4, out), " iq ");
    EXPECT_ERR(tsdr_fm_demod_iq_d(&c, p, h.fmt, 1.f, 4, out), " iq ");
    EXPECT_ERR(tsdr_iq_expand_d(&c, p, h.fmt, 1.f, 4, out), " iq ");
  }
  // misaligned outputs
  float *y2 = reinterpret_cast<float *>(reinterpret_cast<char *>(out) + 2);
  double *m4 = reinterpret_cast<double *>(reinterpret_cast<char *>(m) + 4);
  EXPECT_ERR(tsdr_spectrum_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, 0, y2), " y ");
  EXPECT_ERR(tsdr_welch_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, 2, 0, y2), " y ");
  EXPECT_ERR(tsdr_waterfall_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, 2, m4), " sMatrix ");
  EXPECT_ERR(tsdr_am_demod_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, y2), " out ");
  EXPECT_ERR(tsdr_abs2_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, y2), " out ");
  EXPECT_ERR(tsdr_invert_am_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, y2), " out ");
  EXPECT_ERR(tsdr_fm_demod_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, y2), " out ");
  EXPECT_ERR(tsdr_iq_expand_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, out + 1), " cf32_out ");
  // NULL pointers and empty inputs, as the ComplexF32 twins
  EXPECT(tsdr_spectrum_iq_d(&c, nullptr, TSDR_IQ_SC8, 1.f, 4, 0, out), TSDR_EINVAL);
  EXPECT(tsdr_spectrum_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, 0, nullptr), TSDR_EINVAL);
  EXPECT(tsdr_spectrum_iq_d(&c, nullptr, TSDR_IQ_SC8, 1.f, 0, 0, nullptr), TSDR_OK);
  EXPECT(tsdr_welch_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, 2, 0, nullptr), TSDR_EINVAL);
  EXPECT(tsdr_welch_iq_d(&c, nullptr, TSDR_IQ_SC8, 1.f, 4, 2, 0, out), TSDR_EINVAL);
  EXPECT(tsdr_waterfall_iq_d(&c, nullptr, TSDR_IQ_SC8, 1.f, 4, 2, m), TSDR_EINVAL);
  EXPECT(tsdr_waterfall_iq(&c, iq, TSDR_IQ_SC8, 1.f, 4, 0, m), TSDR_EINVAL);
  EXPECT(tsdr_am_demod_iq_d(&c, nullptr, TSDR_IQ_SC16, 1.f, 0, nullptr), TSDR_OK);
  EXPECT(tsdr_abs2_iq_d(&c, iq, TSDR_IQ_UC8, 1.f, 0, out), TSDR_OK);
  EXPECT(tsdr_fm_demod_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 0, out), TSDR_OK);
  EXPECT(tsdr_invert_am_iq_d(&c, iq, TSDR_IQ_SC8, 1.f, 0, out), TSDR_EINVAL);
  EXPECT(tsdr_am_demod_iq_d(&c, nullptr, TSDR_IQ_SC8, 1.f, 4, out), TSDR_EINVAL);
  EXPECT(tsdr_iq_expand_d(&c, iq, TSDR_IQ_SC8, 1.f, 0, out), TSDR_OK);
  EXPECT(tsdr_iq_expand_d(&c, iq, TSDR_IQ_SC8, 1.f, 4, nullptr), TSDR_EINVAL);
  std::printf(fails ? "%d check(s) failed\n" : "iq argument checks: all answered on the host, no sanitizer report\n", fails);
  return fails ? 1 : 0;
}
