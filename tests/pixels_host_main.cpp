// Stand-alone check of be_observe_pixels' host logic in csrc/pixels_host.h (no HIP), built by the host
// C++ compiler alone under ASan + UBSan (tests/test_pixels_host.py):
//   * prints "row XX FIRST TAPS K0 .. K9" for every output of the 100 -> 40 resize (the test compares
//     them against its numpy restatement and the fixture);
//   * checks the accumulator bound, the six packed rows and the argument checks;
//   * prints one OK line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pixels_host.h"

using namespace behost;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

static bool says(const char* msg, const char* part) { return msg && strstr(msg, part); }

int main() {
  int32_t kk[PIX_OUT][PIX_TAPS], bounds[PIX_OUT][2];
  CHECK(pix_coeffs(kk, bounds));
  for (int xx = 0; xx < PIX_OUT; ++xx) {
    printf("row %d %d %d", xx, bounds[xx][0], bounds[xx][1]);
    int64_t sum = 0, mag = 0;
    for (int t = 0; t < PIX_TAPS; ++t) {
      printf(" %d", kk[xx][t]);
      sum += kk[xx][t];
      mag += kk[xx][t] < 0 ? -(int64_t)kk[xx][t] : kk[xx][t];
      if (t >= bounds[xx][1]) CHECK(kk[xx][t] == 0);
    }
    printf("\n");
    CHECK(bounds[xx][0] >= 0 && bounds[xx][1] >= 1 && bounds[xx][1] <= PIX_TAPS && bounds[xx][0] + bounds[xx][1] <= PIX_PATCH);
    CHECK(sum > (1 << PIX_BITS) - 16 && sum < (1 << PIX_BITS) + 16);          // the weights sum to 1, rounded per tap
    CHECK(((int64_t)1 << (PIX_BITS - 1)) + 255 * mag < ((int64_t)1 << 31));   // PIL's int accumulator holds any row
    CHECK(bounds[xx][0] == pix_first_of(xx) && pix_row_of(xx) >= 0 && pix_row_of(xx) < PIX_ROWS);
  }
  PixCoeffs c;
  CHECK(pix_coeffs_pack(&c));
  for (int xx = 0; xx < PIX_OUT; ++xx) CHECK(memcmp(c.k[pix_row_of(xx)], kk[xx], sizeof kk[xx]) == 0);
  // the filter is symmetric: the last outputs mirror the first
  for (int xx = 0; xx < PIX_OUT; ++xx)
    for (int t = 0; t < bounds[xx][1]; ++t) CHECK(kk[xx][t] == kk[PIX_OUT - 1 - xx][bounds[xx][1] - 1 - t]);
  CHECK(pix_bicubic(0.0) == 1.0 && pix_bicubic(1.0) == 0.0 && pix_bicubic(2.0) == 0.0 && pix_bicubic(-0.5) == pix_bicubic(0.5));

  // the argument checks, in their order
  alignas(16) uint8_t buf[64];
  alignas(16) float f32[8];
  CHECK(pixels_args_error(buf, buf + 16, f32, 5, 20) == nullptr);
  CHECK(pixels_args_error(buf, nullptr, nullptr, 5, 20) == nullptr);
  CHECK(pixels_args_error(nullptr, buf, nullptr, 0, 0) == nullptr);
  CHECK(pixels_args_error(nullptr, nullptr, f32, PIX_MAX_RADIUS, PIX_MAX_RADIUS) == nullptr);
  CHECK(says(pixels_args_error(nullptr, nullptr, nullptr, 5, 20), "needs patch, out or out_f32"));
  CHECK(says(pixels_args_error(buf + 4, nullptr, nullptr, 5, 20), "16-byte"));
  CHECK(says(pixels_args_error(nullptr, buf + 8, nullptr, 5, 20), "16-byte"));
  CHECK(says(pixels_args_error(nullptr, nullptr, f32 + 1, 5, 20), "16-byte"));
  CHECK(says(pixels_args_error(buf, nullptr, nullptr, PIX_MAX_RADIUS + 1, 20), "radius"));
  CHECK(says(pixels_args_error(buf, nullptr, nullptr, 5, PIX_MAX_RADIUS + 1), "radius"));
  CHECK(says(pixels_args_error(buf, nullptr, nullptr, -1, 20), "radius"));
  printf("pixels_host: OK\n");
  return 0;
}
