// Stand-alone check of be_step's wide-instance rule (behost::step2_wide, csrc/host_logic.h): host
// C++ only, built and run by tests/test_step2_wide_host.py under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>

#include "host_logic.h"

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); ++fails; } } while (0)

int main() {
  using namespace behost;
  alignas(16) static unsigned char buf[64];
  const void* a0 = buf;            // 16-byte aligned
  const void* a4 = buf + 4;
  const void* a8 = buf + 8;
  const void* a16 = buf + 16;
  const void* a32 = buf + 32;

  // the rule on its own (force = -1) follows the default wherever the instance may run
  const bool D = STEP2_WIDE_DEFAULT;
  CHECK(step2_wide(0, a0, a16, a32) == false);
  CHECK(step2_wide(31, a0, a16, a32) == false);
  CHECK(step2_wide(32, a0, a16, a32) == D);
  CHECK(step2_wide(33, a0, a16, a32) == false);
  CHECK(step2_wide(64, a0, a16, a32) == D);
  CHECK(step2_wide((1ll << 29) - 32, a0, a16, a32) == D);
  CHECK(step2_wide((1ll << 29) - 31, a0, a16, a32) == false);
  CHECK(step2_wide(-32, a0, a16, a32) == false);

  // the overrides: 1 takes the instance wherever it is correct, 0 never
  const int64_t sizes[] = {0, 31, 32, 33, 64, (1ll << 29) - 32};
  const bool whole[] = {false, false, true, false, true, true};
  for (int k = 0; k < 6; ++k) {
    CHECK(step2_wide(sizes[k], a0, a16, a32, 1) == whole[k]);
    CHECK(step2_wide(sizes[k], a0, a16, a32, 0) == false);
    CHECK(step2_wide(sizes[k], a0, a16, a32, -1) == (whole[k] && D));
  }

  // each pointer misaligned by 4 and by 8, and null: never, whatever the override
  const void* bad[] = {a4, a8, nullptr};
  const int forces[] = {-1, 0, 1};
  for (const int force : forces)
    for (const void* b : bad) {
      CHECK(step2_wide(64, b, a16, a32, force) == false);
      CHECK(step2_wide(64, a0, b, a32, force) == false);
      CHECK(step2_wide(64, a0, a16, b, force) == false);
    }
  CHECK(step2_wide(64, a0, a0, a0, 1) == true);

  // BALLENV_STEP2_WIDE: exactly "0" or "1"
  CHECK(step2_wide_env(nullptr) == -1);
  CHECK(step2_wide_env("") == -1);
  CHECK(step2_wide_env("0") == 0);
  CHECK(step2_wide_env("1") == 1);
  CHECK(step2_wide_env("2") == -1);
  CHECK(step2_wide_env("10") == -1);
  CHECK(step2_wide_env("01") == -1);
  CHECK(step2_wide_env("on") == -1);
  CHECK(STEP_INSTANCE_NONE == 0 && STEP_INSTANCE_PLAIN == 1 && STEP_INSTANCE_WIDE == 2);

  if (fails) return 1;
  printf("step2_wide_host: OK\n");
  return 0;
}
