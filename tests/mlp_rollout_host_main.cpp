// Stand-alone check of be_mlp_rollout's host logic in csrc/host_logic.h (no HIP), built by the host C++
// compiler alone under ASan + UBSan (tests/test_mlp_rollout_host.py):
//   * prints "waves N CUS LAYERS -> NW" for every row of the table given on the command line as
//     N:CUS:LAYERS arguments (the test compares them against its own table);
//   * checks BALLENV_MLP_ROLLOUT_WAVES's parse and the argument checks that need no device;
//   * prints one OK line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>

#include "host_logic.h"

using namespace behost;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

static bool says(const char* msg, const char* part) { return msg && strstr(msg, part); }

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    long long n = 0;
    int cus = 0, layers = 0;
    CHECK(sscanf(argv[i], "%lld:%d:%d", &n, &cus, &layers) == 3);
    printf("waves %lld %d %d -> %d\n", n, cus, layers, mlp_rollout_waves((int64_t)n, cus, layers));
  }
  // a forced value wins over the rule, 0 (the loop) included
  for (const int f : {0, 1, 2, 4, 8}) CHECK(mlp_rollout_waves(65536, 256, 3, f) == f && mlp_rollout_waves(1, 256, 2, f) == f);
  CHECK(mlp_rollout_waves(65536, 256, 3, -1) == mlp_rollout_waves(65536, 256, 3));
  // the variable: exactly one of 0, 1, 2, 4, 8
  CHECK(mlp_rollout_waves_env(nullptr) == -1 && mlp_rollout_waves_env("") == -1);
  for (const char* v : {"0", "1", "2", "4", "8"}) CHECK(mlp_rollout_waves_env(v) == v[0] - '0');
  for (const char* v : {"3", "5", "16", "-1", "8 ", " 8", "x", "08"}) CHECK(mlp_rollout_waves_env(v) == -1);

  // the argument checks, in their order
  double reward[1];
  uint8_t done[1], action[1];
  alignas(16) uint8_t obs[32];
  float f32[1];
  be_out out{};
  out.reward = reward; out.done = done;
  be_act_out act{};
  act.action = action;
  CHECK(mlp_rollout_args_error(obs, 3, &out, &act) == nullptr);
  CHECK(mlp_rollout_args_error(obs, 0, &out, &act) == nullptr);
  CHECK(says(mlp_rollout_args_error(obs, -1, &out, &act), "steps"));
  CHECK(says(mlp_rollout_args_error(obs, 1, nullptr, &act), "out->reward"));
  CHECK(says(mlp_rollout_args_error(obs, 1, &out, nullptr), "act->action"));
  CHECK(says(mlp_rollout_args_error(nullptr, 1, &out, &act), "obs_last"));
  CHECK(says(mlp_rollout_args_error(obs + 4, 1, &out, &act), "16-byte"));
  { be_out o = out; o.reward = nullptr; CHECK(says(mlp_rollout_args_error(obs, 1, &o, &act), "out->reward")); }
  { be_out o = out; o.done = nullptr; CHECK(says(mlp_rollout_args_error(obs, 1, &o, &act), "out->done")); }
  { be_out o = out; o.obs = obs; CHECK(says(mlp_rollout_args_error(obs, 1, &o, &act), "out->obs")); }
  { be_out o = out; o.obs_f32 = f32; CHECK(says(mlp_rollout_args_error(obs, 1, &o, &act), "obs_f32")); }
  { be_out o = out; o.terminal_obs = obs; CHECK(says(mlp_rollout_args_error(obs, 1, &o, &act), "terminal_obs")); }
  { be_act_out a = act; a.action = nullptr; CHECK(says(mlp_rollout_args_error(obs, 1, &out, &a), "act->action")); }
  { be_act_out a = act; a.value = f32; CHECK(says(mlp_rollout_args_error(obs, 1, &out, &a), "act->value")); }
  { be_act_out a = act; a.probs = f32; CHECK(says(mlp_rollout_args_error(obs, 1, &out, &a), "act->probs")); }
  { be_out o = out; double st[8]; o.stats = st; o.truncated = done; CHECK(mlp_rollout_args_error(obs, 1, &o, &act) == nullptr); }
  printf("mlp_rollout_host: OK\n");
  return 0;
}
