// Stand-alone check of be_cnn_*'s host logic in csrc/cnn_host.h (no HIP), built by the host C++ compiler
// alone under ASan + UBSan (tests/test_pixel_policy_host.py):
//   * the packed image's index function is a bijection onto the unpadded weights, for every action
//     count, and its pads are where the layout says;
//   * the argument checks, each naming its argument;
//   * prints "layout ..." (the constants the Python side mirrors) and one OK line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "cnn_host.h"

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
  for (int A = 1; A <= CNN_MAXA; ++A) {
    std::vector<std::vector<int>> hits(CNN_TENSORS);
    for (int t = 0; t < CNN_TENSORS; ++t) hits[t].assign((size_t)cnn_tensor_elems(t, A), 0);
    int zeros = 0, neginf = 0;
    for (int i = 0; i < CNN_TOTAL; ++i) {
      int elem = -1;
      const int src = cnn_pack_source(i, A, &elem);
      if (src == CNN_SRC_ZERO) { ++zeros; continue; }
      if (src == CNN_SRC_NEGINF) { CHECK(i >= CNN_HB + A && i < CNN_HB + CNN_NO - 1); ++neginf; continue; }
      CHECK(src >= 0 && src < CNN_TENSORS);
      CHECK(elem >= 0 && elem < cnn_tensor_elems(src, A));
      ++hits[src][(size_t)elem];
      // a fragment section holds its own tensor only
      if (i < CNN_FH) CHECK(src == CT_CONV1_W);
      else if (i < CNN_PR) CHECK(src == CT_HEAD_W);
      else if (i >= CNN_F3) CHECK(src == CT_CONV3_W);
      else if (i >= CNN_F2) CHECK(src == CT_CONV2_W);
    }
    int64_t elems = 0;
    for (int t = 0; t < CNN_TENSORS; ++t) {
      for (int h : hits[t]) CHECK(h == 1);              // every weight exactly once
      elems += cnn_tensor_elems(t, A);
    }
    CHECK(neginf == CNN_NO - 1 - A);
    CHECK(elems + zeros + neginf == CNN_TOTAL);
    // conv1's K 75 -> 76 (16 zero weights), the head's rows A..15, the head bias's, hb's zeros
    CHECK(zeros == CNN_C1 + (CNN_NO - A) * CNN_HEAD_IN + (CNN_NO - A) + A + 1);
  }
  CHECK(CNN_TILE * CNN_N1 % 16 == 0 && CNN_TILE * CNN_N3 == 16 && CNN_K1 * 4 == CNN_C0 * CNN_TAPS + 1);
  CHECK(CNN_K2 * 4 == CNN_C1 * CNN_TAPS && CNN_K3 * 4 == CNN_C2 * CNN_TAPS && CNN_KH * 4 == CNN_HEAD_IN);
  CHECK(cnn_tensor_elems(CT_CONV3_W, 9) == 25600 && cnn_tensor_elems(CT_BN1_V, 9) == 16 && cnn_tensor_elems(CT_BN3_M, 9) == 32);
  printf("layout tile %d waves %d total %d staged %d lds %d\n", CNN_TILE, CNN_WAVES, CNN_TOTAL, CNN_STAGED, CNN_LDS_BYTES);

  // the argument checks, in their order
  CHECK(cnn_create_args_error(1) == nullptr && cnn_create_args_error(9) == nullptr && cnn_create_args_error(15) == nullptr);
  CHECK(says(cnn_create_args_error(0), "num_actions") && says(cnn_create_args_error(16), "num_actions"));
  CHECK(says(cnn_create_args_error(-3), "num_actions"));
  alignas(16) uint8_t image[64];
  uint8_t action[4];
  float value[4];
  const be_act_out ok{action, nullptr, nullptr, nullptr};
  CHECK(cnn_act_args_error(image, BE_CNN_NORM_SAMPLE, &ok) == nullptr);
  CHECK(cnn_act_args_error(image + 16, BE_CNN_NORM_RUNNING, &ok) == nullptr);
  CHECK(says(cnn_act_args_error(nullptr, BE_CNN_NORM_SAMPLE, &ok), "image"));
  CHECK(says(cnn_act_args_error(image + 4, BE_CNN_NORM_SAMPLE, &ok), "image"));
  CHECK(says(cnn_act_args_error(image + 4, BE_CNN_NORM_SAMPLE, &ok), "16-byte"));
  CHECK(says(cnn_act_args_error(image, 2, &ok), "norm") && says(cnn_act_args_error(image, -1, &ok), "norm"));
  const be_act_out with_value{action, nullptr, value, nullptr};
  CHECK(says(cnn_act_args_error(image, BE_CNN_NORM_SAMPLE, &with_value), "value"));
  const be_act_out no_action{nullptr, value, nullptr, nullptr};
  CHECK(says(cnn_act_args_error(image, BE_CNN_NORM_SAMPLE, &no_action), "action"));
  CHECK(says(cnn_act_args_error(image, BE_CNN_NORM_SAMPLE, nullptr), "action"));

  float w[8];
  const float* all[CNN_TENSORS];
  for (int t = 0; t < CNN_TENSORS; ++t) all[t] = w;
  auto weights = [&]() {
    return be_cnn_weights{all[0], all[1], all[2], all[3], all[4], all[5], all[6], all[7], all[8], all[9],
                          all[10], all[11], all[12], all[13], all[14], all[15], all[16], all[17], all[18], all[19]};
  };
  be_cnn_weights bw = weights();
  CHECK(cnn_bad_tensor(&bw) == -1);
  for (int t = 0; t < CNN_TENSORS; ++t) {
    all[t] = nullptr;
    bw = weights();
    CHECK(cnn_bad_tensor(&bw) == t);
    all[t] = (const float*)((const char*)w + 2);
    bw = weights();
    CHECK(cnn_bad_tensor(&bw) == t);
    all[t] = w;
  }
  CHECK(!strcmp(CNN_TENSOR_NAMES[CT_BN2_V], "bn2_running_var") && !strcmp(CNN_TENSOR_NAMES[CT_HEAD_B], "head_bias"));
  printf("cnn_host: OK\n");
  return 0;
}
