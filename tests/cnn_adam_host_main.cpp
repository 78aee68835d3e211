// Stand-alone check of be_cnn_adam's host logic in csrc/cnn_host.h (no HIP), built by the host C++ compiler
// alone under ASan + UBSan (tests/test_pixel_adam_host.py):
//   * cnn_pack_dest inverts cnn_pack_source on every element of the 14 parameters, for A in {1, 9, 15};
//   * every image index that holds a parameter is hit exactly once; no pad, -inf or running-statistics
//     index is hit;
//   * cnn_param_at walks the 14 parameters end to end;
//   * the argument checks, each naming its argument;
//   * prints "elems A n" per action count (the update kernel's element count) and one OK line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "cnn_host.h"
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

static bool is_running(int t) { return t % 6 == 4 || t % 6 == 5; }

// the kernel's text, evaluated by the compiler too
static_assert(cnn_pack_dest(CT_CONV1_W, 0) == CNN_F1 && cnn_pack_dest(CT_HEAD_B, 3) == CNN_HBIAS + 3, "cnn_pack_dest");
static_assert(cnn_pack_dest(CT_BN2_W, 5) == CNN_P2 + CNN_C2 + 5 && cnn_pack_dest(CT_BN1_M, 0) == -1, "cnn_pack_dest");
static_assert(cnn_param_tensor(0) == CT_CONV1_W && cnn_param_tensor(7) == CT_BN2_B && cnn_param_tensor(13) == CT_HEAD_B,
              "cnn_param_tensor");

int main() {
  const int As[3] = {1, 9, 15};
  for (int A : As) {
    std::vector<int> hits((size_t)CNN_TOTAL, 0);
    int params = 0, n = 0;
    for (int t = 0; t < CNN_TENSORS; ++t) {
      if (is_running(t)) {
        for (int e = 0; e < cnn_tensor_elems(t, A); ++e) CHECK(cnn_pack_dest(t, e) == -1);
        continue;
      }
      CHECK(cnn_param_tensor(params) == t);
      CHECK(!strcmp(CNN_PARAM_NAMES[params], CNN_TENSOR_NAMES[t]));
      for (int e = 0; e < cnn_tensor_elems(t, A); ++e, ++n) {
        const int dst = cnn_pack_dest(t, e);
        CHECK(dst >= 0 && dst < CNN_TOTAL);
        int elem = -1;
        CHECK(cnn_pack_source(dst, A, &elem) == t && elem == e);
        ++hits[(size_t)dst];
        int at = -1;
        CHECK(cnn_param_at(n, A, &at) == params && at == e);        // the kernel's thread n takes this element
      }
      ++params;
    }
    CHECK(params == CNN_PARAMS && n == cnn_param_elems(A));
    int at = 0;
    CHECK(cnn_param_at(n, A, &at) == -1 && cnn_param_at(n + 255, A, &at) == -1 && cnn_param_at(-1, A, &at) == -1);
    for (int i = 0; i < CNN_TOTAL; ++i) {
      int elem = -1;
      const int src = cnn_pack_source(i, A, &elem);
      const bool param = src >= 0 && !is_running(src);
      CHECK(hits[(size_t)i] == (param ? 1 : 0));                    // pads, -inf and running statistics: never
    }
    printf("elems %d %d\n", A, n);
  }

  // the argument checks, in their order
  float w[8];
  float* all[4][CNN_PARAMS];
  for (auto& set : all)
    for (float*& p : set) p = w;
  auto tensors = [&](int s) {
    float** p = all[s];
    return be_cnn_tensors{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13]};
  };
  const char* const set_names[4] = {"params", "grads", "exp_avg", "exp_avg_sq"};
  const char *set = nullptr, *field = nullptr;
  be_cnn_tensors t[4] = {tensors(0), tensors(1), tensors(2), tensors(3)};
  CHECK(!cnn_adam_sets_error(&t[0], &t[1], &t[2], &t[3], &set, &field));
  CHECK(cnn_bad_param(&t[0]) == -1);
  for (int s = 0; s < 4; ++s) {
    const be_cnn_tensors* ptr[4] = {&t[0], &t[1], &t[2], &t[3]};
    ptr[s] = nullptr;
    CHECK(cnn_adam_sets_error(ptr[0], ptr[1], ptr[2], ptr[3], &set, &field));
    CHECK(!strcmp(set, set_names[s]) && field == nullptr);
    for (int k = 0; k < CNN_PARAMS; ++k) {
      for (int how = 0; how < 2; ++how) {
        all[s][k] = how ? (float*)((char*)w + 2) : nullptr;
        t[s] = tensors(s);
        CHECK(cnn_bad_param(&t[s]) == k);
        CHECK(cnn_adam_sets_error(&t[0], &t[1], &t[2], &t[3], &set, &field));
        CHECK(!strcmp(set, set_names[s]) && !strcmp(field, CNN_PARAM_NAMES[k]));
      }
      all[s][k] = w;
      t[s] = tensors(s);
    }
  }
  // a NULL set is reported ahead of a bad tensor of an earlier set
  all[0][4] = nullptr;
  t[0] = tensors(0);
  CHECK(cnn_adam_sets_error(&t[0], &t[1], nullptr, &t[3], &set, &field) && !strcmp(set, "exp_avg") && !field);
  CHECK(cnn_adam_sets_error(&t[0], &t[1], &t[2], &t[3], &set, &field) && !strcmp(set, "params") &&
        !strcmp(field, "conv2_weight"));

  alignas(8) double state[4], losses[2], log[4];
  CHECK(optim_args_error(state, true, 0.9, 0.999, 1e-8, nullptr, nullptr, 0) == nullptr);
  CHECK(optim_args_error(state, true, 0.0, 0.0, 0.0, losses, log, 2) == nullptr);
  CHECK(says(optim_args_error(nullptr, true, 0.9, 0.999, 1e-8, nullptr, nullptr, 0), "state"));
  CHECK(says(optim_args_error((double*)((char*)state + 4), true, 0.9, 0.999, 1e-8, nullptr, nullptr, 0), "8-byte"));
  CHECK(says(optim_args_error(state, true, 1.0, 0.999, 1e-8, nullptr, nullptr, 0), "beta1"));
  CHECK(says(optim_args_error(state, true, -0.1, 0.999, 1e-8, nullptr, nullptr, 0), "beta1"));
  CHECK(says(optim_args_error(state, true, 0.9, 1.0, 1e-8, nullptr, nullptr, 0), "beta2"));
  CHECK(says(optim_args_error(state, true, 0.9, 0.999, -1e-8, nullptr, nullptr, 0), "eps"));
  CHECK(says(optim_args_error(state, true, 0.9, 0.999, 1e-8, losses, nullptr, 0), "losses and loss_log"));
  CHECK(says(optim_args_error(state, true, 0.9, 0.999, 1e-8, nullptr, log, 2), "losses and loss_log"));
  CHECK(says(optim_args_error(state, true, 0.9, 0.999, 1e-8, (double*)((char*)losses + 4), log, 2), "not 8-byte aligned"));
  CHECK(says(optim_args_error(state, true, 0.9, 0.999, 1e-8, losses, (double*)((char*)log + 4), 2), "not 8-byte aligned"));
  CHECK(says(optim_args_error(state, true, 0.9, 0.999, 1e-8, losses, log, 0), "log_rows"));
  printf("cnn_adam_host: OK\n");
  return 0;
}
