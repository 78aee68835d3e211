// Stand-alone check of be_cnn_grad's host logic in csrc/cnn_grad_host.h (no HIP), built by the host C++
// compiler alone under ASan + UBSan (tests/test_pixel_grad_host.py):
//   * the transposed weights' index function is a bijection onto conv2's and conv3's elements;
//   * a slot's sections neither overlap nor leave its bounds, and the reduce kernel's outputs cover every
//     gradient element exactly once, each with partial sums inside its own section;
//   * the argument checks, each naming its argument, in the header's order;
//   * prints "layout ..." (the constants the Python side mirrors) and one OK line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "cnn_grad_host.h"

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
  {  // the transposed part: every element of conv2 and conv3 exactly once
    std::vector<int> h2((size_t)CNN_G_W2, 0), h3((size_t)CNN_G_W3, 0);
    for (int i = 0; i < CNN_G_PACK - CNN_G_T2; ++i) {
      int elem = -1;
      const int src = cnn_grad_pack_source(i, &elem);
      CHECK(src == (i < CNN_G_T3 - CNN_G_T2 ? CT_CONV2_W : CT_CONV3_W));
      CHECK(elem >= 0 && elem < (src == CT_CONV2_W ? CNN_G_W2 : CNN_G_W3));
      ++(src == CT_CONV2_W ? h2 : h3)[(size_t)elem];
    }
    for (int h : h2) CHECK(h == 1);
    for (int h : h3) CHECK(h == 1);
    // the fragment dy = W^T dconv reads: lane 16 l4 + l15 of (tap, cs, rt) is W[4 cs + l4][16 rt + l15][tap]
    int elem = -1;
    cnn_grad_pack_source(((7 * 8 + 3) * 64) + 16 * 2 + 5, &elem);
    CHECK(elem == ((4 * 3 + 2) * CNN_C1 + 5) * CNN_TAPS + 7);
    cnn_grad_pack_source((CNN_G_T3 - CNN_G_T2) + (((7 * 8 + 3) * 2 + 1) * 64) + 16 * 2 + 5, &elem);
    CHECK(elem == ((4 * 3 + 2) * CNN_C2 + 16 + 5) * CNN_TAPS + 7);
  }
  for (int A = 1; A <= CNN_MAXA; ++A) {
    const CnnGradSlot s = cnn_grad_slot(A);
    CHECK(s.loss_off % 8 == 0 && s.loss_off >= s.floats * 4 && s.slot_bytes % 16 == 0);
    CHECK(s.slot_bytes >= s.loss_off + CNN_GRAD_TILE * 16);
    CHECK(cnn_grad_workspace_bytes(3, A) == (int64_t)CNN_G_PACK * 4 + 3 * (int64_t)s.slot_bytes);
    std::vector<int> used((size_t)s.floats, 0);
    const int sizes[14] = {CNN_G_W1, CNN_C1, CNN_C1, CNN_C1, CNN_G_W2, CNN_C2, CNN_C2, CNN_C2,
                           CNN_G_W3, CNN_C3, CNN_C3, CNN_C3, A * CNN_HEAD_IN, A};
    std::vector<std::vector<int>> hits(14);
    for (int t = 0; t < 14; ++t) hits[t].assign((size_t)sizes[t], 0);
    int total = 0;
    for (int t = 0; t < 14; ++t) total += sizes[t];
    CHECK(total == s.outputs);
    for (int i = 0; i < s.outputs; ++i) {
      const CnnGradOut o = cnn_grad_output(i, A);
      CHECK(o.tensor >= 0 && o.tensor < 14 && o.elem >= 0 && o.elem < sizes[o.tensor]);
      ++hits[o.tensor][(size_t)o.elem];
      const bool bias = o.tensor == 1 || o.tensor == 5 || o.tensor == 9;
      CHECK((o.parts == 0) == bias);
      for (int q = 0; q < o.parts; ++q) {
        const int at = o.off + q * o.stride;
        CHECK(at >= 0 && at < s.floats);
        ++used[(size_t)at];
      }
    }
    for (int t = 0; t < 14; ++t)
      for (int h : hits[t]) CHECK(h == 1);
    // no slot float feeds two outputs; the floats no output reads are head.bias' pads (16 - A per row)
    int unused = 0;
    for (int u : used) { CHECK(u <= 1); unused += u == 0; }
    CHECK(unused == CNN_GRAD_TILE * (CNN_NO - A));
  }

  // the argument checks
  alignas(16) static uint8_t buf[64];
  static float f[4];
  static double d[2];
  be_cnn_weights w{};
  const float** wp = (const float**)&w;
  for (int i = 0; i < CNN_TENSORS; ++i) wp[i] = f;
  w.bn1_running_mean = w.bn1_running_var = w.bn2_running_mean = w.bn2_running_var = nullptr;   // not read
  w.bn3_running_mean = w.bn3_running_var = nullptr;
  be_cnn_grads g{};
  float** gp = (float**)&g;
  for (int i = 0; i < 14; ++i) gp[i] = f;
  g.losses = d;
  const int64_t need = cnn_grad_workspace_bytes(4, 9);
  const char* field = nullptr;
  auto err = [&](const void* im, const void* q, const void* a, int64_t rows, const be_cnn_weights* ww, int32_t A,
                 const void* ws, int64_t wb, const be_cnn_grads* gg) {
    return cnn_grad_args_error(im, q, a, rows, ww, A, ws, wb, gg, 4, &field);
  };
  CHECK(err(buf, buf, buf, 0, &w, 9, buf, need, &g) == nullptr);
  CHECK(err(buf, buf, buf, 5, &w, 9, buf, need, &g) == nullptr);
  CHECK(says(err(nullptr, buf, buf, 1, &w, 9, buf, need, &g), "images is NULL"));
  CHECK(says(err(buf + 8, buf, buf, 1, &w, 9, buf, need, &g), "images must be 16-byte aligned"));
  CHECK(says(err(buf, nullptr, buf, 1, &w, 9, buf, need, &g), "quadrants is NULL"));
  CHECK(says(err(buf, buf, nullptr, 1, &w, 9, buf, need, &g), "actions is NULL"));
  CHECK(says(err(buf, buf, buf, -1, &w, 9, buf, need, &g), "rows must be >= 0"));
  CHECK(says(err(buf, buf, buf, 1, &w, 0, buf, need, &g), "num_actions must be in [1, 15]"));
  CHECK(says(err(buf, buf, buf, 1, &w, 16, buf, need, &g), "num_actions must be in [1, 15]"));
  CHECK(says(err(buf, buf, buf, 1, nullptr, 9, buf, need, &g), "weights is NULL"));
  {
    be_cnn_weights w2 = w;
    w2.conv3_weight = nullptr;
    CHECK(says(err(buf, buf, buf, 1, &w2, 9, buf, need, &g), "weights->%s") && says(field, "conv3_weight"));
    w2 = w;
    w2.bn2_bias = (const float*)((const uint8_t*)f + 2);
    CHECK(says(err(buf, buf, buf, 1, &w2, 9, buf, need, &g), "weights->%s") && says(field, "bn2_bias"));
  }
  CHECK(says(err(buf, buf, buf, 1, &w, 9, buf, need, nullptr), "grads is NULL"));
  {
    be_cnn_grads g2 = g;
    g2.head_bias = nullptr;
    CHECK(says(err(buf, buf, buf, 1, &w, 9, buf, need, &g2), "grads->%s") && says(field, "head_bias"));
    g2 = g;
    g2.losses = nullptr;
    CHECK(says(err(buf, buf, buf, 1, &w, 9, buf, need, &g2), "grads->losses"));
    g2 = g;
    g2.probs = (float*)((uint8_t*)f + 1);
    CHECK(says(err(buf, buf, buf, 1, &w, 9, buf, need, &g2), "grads->probs"));
    g2.probs = f;
    CHECK(err(buf, buf, buf, 1, &w, 9, buf, need, &g2) == nullptr);
  }
  CHECK(says(err(buf, buf, buf, 1, &w, 9, nullptr, need, &g), "workspace is NULL"));
  CHECK(says(err(buf, buf, buf, 1, &w, 9, buf + 8, need, &g), "workspace is NULL or not 16-byte aligned"));
  CHECK(says(err(buf, buf, buf, 1, &w, 9, buf, need - 1, &g), "workspace is smaller"));
  // the first failing check wins, in the header's order
  CHECK(says(err(nullptr, nullptr, nullptr, -1, nullptr, 0, nullptr, 0, nullptr), "images is NULL"));
  CHECK(says(err(buf, buf, buf, -1, nullptr, 0, nullptr, 0, nullptr), "rows"));

  const CnnGradSlot s9 = cnn_grad_slot(9);
  printf("layout tile %d waves %d max_slots %d pack %d slot_bytes %d outputs %d lds %d\n", CNN_GRAD_TILE, CNN_GRAD_WAVES,
         CNN_GRAD_MAX_SLOTS, CNN_G_PACK, s9.slot_bytes, s9.outputs, CNN_GRAD_LDS_BYTES);
  printf("cnn_grad_host: OK\n");
  return 0;
}
