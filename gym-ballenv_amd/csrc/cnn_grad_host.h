// cnn_grad_host.h -- be_cnn_grad's host side that needs no HIP (cnn_host.h's sibling): the work split, the
// workspace's layout (the packed weights, then one slot of partial sums per workgroup), the kernel's LDS and
// the entry's argument checks.  Only ballenv.h, cnn_host.h (itself only ballenv.h) and standard headers, so
// the host C++ compiler alone builds and tests it (tests/cnn_grad_host_main.cpp); the layout functions are
// constexpr, so the kernels of cnn_grad.hip use the same text.
#pragma once
#include <stdint.h>

#include "ballenv.h"
#include "cnn_host.h"

namespace behost {

// cnn_grad_kernel's work split: a persistent grid of one workgroup per compute unit, at most
// CNN_GRAD_MAX_SLOTS, CNN_GRAD_WAVES waves each; a workgroup takes CNN_GRAD_TILE rows per round (tile t of G
// workgroups: workgroup t % G, round t / G).
constexpr int CNN_GRAD_TILE = 2, CNN_GRAD_WAVES = 8, CNN_GRAD_MAX_SLOTS = 1024;

// The workspace, in floats.  First the packed weights, written by the pack kernel on every call:
//   [0, CNN_TOTAL)  be_cnn_act's image (cnn_host.h; the running statistics' places hold zeros)
//   CNN_G_T2        conv2 transposed, [tap][cs][64]: lane l = 16 l4 + l15 holds W2[co = 4 cs + l4][ci = l15][tap]
//   CNN_G_T3        conv3 transposed, [tap][cs][rt][64]: W3[co = 4 cs + l4][ci = 16 rt + l15][tap]
// (the A fragments of dy = W^T dconv: row = input channel, k = output channel).  Then the slots.
constexpr int CNN_G_T2 = CNN_TOTAL;
constexpr int CNN_G_T3 = CNN_G_T2 + CNN_TAPS * 8 * 64;
constexpr int CNN_G_PACK = CNN_G_T3 + CNN_TAPS * 8 * 2 * 64;
static_assert(CNN_G_PACK % 4 == 0, "the slots start 16-byte aligned");

// which element of conv2 / conv3 float i of the transposed part holds (i relative to CNN_G_T2)
constexpr int cnn_grad_pack_source(int i, int* elem) {
  const bool third = i >= CNN_G_T3 - CNN_G_T2;
  const int j = third ? i - (CNN_G_T3 - CNN_G_T2) : i;
  const int lane = j & 63, t = j >> 6, rt = third ? (t & 1) : 0, u = third ? (t >> 1) : t, cs = u & 7, tap = u >> 3;
  const int co = 4 * cs + (lane >> 4), ci = 16 * rt + (lane & 15);
  *elem = (co * (third ? CNN_C2 : CNN_C1) + ci) * CNN_TAPS + tap;
  return third ? CT_CONV3_W : CT_CONV2_W;
}

// A workgroup's slot (offsets in floats; the two f64 loss partials per row of a tile at loss_off bytes).
// A gradient with PARTS > 1 is held as that many partial sums, which the reduce kernel adds in order:
//   conv1.weight  one per wave (wave w takes the positions 4 s + l4 of the steps s = w, w + 8, ...)
//   the BatchNorm vectors and head.bias  one per row of the tile
struct CnnGradSlot {
  int32_t o_w1, o_w2, o_w3, o_wh, o_bh, o_g1, o_b1, o_g2, o_b2, o_g3, o_b3, floats;
  int32_t loss_off, slot_bytes;                   // bytes
  int32_t outputs;                                // gradient elements be_cnn_grad writes, the conv biases included
};
constexpr int CNN_G_W1 = CNN_C1 * CNN_C0 * CNN_TAPS, CNN_G_W2 = CNN_C2 * CNN_C1 * CNN_TAPS, CNN_G_W3 = CNN_C3 * CNN_C2 * CNN_TAPS;
constexpr CnnGradSlot cnn_grad_slot(int A) {
  CnnGradSlot s{};
  s.o_w1 = 0;                                           // [WAVES][16][75]
  s.o_w2 = s.o_w1 + CNN_GRAD_WAVES * CNN_G_W1;          // [32][16][25]
  s.o_w3 = s.o_w2 + CNN_G_W2;                           // [32][32][25]
  s.o_wh = s.o_w3 + CNN_G_W3;                           // [A][132]
  s.o_bh = s.o_wh + A * CNN_HEAD_IN;                    // [TILE][16]
  s.o_g1 = s.o_bh + CNN_GRAD_TILE * CNN_NO;             // [TILE][16] gamma, then beta
  s.o_b1 = s.o_g1 + CNN_GRAD_TILE * CNN_C1;
  s.o_g2 = s.o_b1 + CNN_GRAD_TILE * CNN_C1;             // [TILE][32]
  s.o_b2 = s.o_g2 + CNN_GRAD_TILE * CNN_C2;
  s.o_g3 = s.o_b2 + CNN_GRAD_TILE * CNN_C2;
  s.o_b3 = s.o_g3 + CNN_GRAD_TILE * CNN_C3;
  s.floats = s.o_b3 + CNN_GRAD_TILE * CNN_C3;
  s.loss_off = (s.floats * 4 + 7) / 8 * 8;
  s.slot_bytes = (s.loss_off + CNN_GRAD_TILE * 2 * 8 + 15) / 16 * 16;
  s.outputs = CNN_G_W1 + CNN_G_W2 + CNN_G_W3 + A * CNN_HEAD_IN + A + 3 * CNN_C1 + 3 * CNN_C2 + 3 * CNN_C3;
  return s;
}
constexpr int64_t cnn_grad_workspace_bytes(int slots, int A) {
  return (int64_t)CNN_G_PACK * 4 + (int64_t)slots * cnn_grad_slot(A).slot_bytes;
}

// One output element of the reduce kernel: gradient tensor `tensor` (be_cnn_grads' field order, 0..13),
// element `elem`; its partial sums are slot[off + q * stride] for q < parts (parts = 0: a conv bias, exact +0).
struct CnnGradOut { int32_t tensor, elem, off, parts, stride; };
constexpr CnnGradOut cnn_grad_output(int i, int A) {
  const CnnGradSlot s = cnn_grad_slot(A);
  // be_cnn_grads' order: conv1 w, b, bn1 w, b, conv2 ..., conv3 ..., head w, b
  const int n[14] = {CNN_G_W1, CNN_C1, CNN_C1, CNN_C1, CNN_G_W2, CNN_C2, CNN_C2, CNN_C2,
                     CNN_G_W3, CNN_C3, CNN_C3, CNN_C3, A * CNN_HEAD_IN, A};
  const int off[14] = {s.o_w1, 0, s.o_g1, s.o_b1, s.o_w2, 0, s.o_g2, s.o_b2, s.o_w3, 0, s.o_g3, s.o_b3, s.o_wh, s.o_bh};
  const int parts[14] = {CNN_GRAD_WAVES, 0, CNN_GRAD_TILE, CNN_GRAD_TILE, 1, 0, CNN_GRAD_TILE, CNN_GRAD_TILE,
                         1, 0, CNN_GRAD_TILE, CNN_GRAD_TILE, 1, CNN_GRAD_TILE};
  const int stride[14] = {CNN_G_W1, 0, CNN_C1, CNN_C1, 0, 0, CNN_C2, CNN_C2, 0, 0, CNN_C3, CNN_C3, 0, CNN_NO};
  int t = 0, e = i;
  while (t < 13 && e >= n[t]) { e -= n[t]; ++t; }
  return CnnGradOut{t, e, off[t] + e, parts[t], stride[t]};
}

// The grad kernel's LDS (offsets in floats behind the staged image part, as the act kernel's)
constexpr int CNN_GL_LUT = CNN_STAGED;                                       // [256] v / 255.0f
constexpr int CNN_GL_X1 = CNN_GL_LUT + 256;                                  // [TILE][16][324] conv1 -> xhat1 -> dconv1
constexpr int CNN_GL_Y1 = CNN_GL_X1 + CNN_GRAD_TILE * CNN_C1 * CNN_N1;       // y1 -> dy1
constexpr int CNN_GL_X2 = CNN_GL_Y1 + CNN_GRAD_TILE * CNN_C1 * CNN_N1;       // [TILE][32][49]
constexpr int CNN_GL_Y2 = CNN_GL_X2 + CNN_GRAD_TILE * CNN_C2 * CNN_N2;
constexpr int CNN_GL_X3 = CNN_GL_Y2 + CNN_GRAD_TILE * CNN_C2 * CNN_N2;       // [TILE][128]
constexpr int CNN_GL_Y3 = CNN_GL_X3 + CNN_GRAD_TILE * CNN_FEAT;
constexpr int CNN_GL_INV = CNN_GL_Y3 + CNN_GRAD_TILE * CNN_FEAT;             // 1 / sqrt(var + eps) of every map: [TILE][16], [TILE][32] x 2
constexpr int CNN_GL_PART = CNN_GL_INV + CNN_GRAD_TILE * (CNN_C1 + CNN_C2 + CNN_C3);   // conv3's partial chains [2][8][64][4]
constexpr int CNN_GL_ZS = CNN_GL_PART + 2 * 8 * 64 * 4;                      // [TILE][CNN_ZP] logits (48 floats)
constexpr int CNN_GL_PR = CNN_GL_ZS + 48;                                    // [TILE][16] probabilities
constexpr int CNN_GL_DZ = CNN_GL_PR + CNN_GRAD_TILE * CNN_NO;                // [TILE][16] dz
constexpr int CNN_GL_ROW = CNN_GL_DZ + CNN_GRAD_TILE * CNN_NO;               // [TILE] i32 quadrant (16 floats)
constexpr int CNN_GL_IMG = CNN_GL_ROW + 16;                                  // [TILE][3][40][40] u8
constexpr int CNN_GRAD_LDS_BYTES = (CNN_GL_IMG + CNN_GRAD_TILE * CNN_IMG_BYTES / 4) * 4;
static_assert(CNN_GRAD_TILE * CNN_ZP <= 48 && CNN_GL_IMG % 4 == 0 && CNN_GRAD_LDS_BYTES <= 160 * 1024, "the grad kernel's LDS");

// be_cnn_grads' 14 gradient pointers in field order
inline void cnn_grad_pointers(const be_cnn_grads* g, float* (&p)[14]) {
  float* const q[14] = {g->conv1_weight, g->conv1_bias, g->bn1_weight, g->bn1_bias, g->conv2_weight, g->conv2_bias,
                        g->bn2_weight, g->bn2_bias, g->conv3_weight, g->conv3_bias, g->bn3_weight, g->bn3_bias,
                        g->head_weight, g->head_bias};
  for (int i = 0; i < 14; ++i) p[i] = q[i];
}
constexpr const char* const CNN_GRAD_NAMES[14] = {
    "conv1_weight", "conv1_bias", "bn1_weight", "bn1_bias", "conv2_weight", "conv2_bias", "bn2_weight", "bn2_bias",
    "conv3_weight", "conv3_bias", "bn3_weight", "bn3_bias", "head_weight", "head_bias"};
// the first of the 14 weights be_cnn_grad reads (the running statistics are not among them) that is NULL or
// not 4-byte aligned, as its name, or NULL
inline const char* cnn_grad_bad_weight(const be_cnn_weights* w) {
  const float* const p[14] = {w->conv1_weight, w->conv1_bias, w->bn1_weight, w->bn1_bias, w->conv2_weight, w->conv2_bias,
                              w->bn2_weight, w->bn2_bias, w->conv3_weight, w->conv3_bias, w->bn3_weight, w->bn3_bias,
                              w->head_weight, w->head_bias};
  for (int i = 0; i < 14; ++i)
    if (!p[i] || ((uintptr_t)p[i] & 3)) return CNN_GRAD_NAMES[i];
  return nullptr;
}
inline const char* cnn_grad_bad_grad(const be_cnn_grads* g) {
  float* p[14];
  cnn_grad_pointers(g, p);
  for (int i = 0; i < 14; ++i)
    if (!p[i] || ((uintptr_t)p[i] & 3)) return CNN_GRAD_NAMES[i];
  return nullptr;
}

// The entry's argument checks that need no device, in this order; NULL: fine, else the message (each
// names its argument; a weight or gradient tensor's name goes behind "weights->" / "grads->").
// slots: the workgroups of the grid (>= 1).  *field: the tensor's name for the two messages that end in "%s".
inline const char* cnn_grad_args_error(const void* images, const void* quadrants, const void* actions, int64_t rows,
                                       const be_cnn_weights* weights, int32_t num_actions, const void* workspace,
                                       int64_t workspace_bytes, const be_cnn_grads* grads, int slots,
                                       const char** field) {
  *field = nullptr;
  if (!images) return "be_cnn_grad: images is NULL";
  if ((uintptr_t)images & 15) return "be_cnn_grad: images must be 16-byte aligned";
  if (!quadrants) return "be_cnn_grad: quadrants is NULL";
  if (!actions) return "be_cnn_grad: actions is NULL";
  if (rows < 0) return "be_cnn_grad: rows must be >= 0";
  if (num_actions < 1 || num_actions > CNN_MAXA) return "be_cnn_grad: num_actions must be in [1, 15]";
  if (!weights) return "be_cnn_grad: weights is NULL";
  if ((*field = cnn_grad_bad_weight(weights))) return "be_cnn_grad: weights->%s is NULL or not 4-byte aligned";
  if (!grads) return "be_cnn_grad: grads is NULL";
  if ((*field = cnn_grad_bad_grad(grads))) return "be_cnn_grad: grads->%s is NULL or not 4-byte aligned";
  if (!grads->losses || ((uintptr_t)grads->losses & 7)) return "be_cnn_grad: grads->losses is NULL or not 8-byte aligned";
  if (grads->probs && ((uintptr_t)grads->probs & 3)) return "be_cnn_grad: grads->probs is not 4-byte aligned";
  if (!workspace || ((uintptr_t)workspace & 15)) return "be_cnn_grad: workspace is NULL or not 16-byte aligned";
  if (workspace_bytes < cnn_grad_workspace_bytes(slots, num_actions))
    return "be_cnn_grad: workspace is smaller than be_cnn_grad_workspace_bytes";
  return nullptr;
}

}  // namespace behost
