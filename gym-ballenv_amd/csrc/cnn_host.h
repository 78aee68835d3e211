// cnn_host.h -- be_cnn_*'s host side that needs no HIP (pixels_host.h's and host_logic.h's sibling):
// the pixel agent's network shape, the packed weight image's layout, its index function and that
// function's inverse (be_cnn_adam's scatter), and the entries' argument checks.  Only ballenv.h and
// standard headers, so the host C++ compiler alone builds and tests it (tests/cnn_host_main.cpp,
// tests/cnn_adam_host_main.cpp); the layout functions are constexpr, so the kernels of cnn_policy.hip
// use the same text.
#pragma once
#include <stdint.h>

#include "ballenv.h"

namespace behost {

// Policy of examples/ball_cnn_reinforce.py:60-83: the reference's only shape.
constexpr int CNN_IMG = 40, CNN_C0 = 3, CNN_KS = 5, CNN_TAPS = 25;
constexpr int CNN_C1 = 16, CNN_S1 = 18, CNN_N1 = 324;    // conv1: channels, side, positions
constexpr int CNN_C2 = 32, CNN_S2 = 7, CNN_N2 = 49;
constexpr int CNN_C3 = 32, CNN_S3 = 2, CNN_N3 = 4;
constexpr int CNN_FEAT = CNN_C3 * CNN_N3, CNN_HEAD_IN = CNN_FEAT + 4;   // 128 features + the quadrant one-hot
constexpr int CNN_MAXA = 15, CNN_NO = 16;                // be_mlp_create's action bound: policy_finish<16>
constexpr int CNN_IMG_BYTES = CNN_C0 * CNN_IMG * CNN_IMG;
constexpr int CNN_TENSORS = 20;

// cnn_act_kernel's work split: a persistent grid of one workgroup per compute unit, CNN_WAVES waves
// each; a workgroup takes CNN_TILE envs per round (tile t of G workgroups: workgroup t % G, round t / G).
constexpr int CNN_TILE = 4, CNN_WAVES = 8;

// be_cnn_weights' fields in order (the index of a tensor in the pack's pointer table)
enum CnnTensor {
  CT_CONV1_W, CT_CONV1_B, CT_BN1_W, CT_BN1_B, CT_BN1_M, CT_BN1_V,
  CT_CONV2_W, CT_CONV2_B, CT_BN2_W, CT_BN2_B, CT_BN2_M, CT_BN2_V,
  CT_CONV3_W, CT_CONV3_B, CT_BN3_W, CT_BN3_B, CT_BN3_M, CT_BN3_V,
  CT_HEAD_W, CT_HEAD_B
};
constexpr const char* const CNN_TENSOR_NAMES[CNN_TENSORS] = {
    "conv1_weight", "conv1_bias", "bn1_weight", "bn1_bias", "bn1_running_mean", "bn1_running_var",
    "conv2_weight", "conv2_bias", "bn2_weight", "bn2_bias", "bn2_running_mean", "bn2_running_var",
    "conv3_weight", "conv3_bias", "bn3_weight", "bn3_bias", "bn3_running_mean", "bn3_running_var",
    "head_weight", "head_bias"};
constexpr int cnn_tensor_elems(int t, int A) {
  switch (t) {
    case CT_CONV1_W: return CNN_C1 * CNN_C0 * CNN_TAPS;
    case CT_CONV2_W: return CNN_C2 * CNN_C1 * CNN_TAPS;
    case CT_CONV3_W: return CNN_C3 * CNN_C2 * CNN_TAPS;
    case CT_HEAD_W: return A * CNN_HEAD_IN;
    case CT_HEAD_B: return A;
    default: return t < CT_CONV2_W ? CNN_C1 : CNN_C2;     // a layer's bias and its four BatchNorm vectors
  }
}

// The packed image (offsets in floats).  A fragment is the A operand of one v_mfma_f32_16x16x4_f32:
// 64 floats, lane l = 16 l4 + l15 holding W[row 16 rt + l15][k of (step, l4)].  The k of a step:
//   conv1   steps 0..14: (ci, ky) = (s / 5, s % 5), kx = l4; steps 15..18: kx = 4 and
//           (ci, ky) = (j / 5, j % 5) of j = 4 (s - 15) + l4, j = 15 a zero weight (K 75 -> 76)
//   conv2/3 step s = 25 cg + tap: input channel 4 cg + l4, (ky, kx) = (tap / 5, tap % 5)
//   head    step s: input 4 s + l4 of [flatten(y3), one_hot(quadrant)]; rows >= num_actions zero
// The first CNN_STAGED floats are what the act kernel stages in LDS; conv2's and conv3's fragments
// it reads from global memory, 256 contiguous bytes per wave and fragment.
constexpr int CNN_K1 = 19, CNN_K2 = 100, CNN_K3 = 200, CNN_KH = CNN_HEAD_IN / 4;
constexpr int CNN_F1 = 0;                                  // [CNN_K1][64]
constexpr int CNN_FH = CNN_F1 + CNN_K1 * 64;               // [CNN_KH][64]
constexpr int CNN_PR = CNN_FH + CNN_KH * 64;               // the per-channel vectors, below
constexpr int CNN_P1 = CNN_PR;                             // [5][16]: conv bias, gamma, beta, running mean, running var
constexpr int CNN_P2 = CNN_P1 + 5 * CNN_C1;                // [5][32]
constexpr int CNN_P3 = CNN_P2 + 5 * CNN_C2;                // [5][32]
constexpr int CNN_HBIAS = CNN_P3 + 5 * CNN_C3;             // [16] head bias, 0 behind num_actions
constexpr int CNN_HB = CNN_HBIAS + CNN_NO;                 // [16] 0 for an action (and slot 15), -inf for a pad action
constexpr int CNN_STAGED = CNN_HB + CNN_NO;
constexpr int CNN_F2 = CNN_STAGED;                         // [CNN_K2][2 row tiles][64]
constexpr int CNN_F3 = CNN_F2 + CNN_K2 * 2 * 64;           // [CNN_K3][2 row tiles][64]
constexpr int CNN_TOTAL = CNN_F3 + CNN_K3 * 2 * 64;
static_assert(CNN_STAGED % 4 == 0 && CNN_TOTAL % 4 == 0, "the image is staged in 16-byte words");

constexpr int CNN_SRC_ZERO = -1, CNN_SRC_NEGINF = -2;
// The image's index function, as the pack kernel needs it: which element of which tensor image float
// i holds (the tensor's CnnTensor id, *elem its flat state_dict index), or CNN_SRC_ZERO / CNN_SRC_NEGINF
// for a pad.  Onto the tensors' elements it is a bijection (tests/cnn_host_main.cpp).
constexpr int cnn_pack_source(int i, int A, int* elem) {
  *elem = 0;
  if (i < CNN_FH) {
    const int s = i >> 6, lane = i & 63, m = lane & 15, l4 = lane >> 4;
    int ci = s / 5, ky = s % 5, kx = l4;
    if (s >= 15) {
      const int j = 4 * (s - 15) + l4;
      if (j >= 15) return CNN_SRC_ZERO;
      ci = j / 5; ky = j % 5; kx = 4;
    }
    *elem = ((m * CNN_C0 + ci) * CNN_KS + ky) * CNN_KS + kx;
    return CT_CONV1_W;
  }
  if (i < CNN_PR) {
    const int j = i - CNN_FH, s = j >> 6, lane = j & 63, m = lane & 15, k = 4 * s + (lane >> 4);
    if (m >= A) return CNN_SRC_ZERO;
    *elem = m * CNN_HEAD_IN + k;
    return CT_HEAD_W;
  }
  if (i < CNN_HBIAS) {
    const int layer = i < CNN_P2 ? 0 : (i < CNN_P3 ? 1 : 2);
    const int C = layer == 0 ? CNN_C1 : CNN_C2;
    const int j = i - (layer == 0 ? CNN_P1 : (layer == 1 ? CNN_P2 : CNN_P3));
    *elem = j % C;
    // row 0 the conv bias, rows 1..4 the BatchNorm vectors: the tensors' order in be_cnn_weights
    return 6 * layer + 1 + j / C;
  }
  if (i < CNN_HB) {
    const int m = i - CNN_HBIAS;
    if (m >= A) return CNN_SRC_ZERO;
    *elem = m;
    return CT_HEAD_B;
  }
  if (i < CNN_STAGED) {
    const int m = i - CNN_HB;
    return (m < A || m == CNN_NO - 1) ? CNN_SRC_ZERO : CNN_SRC_NEGINF;
  }
  const bool third = i >= CNN_F3;
  const int j = i - (third ? CNN_F3 : CNN_F2), lane = j & 63, t = j >> 6, rt = t & 1, s = t >> 1;
  const int m = 16 * rt + (lane & 15), ci = 4 * (s / CNN_TAPS) + (lane >> 4), tap = s % CNN_TAPS;
  *elem = (m * (third ? CNN_C2 : CNN_C1) + ci) * CNN_TAPS + tap;
  return third ? CT_CONV3_W : CT_CONV2_W;
}

// be_cnn_tensors' fields in order: the 14 parameters, be_cnn_weights without the six running statistics.
constexpr int CNN_PARAMS = 14;
constexpr const char* const CNN_PARAM_NAMES[CNN_PARAMS] = {
    "conv1_weight", "conv1_bias", "bn1_weight", "bn1_bias", "conv2_weight", "conv2_bias", "bn2_weight", "bn2_bias",
    "conv3_weight", "conv3_bias", "bn3_weight", "bn3_bias", "head_weight", "head_bias"};
// parameter k's CnnTensor id: four per layer, then the head's two
constexpr int cnn_param_tensor(int k) { return k < 12 ? 6 * (k >> 2) + (k & 3) : k + 6; }
// Element i of the 14 parameters laid end to end in that order: its parameter, *elem its flat state_dict
// index; -1 behind the last.  Compares against the running ends, which but for the head's are constants.
constexpr int cnn_param_at(int i, int A, int* elem) {
  int k = -1, lo = 0, end = 0;
  for (int q = 0; q < CNN_PARAMS; ++q) {
    const int next = end + cnn_tensor_elems(cnn_param_tensor(q), A);
    const bool in = i >= end && i < next;
    k = in ? q : k;
    lo = in ? end : lo;
    end = next;
  }
  *elem = i - lo;
  return k;
}
constexpr int cnn_param_elems(int A) {
  int n = 0;
  for (int q = 0; q < CNN_PARAMS; ++q) n += cnn_tensor_elems(cnn_param_tensor(q), A);
  return n;
}
// cnn_pack_source inverted: the one image index that holds element elem of tensor t (a CnnTensor id), as
// be_cnn_adam's update kernel scatters it; -1 for a running statistic, which is no parameter.
constexpr int cnn_pack_dest(int t, int elem) {
  if (t == CT_CONV1_W) {
    const int m = elem / (CNN_C0 * CNN_TAPS), r = elem % (CNN_C0 * CNN_TAPS);
    const int j = r / CNN_KS, kx = r % CNN_KS;              // j = 5 ci + ky
    const int s = kx < 4 ? j : 15 + j / 4, l4 = kx < 4 ? kx : j % 4;
    return CNN_F1 + s * 64 + l4 * 16 + m;
  }
  if (t == CT_CONV2_W || t == CT_CONV3_W) {
    const int cin = t == CT_CONV2_W ? CNN_C1 : CNN_C2;
    const int tap = elem % CNN_TAPS, mc = elem / CNN_TAPS, ci = mc % cin, m = mc / cin;
    const int s = CNN_TAPS * (ci / 4) + tap;
    return (t == CT_CONV2_W ? CNN_F2 : CNN_F3) + (2 * s + m / 16) * 64 + (ci % 4) * 16 + m % 16;
  }
  if (t == CT_HEAD_W) {
    const int m = elem / CNN_HEAD_IN, k = elem % CNN_HEAD_IN;
    return CNN_FH + (k / 4) * 64 + (k % 4) * 16 + m;
  }
  if (t == CT_HEAD_B) return CNN_HBIAS + elem;
  const int layer = t / 6, row = t % 6 - 1;                 // row 0 the conv bias, 1 gamma, 2 beta
  if (row > 2) return -1;
  return (layer == 0 ? CNN_P1 : (layer == 1 ? CNN_P2 : CNN_P3)) + row * (layer == 0 ? CNN_C1 : CNN_C2) + elem;
}

// The act kernel's LDS (offsets in floats behind the staged image part)
constexpr int CNN_L_LUT = CNN_STAGED;                          // [256] v / 255.0f
constexpr int CNN_L_A1 = CNN_L_LUT + 256;                      // [TILE][16][324] conv1, then y1 in place
constexpr int CNN_L_A2 = CNN_L_A1 + CNN_TILE * CNN_C1 * CNN_N1;   // [TILE][32][49]
constexpr int CNN_L_Y3 = CNN_L_A2 + CNN_TILE * CNN_C2 * CNN_N2;   // [TILE][128]
constexpr int CNN_ZP = 17;                                     // row stride of a tile's logits
constexpr int CNN_L_ZS = CNN_L_Y3 + CNN_TILE * CNN_FEAT;       // [TILE][CNN_ZP] (80 floats)
constexpr int CNN_L_QD = CNN_L_ZS + 80;                        // [TILE] i32 quadrant (16 floats)
constexpr int CNN_L_IMG = CNN_L_QD + 16;                       // [TILE][3][40][40] u8
constexpr int CNN_LDS_BYTES = (CNN_L_IMG + CNN_TILE * CNN_IMG_BYTES / 4) * 4;
constexpr int CNN_L_PART = CNN_L_A1;                           // conv3's 16 partial chains [2][8][64][4], over the dead y1
static_assert(CNN_TILE * CNN_ZP <= 80 && CNN_L_IMG % 4 == 0 && CNN_LDS_BYTES <= 160 * 1024, "the act kernel's LDS");
static_assert(2 * 8 * 64 * 4 <= CNN_TILE * CNN_C1 * CNN_N1, "conv3's partials fit conv1's maps");

// The entries' argument checks that need no device, in this order; NULL: fine, else the message
// (each names its argument).
inline const char* cnn_create_args_error(int32_t num_actions) {
  if (num_actions < 1 || num_actions > CNN_MAXA) return "be_cnn_create: num_actions must be in [1, 15]";
  return nullptr;
}
// the first of the 20 pointers that is NULL or not 4-byte aligned, as an index, or -1
inline int cnn_bad_tensor(const be_cnn_weights* w) {
  const float* const p[CNN_TENSORS] = {
      w->conv1_weight, w->conv1_bias, w->bn1_weight, w->bn1_bias, w->bn1_running_mean, w->bn1_running_var,
      w->conv2_weight, w->conv2_bias, w->bn2_weight, w->bn2_bias, w->bn2_running_mean, w->bn2_running_var,
      w->conv3_weight, w->conv3_bias, w->bn3_weight, w->bn3_bias, w->bn3_running_mean, w->bn3_running_var,
      w->head_weight, w->head_bias};
  for (int i = 0; i < CNN_TENSORS; ++i)
    if (!p[i] || ((uintptr_t)p[i] & 3)) return i;
  return -1;
}
inline const char* cnn_act_args_error(const void* image, int32_t norm, const be_act_out* out) {
  if (!image) return "be_cnn_act: image is NULL";
  if ((uintptr_t)image & 15) return "be_cnn_act: image must be 16-byte aligned";
  if (norm != BE_CNN_NORM_SAMPLE && norm != BE_CNN_NORM_RUNNING)
    return "be_cnn_act: norm must be BE_CNN_NORM_SAMPLE or BE_CNN_NORM_RUNNING";
  if (!out || !out->action) return "be_cnn_act needs out->action";
  if (out->value) return "be_cnn_act: out->value must be NULL (this network has no value head)";
  return nullptr;
}
// the first of a set's 14 pointers that is NULL or not 4-byte aligned, as an index, or -1
inline int cnn_bad_param(const be_cnn_tensors* t) {
  const float* const p[CNN_PARAMS] = {
      t->conv1_weight, t->conv1_bias, t->bn1_weight, t->bn1_bias, t->conv2_weight, t->conv2_bias, t->bn2_weight,
      t->bn2_bias, t->conv3_weight, t->conv3_bias, t->bn3_weight, t->bn3_bias, t->head_weight, t->head_bias};
  for (int i = 0; i < CNN_PARAMS; ++i)
    if (!p[i] || ((uintptr_t)p[i] & 3)) return i;
  return -1;
}
// be_cnn_adam's four tensor sets, checked in this order (every set before any tensor).  false: fine; else
// *set names the set and *field the tensor ("grads", "conv2_weight"), or is NULL where the set itself is NULL.
inline bool cnn_adam_sets_error(const be_cnn_tensors* params, const be_cnn_tensors* grads, const be_cnn_tensors* exp_avg,
                                const be_cnn_tensors* exp_avg_sq, const char** set, const char** field) {
  const be_cnn_tensors* const sets[4] = {params, grads, exp_avg, exp_avg_sq};
  const char* const names[4] = {"params", "grads", "exp_avg", "exp_avg_sq"};
  for (int s = 0; s < 4; ++s)
    if (!sets[s]) { *set = names[s]; *field = nullptr; return true; }
  for (int s = 0; s < 4; ++s) {
    const int bad = cnn_bad_param(sets[s]);
    if (bad >= 0) { *set = names[s]; *field = CNN_PARAM_NAMES[bad]; return true; }
  }
  return false;
}

}  // namespace behost
