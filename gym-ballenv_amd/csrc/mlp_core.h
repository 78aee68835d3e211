// mlp_core.h -- the block-count MLP's packed image and forward, shared by the
// select_action kernel (mlp_policy.hip: mlp_act_kernel) and the fused rollout (ballenv.hip:
// mlp_rollout_kernel), as policy_core.h is for the A2C Policy and blocks_core.h for
// prep_state2.  Device code and constexpr layout only; every product is an f32 fma chain on
// v_mfma_f32_16x16x4_f32 in ONE k order, so an env's logits are the same bits in whichever kernel and
// whichever 16-env tile they are computed: an MFMA column is an env, and no column reads another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blocks_core.h"
#include "philox.h"
#include "policy_core.h"

namespace {

#ifndef BE_MLP_WAVES
#define BE_MLP_WAVES 8       // -DBE_MLP_WAVES=n: timing builds with n waves per workgroup
#endif
constexpr int MLP_NW = BE_MLP_WAVES;          // mlp_act_kernel's waves per workgroup (MlpLayout::lds counts their slices)
constexpr int MLP_MAXH = 128, MLP_KS1 = 8;   // 4-wide k steps of layer 1 (29 -> 32 inputs)
constexpr int MLP_NO = 16;                   // padded outputs: policy_finish<16> (actions 0..14, slot 15 unused)
constexpr int MLP_ZP = 17;                   // row stride of a tile's logits in the wave's slice
constexpr int MLP_SLICE = 16 * MLP_ZP + 16 * BLK_ROW / 4 + 12;   // mlp_act_kernel's floats per wave: logits, then 16 rows of blocks
static_assert(MLP_SLICE % 4 == 0 && 16 * BLK_ROW % 4 == 0, "the slices stay 16-byte aligned");
static_assert(POL_MAXA < MLP_NO, "policy_finish<16> holds be_policy_create's action bound");
// Every shape runs the instance of its layer count, padded to 128 hidden units.
constexpr int MLP_HT = MLP_MAXH / 16;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The packed image, identical in HBM and in each workgroup's LDS (offsets in floats).  HT1 / HT2 / HTL
// are 16-row tiles of hidden1 / hidden2 / the last layer's input; l15 = lane & 15, l4 = lane >> 4.
struct MlpLayout {
  int layers, HT1, HT2, HTL;
  int f1;      // [MLP_KS1][HT1][64]   W1[16 t + l15][4 k + l4]
  int b1;      // [16 HT1]
  int f2;      // [4 HT1][HT2][64]     W2[16 t + l15][16 (s >> 2) + 4 l4 + (s & 3)]     (3 layers)
  int b2;      // [16 HT2]                                                               (3 layers)
  int f3;      // [4 HTL][64]          W_last[l15][16 (s >> 2) + 4 l4 + (s & 3)]
  int b3;      // [16]
  int hb;      // [16]                 0 for an action (and slot 15), -inf for a pad action
  int total, lds;                      // floats of the image; bytes of mlp_act_kernel's LDS with the waves' slices
};
__host__ __device__ constexpr MlpLayout mlp_layout(int layers, int HT1, int HT2) {
  MlpLayout L{};
  L.layers = layers; L.HT1 = HT1; L.HT2 = layers == 3 ? HT2 : 0; L.HTL = layers == 3 ? HT2 : HT1;
  L.f1 = 0;
  L.b1 = L.f1 + MLP_KS1 * HT1 * 64;
  L.f2 = L.b1 + 16 * HT1;
  L.b2 = L.f2 + 4 * HT1 * L.HT2 * 64;
  L.f3 = L.b2 + 16 * L.HT2;
  L.b3 = L.f3 + 4 * L.HTL * 64;
  L.hb = L.b3 + 16;
  L.total = L.hb + 16;
  L.lds = (L.total + MLP_NW * MLP_SLICE) * 4;
  return L;
}

// sum of x over lanes l, l^16, l^32, l^48 (or_groups of policy_core.h with +)
__device__ __forceinline__ uint32_t sum_groups_u32(uint32_t x) {
  const auto a = __builtin_amdgcn_permlane16_swap(x, x, false, false);
  x = a[0] + a[1];
  const auto b = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return b[0] + b[1];
}

// wave barrier between a slice's writes and its reads by other lanes of the wave
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#define BE_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// TWO forwards live here and must stay in step: mlp_act_kernel's (its inline layer 1, then mlp_hidden and
// mlp_last below) and the fused rollout's (mlp_forward on mlp_chain_ahead, further down).  They differ only in
// when a weight fragment is read from LDS; the k order of every chain, the bias in the chain's start and the
// last layer's (c0 + c1) + (c2 + c3) are the same, and tests/test_gpu_mlp_rollout.py holds the two to the same
// bits.  Whoever changes the arithmetic of one changes the other.
//
// One layer with HTI input tiles (h, relu'd, in the accumulator layout) and HTO output tiles:
// acc[t] starts at the bias.  frag: [4 HTI][HTO][64], bias: [16 HTO].
template <int HTI, int HTO>
__device__ __forceinline__ void mlp_hidden(const float* frag, const float* bias, const f32x4 (&h)[HTI], int lane,
                                           f32x4 (&acc)[HTO]) {
#pragma unroll
  for (int t = 0; t < HTO; ++t) acc[t] = *(const f32x4*)(bias + 16 * t + 4 * (lane >> 4));
#pragma unroll
  for (int hp = 0; hp < HTI; ++hp)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int t = 0; t < HTO; ++t) acc[t] = BE_MFMA(frag[((hp * 4 + r) * HTO + t) * 64 + lane], h[hp][r], acc[t]);
#pragma unroll
  for (int t = 0; t < HTO; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = fmaxf(acc[t][r], 0.0f);
}

// The last layer: one output tile, four fma chains (chain r takes the steps (t, r); chain 0 starts at
// the bias), z = (c0 + c1) + (c2 + c3).
template <int HTI>
__device__ __forceinline__ f32x4 mlp_last(const float* frag, const float* bias, const f32x4 (&h)[HTI], int lane) {
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 c[4] = {*(const f32x4*)(bias + 4 * (lane >> 4)), zero4, zero4, zero4};
#pragma unroll
  for (int hp = 0; hp < HTI; ++hp)
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = BE_MFMA(frag[(hp * 4 + r) * 64 + lane], h[hp][r], c[r]);
  return (c[0] + c[1]) + (c[2] + c[3]);
}

// The same chains for a wave that has its SIMD to itself (the fused rollout's small batches).  Left to the
// compiler, every pair of MFMAs waits for its own fragment read (ds_read2st64_b32, s_waitcnt lgkmcnt(0), two
// MFMAs), which exposes most of the LDS latency: about 46 cycles per MFMA instead of 32.  Here
// the NT fragments of k step s + 1 are read ahead of step s's MFMAs, and a scheduling barrier on either side of
// the MFMAs keeps that order: a read then has a whole k step of MFMAs to arrive in.  Same operands, same order
// in every chain: the same bits.  Step s issues NT MFMAs, acc[t] += fragment (s NT + t) x b(s, t): a hidden
// layer's NT output tiles share the step's B operand, the last layer's four chains each take their own.
template <int NS, int NT, class BOp>
__device__ __forceinline__ void mlp_chain_ahead(const float* frag, int lane, BOp&& b, f32x4 (&acc)[NT]) {
  float a[2][NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) a[0][t] = frag[t * 64 + lane];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s + 1 < NS) {
#pragma unroll
      for (int t = 0; t < NT; ++t) a[(s + 1) & 1][t] = frag[((s + 1) * NT + t) * 64 + lane];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = BE_MFMA(a[s & 1][t], b(s, t), acc[t]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The whole forward of one 16-env tile from its layer-1 B operand: logits 4 l4 + r of env l15 (before
// the optional final relu).  W: the staged image.  The arithmetic of mlp_act_kernel's layer 1, mlp_hidden and
// mlp_last, with the fragment reads a k step ahead (mlp_chain_ahead).
template <int LAYERS, int HT1, int HT2>
__device__ __forceinline__ f32x4 mlp_forward(const float* W, const float (&x)[MLP_KS1], int lane) {
  constexpr MlpLayout L = mlp_layout(LAYERS, HT1, HT2);
  constexpr int HTL = LAYERS == 3 ? HT2 : HT1;
  const int l4 = lane >> 4;
  f32x4 h1[HT1], hl[HTL];
#pragma unroll
  for (int t = 0; t < HT1; ++t) h1[t] = *(const f32x4*)(W + L.b1 + 16 * t + 4 * l4);
  mlp_chain_ahead<MLP_KS1, HT1>(W + L.f1, lane, [&](int s, int) { return x[s]; }, h1);
#pragma unroll
  for (int t = 0; t < HT1; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) h1[t][r] = fmaxf(h1[t][r], 0.0f);
  if constexpr (LAYERS == 3) {
#pragma unroll
    for (int t = 0; t < HT2; ++t) hl[t] = *(const f32x4*)(W + L.b2 + 16 * t + 4 * l4);
    mlp_chain_ahead<4 * HT1, HT2>(W + L.f2, lane, [&](int s, int) { return h1[s >> 2][s & 3]; }, hl);
#pragma unroll
    for (int t = 0; t < HT2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) hl[t][r] = fmaxf(hl[t][r], 0.0f);
  } else {
#pragma unroll
    for (int t = 0; t < HT1; ++t) hl[t] = h1[t];
  }
  // the last layer: k steps of four, one per chain (mlp_last: chain r takes the steps (t, r))
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 c[4] = {*(const f32x4*)(W + L.b3 + 4 * l4), zero4, zero4, zero4};
  mlp_chain_ahead<HTL, 4>(W + L.f3, lane, [&](int hp, int r) { return hl[hp][r]; }, c);
  return (c[0] + c[1]) + (c[2] + c[3]);
}

}  // namespace
