// cnn_policy.hip -- on-GPU select_action of the reference's pixel agent: the conv net
// of examples/ball_cnn_reinforce.py on the 40 x 40 patch image be_observe_pixels writes, with the
// reference's per-env BatchNorm statistics, plus the Categorical draw -- one launch for every env.
//
// Reference:
//   examples/ball_cnn_reinforce.py:60-83   Policy: conv1..3 (5 x 5, stride 2) + bn1..3 + relu, head
//                                          Linear(132, 9) on the features and the quadrant, softmax
//   examples/ball_cnn_reinforce.py:85-95   select_action (policy.eval() is never called, and the batch
//                                          is one image: BatchNorm uses that image's own statistics)
//
//   be_cnn_load   one launch: the 20 f32 state_dict arrays into the packed image (cnn_host.h)
//   be_cnn_act    one launch: the forward, softmax and draw, the arithmetic include/ballenv.h pins
//   be_cnn_adam   two launches: optimizer.step() (Adam, ball_cnn_reinforce.py:115, :244) on the 14 parameters
//                 fused with the re-pack of the image, then the state kernel shared with
//                 be_a2c_adam and be_mlp_opt (be_internal_optim_advance)
//
// Every product runs on v_mfma_f32_16x16x4_f32 (an exact f32 fma chain) as an implicit GEMM
// D = W . patches: the weights are the A operand (row = output channel), a column of the B operand is
// one output position of one env, and a k step takes four inputs of that position's 5 x 5 patches
// straight from the layer below in LDS -- lane (c = lane & 15, g = lane >> 4) reads input g of the
// step for column c.  The k order (cnn_host.h) makes that address the lane's own base plus a
// compile-time offset: conv2 / conv3 take four input channels at one tap per step (the channel is
// the lane's, the tap the step's), conv1 four kx of one (ci, ky).  No column reads another, so an
// env's result does not depend on which columns its positions fall in.
//
// A persistent grid, one workgroup of 8 waves per CU; conv1's fragments, the head's and the per-channel
// vectors are staged once per workgroup in LDS (15 KB), conv2's and conv3's A fragments (154 KB) come
// from the packed image in global memory, 256 contiguous bytes per wave and fragment, the same bytes for
// every wave of the grid.  A workgroup takes 4 envs per round, whose activations live in LDS
// (19 KB of u8 image, 81 KB conv1, 24.5 KB conv2): 4 envs fill conv1's column tiles exactly
// (4 x 324 = 81 x 16) and conv3's (4 x 4 = 16), conv2's to 196 of 208.  Per round, with a workgroup
// barrier between the phases:
//   0  the tile's images into LDS (16-byte loads), the quadrants
//   1  conv1: wave w takes the column tiles w, w + 8, ... two at a time; image byte -> x through a
//      256-entry table of v / 255.0f
//   2  BatchNorm + relu of conv1 in place: 8 threads per (env, channel) map, the map in registers
//      across the two statistics passes and the write-back
//   3  conv2: wave w takes row tile w & 1 and the column tiles (w >> 1) + 4 i, so a fragment read
//      serves up to 4 MFMAs; the fragments of the next 5 steps are read from global memory ahead of
//      this row's MFMAs (10 % of the kernel's time at 65 536 envs, profiles/pixel_act.json's history
//      in DESIGN 3.19)
//   4  BatchNorm + relu of conv2 in place, 4 threads per map
//   5  conv3: wave w takes row tile w & 1 and chains 2 (w >> 1), 2 (w >> 1) + 1 of the eight
//   6  the chains' sum, BatchNorm + relu of conv3 (4 threads per map) into the feature rows
//   7  wave 0: the head (33 MFMAs), then lanes 0..3 finish one env each (policy_core.h's policy_finish)
#include <hip/hip_runtime.h>

#include <math.h>
#include <new>
#include <stdint.h>

#include "ballenv.h"
#include "cnn_host.h"
#include "host_logic.h"
#include "internal.h"
#include "mlp_core.h"
#include "optim_core.h"
#include "philox.h"
#include "policy_core.h"

namespace {

using namespace behost;

constexpr int CNN_THREADS = 64 * CNN_WAVES;
static_assert(CNN_WAVES == 8 && CNN_TILE == 4, "the phases' work split is written for 8 waves and 4 envs");
static_assert(CNN_MAXA == POL_MAXA && CNN_NO == MLP_NO, "policy_finish<16> holds the action bound");
constexpr float CNN_EPS = 1e-5f;

struct CPack {
  const float* t[CNN_TENSORS];
  int32_t A;
};

__global__ __launch_bounds__(256) void cnn_pack_kernel(CPack a, float* img) {
  for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < CNN_TOTAL; i += (int)gridDim.x * 256) {
    int elem;
    const int src = cnn_pack_source(i, a.A, &elem);
    float v = src == CNN_SRC_NEGINF ? -INFINITY : 0.0f;
    if (src >= 0) {
      const float* t = a.t[0];
#pragma unroll
      for (int k = 1; k < CNN_TENSORS; ++k) t = src == k ? a.t[k] : t;   // selects: no indexed copy of the table
      v = t[elem];
    }
    img[i] = v;
  }
}

// be_cnn_adam: the Adam step on the 14 parameters and the pack above, inverted.  Thread i takes source
// element i of the parameters laid end to end in be_cnn_tensors' order (cnn_param_at), so a wave reads
// w, g, m, v and writes w, m, v as consecutive floats, and scatters its new weight to the one image index
// that cnn_pack_kernel fills from that element (cnn_pack_dest).  The map is a bijection onto the image's
// entries that hold a parameter (tests/cnn_adam_host_main.cpp): no element has two writers and no thread
// reads what another writes.  The running statistics' rows, the pads and hb keep what be_cnn_load wrote.
struct CSet { float* t[CNN_PARAMS]; };

struct CAdam {
  CSet w, g, m, v;           // params, grads (read only), exp_avg, exp_avg_sq
  const double* state;       // [t, beta1^t, beta2^t, lr] before the call
  double beta1, beta2, eps;
  float* img;
  int32_t A;
};

__global__ __launch_bounds__(256) void cnn_adam_kernel(CAdam p) {
  int j;
  const int k = cnn_param_at((int)(blockIdx.x * 256 + threadIdx.x), p.A, &j);
  if (k < 0) return;
  float *w = p.w.t[0], *m1p = p.m.t[0], *m2p = p.v.t[0];
  const float* g = p.g.t[0];
#pragma unroll
  for (int q = 1; q < CNN_PARAMS; ++q) {                     // selects: no indexed copy of the tables
    w = k == q ? p.w.t[q] : w;
    g = k == q ? p.g.t[q] : g;
    m1p = k == q ? p.m.t[q] : m1p;
    m2p = k == q ? p.v.t[q] : m2p;
  }
  // the pinned arithmetic of include/ballenv.h (optim_core.h)
  p.img[cnn_pack_dest(cnn_param_tensor(k), j)] = adam_elem(adam_step(p.state, p.beta1, p.beta2, p.eps), g, m1p, m2p, w, j);
}

CSet cnn_set(const be_cnn_tensors* t) {
  return CSet{{t->conv1_weight, t->conv1_bias, t->bn1_weight, t->bn1_bias, t->conv2_weight, t->conv2_bias, t->bn2_weight,
               t->bn2_bias, t->conv3_weight, t->conv3_bias, t->bn3_weight, t->bn3_bias, t->head_weight, t->head_bias}};
}

struct CParams {
  const float* img;
  const uint8_t* image;        // (N, 3, 40, 40)
  const uint8_t* quadrant_in;  // (N) or NULL: from agent / goal
  const int32_t* agent; const int32_t* goal;
  const uint32_t* episode;     // (N) Philox key words (be_state.episode / ep_len)
  const int32_t* ep_len;
  uint8_t* action;             // (N)
  float* log_prob;             // (N) or NULL
  float* probs;                // (N, A) or NULL
  unsigned long long seed;
  int32_t n, ntiles, A, gid0, sample;
};

// sum over the P lanes that share a map (lanes j ^ 1, j ^ 2, j ^ 4): ((s0 + s1) + (s2 + s3)) + ...
template <int P>
__device__ __forceinline__ float cnn_tree(float s) {
#pragma unroll
  for (int m = 1; m < P; m <<= 1) s = s + __shfl_xor(s, m);
  return s;
}

// BatchNorm + relu of one map of NPOS positions in place, by the P threads j = 0..P-1 that share it:
// thread j holds the positions j, j + P, ... in registers.  prm: the layer's [5][C] vectors.
template <int NPOS, int P>
__device__ __forceinline__ void cnn_norm_map(float* map, int j, const float* prm, int C, int ch, bool sample) {
  constexpr int NI = (NPOS + P - 1) / P;
  float v[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) v[i] = map[min(j + P * i, NPOS - 1)];
  float mean, var;
  if (sample) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NI; ++i) s = j + P * i < NPOS ? s + v[i] : s;
    mean = cnn_tree<P>(s) / (float)NPOS;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const float d = v[i] - mean;
      q = j + P * i < NPOS ? q + d * d : q;
    }
    var = cnn_tree<P>(q) / (float)NPOS;
  } else {
    mean = prm[3 * C + ch];
    var = prm[4 * C + ch];
  }
  const float inv = 1.0f / sqrtf(var + CNN_EPS);
  const float gamma = prm[C + ch], beta = prm[2 * C + ch];
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (j + P * i < NPOS) map[j + P * i] = fmaxf(((v[i] - mean) * inv) * gamma + beta, 0.0f);
}

// conv2 for one wave: row tile rt, the NCT column tiles j0, j0 + 4, ...  g2: the wave's fragments
// (image + CNN_F2 + 64 rt + lane, 128 floats per step).
template <int NCT>
__device__ __forceinline__ void cnn_conv2(const float* g2, const float* A1, float* A2, const float* bias, int j0, int rt,
                                          int l15, int l4) {
  int base[NCT], p[NCT];
  f32x4 acc[NCT];
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    p[c] = 16 * (j0 + 4 * c) + l15;
    const int pc = min(p[c], CNN_TILE * CNN_N2 - 1);     // a pad column computes its neighbour's and writes nothing
    const int env = pc / CNN_N2, pos = pc - CNN_N2 * env, oy = pos / CNN_S2, ox = pos - CNN_S2 * oy;
    base[c] = (env * CNN_C1 + l4) * CNN_N1 + 2 * oy * CNN_S1 + 2 * ox;
    acc[c] = *(const f32x4*)bias;
  }
  // A row is the 5 kx steps of one (cg, ky).  The rows stay a loop (unrolled over all 25 taps the hoisted
  // operand reads outgrow the register file), two rows per trip: the fragments of the next row are read from
  // global memory ahead of this row's MFMAs, and a scheduling barrier on either side of the MFMAs keeps that
  // order, so a read has a row of MFMAs to arrive in (mlp_chain_ahead's scheme; the same operands in the
  // same order in every chain).
  constexpr int ROWS = (CNN_C1 / 4) * CNN_KS;
  static_assert(ROWS % 2 == 0, "two rows per trip");
  float a[2][CNN_KS];
#pragma unroll
  for (int kx = 0; kx < CNN_KS; ++kx) a[0][kx] = g2[kx * 128];
#pragma unroll 1
  for (int row = 0; row < ROWS; row += 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cur = row + h, nxt = min(cur + 1, ROWS - 1);      // the last trip re-reads its own row
#pragma unroll
      for (int kx = 0; kx < CNN_KS; ++kx) a[h ^ 1][kx] = g2[(nxt * CNN_KS + kx) * 128];
      const int cg = cur / CNN_KS, ky = cur - CNN_KS * cg;
      const int off = cg * 4 * CNN_N1 + ky * CNN_S1;
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kx = 0; kx < CNN_KS; ++kx)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[c] = BE_MFMA(a[h][kx], A1[base[c] + off + kx], acc[c]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    if (p[c] < CNN_TILE * CNN_N2) {
      const int env = p[c] / CNN_N2, pos = p[c] - CNN_N2 * env;
#pragma unroll
      for (int r = 0; r < 4; ++r) A2[(env * CNN_C2 + 16 * rt + 4 * l4 + r) * CNN_N2 + pos] = acc[c][r];
    }
  }
}

__global__ __launch_bounds__(CNN_THREADS) void cnn_act_kernel(CParams p) {
  extern __shared__ uint4 cnn_lds[];
  float* S = (float*)cnn_lds;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  stage_image<CNN_THREADS, 2>(cnn_lds, (const uint4*)p.img, CNN_STAGED / 4, tid);
  if (tid < 256) S[CNN_L_LUT + tid] = (float)tid / 255.0f;
  const float* LUT = S + CNN_L_LUT;
  float* A1 = S + CNN_L_A1;
  float* A2 = S + CNN_L_A2;
  float* Y3 = S + CNN_L_Y3;
  float* Zs = S + CNN_L_ZS;
  float* P3 = S + CNN_L_PART;
  int* QD = (int*)(S + CNN_L_QD);
  uint8_t* IMG = (uint8_t*)(S + CNN_L_IMG);
  const bool sample = p.sample != 0;
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  // conv1's steps 15..18: the lane's (ci, ky) at kx = 4 (j = 15 is the zero weight: any byte serves)
  int off4[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = min(4 * q + l4, 14);
    off4[q] = (j / 5) * CNN_IMG * CNN_IMG + (j % 5) * CNN_IMG + 4;
  }
  const int rt = wave & 1, wq = wave >> 1;

  for (int tile = (int)blockIdx.x; tile < p.ntiles; tile += (int)gridDim.x) {
    const int e0 = tile * CNN_TILE, nv = min(CNN_TILE, p.n - e0);

    // 0: the images (an env past the end is all zero bytes: it computes and writes nothing out)
    {
      const uint4* src = (const uint4*)(p.image + (int64_t)e0 * CNN_IMG_BYTES);
      constexpr int W16 = CNN_IMG_BYTES / 16;
      for (int k = tid; k < CNN_TILE * W16; k += CNN_THREADS)
        ((uint4*)IMG)[k] = k < nv * W16 ? src[k] : uint4{0u, 0u, 0u, 0u};
      if (tid < CNN_TILE) {
        int quad = 0;
        if (tid < nv) {
          if (p.quadrant_in) {
            quad = p.quadrant_in[e0 + tid] & 3;
          } else {                                  // blocks_init's rule (blocks_core.h)
            const int32_t a = p.agent[e0 + tid], g = p.goal[e0 + tid];
            const int dx = px(g) - px(a), dy = py(g) - py(a);
            quad = dx >= 0 ? (dy >= 0 ? 1 : 2) : (dy >= 0 ? 0 : 3);
          }
        }
        QD[tid] = quad;
      }
    }
    __syncthreads();

    // 1: conv1
    for (int tA = wave; tA < CNN_TILE * CNN_N1 / 16; tA += 16) {
      const bool hasB = tA + 8 < CNN_TILE * CNN_N1 / 16;
      const int pA = 16 * tA + l15, pB = 16 * (hasB ? tA + 8 : tA) + l15;
      const int envA = pA / CNN_N1, posA = pA - CNN_N1 * envA, oyA = posA / CNN_S1, oxA = posA - CNN_S1 * oyA;
      const int envB = pB / CNN_N1, posB = pB - CNN_N1 * envB, oyB = posB / CNN_S1, oxB = posB - CNN_S1 * oyB;
      const uint8_t* iA = IMG + envA * CNN_IMG_BYTES + 2 * oyA * CNN_IMG + 2 * oxA;
      const uint8_t* iB = IMG + envB * CNN_IMG_BYTES + 2 * oyB * CNN_IMG + 2 * oxB;
      f32x4 accA = *(const f32x4*)(S + CNN_P1 + 4 * l4), accB = accA;
#pragma unroll
      for (int s = 0; s < CNN_K1; ++s) {
        const int off = s < 15 ? (s / 5) * CNN_IMG * CNN_IMG + (s % 5) * CNN_IMG + l4 : off4[s < 15 ? 0 : s - 15];
        const float a = S[CNN_F1 + s * 64 + lane];
        accA = BE_MFMA(a, LUT[iA[off]], accA);
        accB = BE_MFMA(a, LUT[iB[off]], accB);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) A1[(envA * CNN_C1 + 4 * l4 + r) * CNN_N1 + posA] = accA[r];
      if (hasB) {
#pragma unroll
        for (int r = 0; r < 4; ++r) A1[(envB * CNN_C1 + 4 * l4 + r) * CNN_N1 + posB] = accB[r];
      }
    }
    __syncthreads();

    // 2: bn1 + relu in place: map tid >> 3 = env * 16 + channel
    cnn_norm_map<CNN_N1, 8>(A1 + (tid >> 3) * CNN_N1, tid & 7, S + CNN_P1, CNN_C1, (tid >> 3) & (CNN_C1 - 1), sample);
    __syncthreads();

    // 3: conv2
    {
      const float* g2 = p.img + CNN_F2 + 64 * rt + lane;
      const float* bias = S + CNN_P2 + 16 * rt + 4 * l4;
      if (wq == 0) cnn_conv2<4>(g2, A1, A2, bias, wq, rt, l15, l4);
      else cnn_conv2<3>(g2, A1, A2, bias, wq, rt, l15, l4);
    }
    __syncthreads();

    // 4: bn2 + relu in place: map tid >> 2 = env * 32 + channel
    cnn_norm_map<CNN_N2, 4>(A2 + (tid >> 2) * CNN_N2, tid & 3, S + CNN_P2, CNN_C2, (tid >> 2) & (CNN_C2 - 1), sample);
    __syncthreads();

    // 5: conv3: column l15 = env * 4 + position; chains 2 wq and 2 wq + 1
    {
      const int env = l15 >> 2, oy = (l15 >> 1) & 1, ox = l15 & 1;
      const int base = (env * CNN_C2 + 8 * wq + l4) * CNN_N2 + 2 * oy * CNN_S2 + 2 * ox;
      const float* g3 = p.img + CNN_F3 + (2 * wq * CNN_TAPS) * 128 + 64 * rt + lane;
      f32x4 c0 = wq == 0 ? *(const f32x4*)(S + CNN_P3 + 16 * rt + 4 * l4) : zero4, c1 = zero4;
      // the fragments of row ky + 1 are read ahead of row ky's MFMAs (cnn_conv2's scheme; the last row re-reads itself)
      float a0[CNN_KS], a1[CNN_KS], n0[CNN_KS], n1[CNN_KS];
#pragma unroll
      for (int kx = 0; kx < CNN_KS; ++kx) { a0[kx] = g3[kx * 128]; a1[kx] = g3[(CNN_TAPS + kx) * 128]; }
#pragma unroll 1
      for (int ky = 0; ky < CNN_KS; ++ky) {
        const int nk = min(ky + 1, CNN_KS - 1);
#pragma unroll
        for (int kx = 0; kx < CNN_KS; ++kx) {
          n0[kx] = g3[(nk * CNN_KS + kx) * 128];
          n1[kx] = g3[(CNN_TAPS + nk * CNN_KS + kx) * 128];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kx = 0; kx < CNN_KS; ++kx) {
          const int off = ky * CNN_S2 + kx;
          c0 = BE_MFMA(a0[kx], A2[base + off], c0);
          c1 = BE_MFMA(a1[kx], A2[base + 4 * CNN_N2 + off], c1);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kx = 0; kx < CNN_KS; ++kx) { a0[kx] = n0[kx]; a1[kx] = n1[kx]; }
      }
      *(f32x4*)(P3 + ((rt * 8 + 2 * wq) * 64 + lane) * 4) = c0;
      *(f32x4*)(P3 + ((rt * 8 + 2 * wq + 1) * 64 + lane) * 4) = c1;
    }
    __syncthreads();

    // 6: the eight chains' sum, bn3 + relu: thread = (env * 32 + channel) * 4 + position, 4 threads per map
    // (a map of four equal values then has exactly their value as its mean: (v + v) + (v + v))
    {
      const int env = tid >> 7, ch = (tid >> 2) & 31, pos = tid & 3;
      float* row = Y3 + env * CNN_FEAT + ch * CNN_N3;
      const float* c = P3 + (((ch >> 4) * 8) * 64 + ((ch >> 2) & 3) * 16 + env * 4 + pos) * 4 + (ch & 3);
      row[pos] = ((c[0] + c[256]) + (c[512] + c[768])) + ((c[1024] + c[1280]) + (c[1536] + c[1792]));
      cnn_norm_map<CNN_N3, 4>(row, pos, S + CNN_P3, CNN_C3, ch, sample);
    }
    __syncthreads();

    // 7: the head and the draw: column l15 is env l15 & 3 (columns 4..15 repeat them)
    if (wave == 0) {
      const int env = l15 & 3;
      f32x4 c[4] = {*(const f32x4*)(S + CNN_HBIAS + 4 * l4), zero4, zero4, zero4};
#pragma unroll
      for (int s = 0; s < CNN_KH - 1; ++s)
        c[s & 3] = BE_MFMA(S[CNN_FH + s * 64 + lane], Y3[env * CNN_FEAT + 4 * s + l4], c[s & 3]);
      c[0] = BE_MFMA(S[CNN_FH + (CNN_KH - 1) * 64 + lane], l4 == QD[env] ? 1.0f : 0.0f, c[0]);
      const f32x4 z = (c[0] + c[1]) + (c[2] + c[3]);
      if (l15 < CNN_TILE) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Zs[l15 * CNN_ZP + 4 * l4 + r] = z[r];
      }
      wave_sync();
      if (lane < nv) {
        const int e = e0 + lane;
        float lp, val;
        const int act = policy_finish<CNN_NO>(Zs + lane * CNN_ZP, S + CNN_HB, p.A, (uint32_t)(p.gid0 + e), p.episode[e],
                                              (uint32_t)p.ep_len[e], p.seed,
                                              p.probs ? p.probs + (int64_t)e * p.A : nullptr, lp, val);
        p.action[e] = (uint8_t)act;
        if (p.log_prob) p.log_prob[e] = lp;
      }
      wave_sync();
    }
    // the next round's first writes (the images, QD) touch nothing wave 0 still reads; its barrier orders the rest
  }
}

}  // namespace

struct be_cnn {
  be_ctx* ctx;
  be_ctx_view cv;
  int A, cus;
  float* img;
  bool loaded;
};

extern "C" {

int be_cnn_create(be_ctx* ctx, int32_t num_actions, be_cnn** out) {
  if (!ctx || !out) return be_ctx_fail(ctx, BE_E_INVALID, "bad arguments to be_cnn_create");
  *out = nullptr;
  if (const char* msg = behost::cnn_create_args_error(num_actions)) return be_ctx_fail(ctx, BE_E_INVALID, msg);
  be_cnn* m = new (std::nothrow) be_cnn();
  if (!m) return be_ctx_fail(ctx, BE_E_NOMEM, "out of host memory");
  m->ctx = ctx; m->cv = be_ctx_get(ctx);
  m->A = num_actions;
  const DeviceGuard dg(m->cv.device);   // the caller's current device is restored on return
  hipError_t e = dg.err;
  if (e == hipSuccess) e = hipDeviceGetAttribute(&m->cus, hipDeviceAttributeMultiprocessorCount, m->cv.device);
  if (e == hipSuccess) e = hipMalloc(&m->img, (size_t)CNN_TOTAL * 4);
  if (e == hipSuccess) e = hipMemset(m->img, 0, (size_t)CNN_TOTAL * 4);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)cnn_act_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CNN_LDS_BYTES);
  if (e != hipSuccess || m->cus < 1) {
    if (m->img) (void)hipFree(m->img);
    delete m;
    if (e == hipSuccess) return be_ctx_fail(ctx, BE_E_HIP, "be_cnn_create: cannot query the device's compute units");
    return be_hip_fail(be_ctx_err(ctx), e);
  }
  *out = m;
  return BE_OK;
}

int be_cnn_destroy(be_cnn* m) {
  if (!m) return BE_OK;
  const DeviceGuard dg(m->cv.device);
  if (m->img) (void)hipFree(m->img);
  delete m;
  return BE_OK;
}

int be_cnn_load(be_cnn* m, const be_cnn_weights* w, void* stream) {
  if (!m) return be_ctx_fail(nullptr, BE_E_INVALID, "be_cnn_load: cnn is NULL");
  be_ctx* ctx = m->ctx;
  if (!w) return be_ctx_fail(ctx, BE_E_INVALID, "be_cnn_load: w is NULL");
  const int bad = behost::cnn_bad_tensor(w);
  if (bad >= 0)
    return be_fail(be_ctx_err(ctx), BE_E_INVALID, "be_cnn_load: w->%s is NULL or not 4-byte aligned", CNN_TENSOR_NAMES[bad]);
  BE_ENTER_DEVICE(be_ctx_err(ctx), m->cv.device);
  const CPack a{{w->conv1_weight, w->conv1_bias, w->bn1_weight, w->bn1_bias, w->bn1_running_mean, w->bn1_running_var,
                 w->conv2_weight, w->conv2_bias, w->bn2_weight, w->bn2_bias, w->bn2_running_mean, w->bn2_running_var,
                 w->conv3_weight, w->conv3_bias, w->bn3_weight, w->bn3_bias, w->bn3_running_mean, w->bn3_running_var,
                 w->head_weight, w->head_bias},
                m->A};
  hipLaunchKernelGGL(cnn_pack_kernel, dim3((unsigned)((CNN_TOTAL + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, m->img);
  if (int rc = be_launched(be_ctx_err(ctx))) return rc;
  m->loaded = true;
  return BE_OK;
}

int be_cnn_act(be_cnn* m, const be_state* st, const uint8_t* image, const uint8_t* quadrant_in, int32_t norm,
               const be_act_out* out, uint64_t seed, void* stream) {
  if (!m) return be_ctx_fail(nullptr, BE_E_INVALID, "be_cnn_act: cnn is NULL");
  be_ctx* ctx = m->ctx;
  if (!m->loaded) return be_ctx_fail(ctx, BE_E_INVALID, "be_cnn_act before be_cnn_load");
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (const char* msg = behost::cnn_act_args_error(image, norm, out)) return be_ctx_fail(ctx, BE_E_INVALID, msg);
  BE_ENTER_DEVICE(be_ctx_err(ctx), m->cv.device);
  CParams p{};
  p.img = m->img;
  p.image = image; p.quadrant_in = quadrant_in;
  p.agent = st->agent; p.goal = st->goal;
  p.episode = st->episode; p.ep_len = st->ep_len;
  p.action = out->action; p.log_prob = out->log_prob; p.probs = out->probs;
  p.seed = (unsigned long long)seed;
  p.n = m->cv.num_envs;
  p.ntiles = (p.n + CNN_TILE - 1) / CNN_TILE;
  p.A = m->A; p.gid0 = (int32_t)(uint32_t)m->cv.env_offset;
  p.sample = norm == BE_CNN_NORM_SAMPLE;
  const dim3 grid((unsigned)(p.ntiles < m->cus ? p.ntiles : m->cus)), block(CNN_THREADS);
  hipLaunchKernelGGL(cnn_act_kernel, grid, block, (size_t)CNN_LDS_BYTES, (hipStream_t)stream, p);
  return be_launched(be_ctx_err(ctx));
}

int be_cnn_adam(be_cnn* m, const be_cnn_tensors* params, const be_cnn_tensors* grads, const be_cnn_tensors* exp_avg,
                const be_cnn_tensors* exp_avg_sq, double* state, double beta1, double beta2, double eps,
                const double* losses, double* loss_log, int32_t log_rows, void* stream) {
  if (!m) return be_ctx_fail(nullptr, BE_E_INVALID, "be_cnn_adam: cnn is NULL");
  be_ctx* ctx = m->ctx;
  char* err = be_ctx_err(ctx);
  if (!m->loaded) return be_ctx_fail(ctx, BE_E_INVALID, "be_cnn_adam before be_cnn_load");
  const char *set, *field;
  if (behost::cnn_adam_sets_error(params, grads, exp_avg, exp_avg_sq, &set, &field)) {
    if (!field) return be_fail(err, BE_E_INVALID, "be_cnn_adam: %s is NULL", set);
    char name[64];
    snprintf(name, sizeof name, "%s->%s", set, field);
    return be_fail(err, BE_E_INVALID, "be_cnn_adam: %s is NULL or not 4-byte aligned", name);
  }
  if (const char* msg = behost::optim_args_error(state, true, beta1, beta2, eps, losses, loss_log, log_rows))
    return be_fail(err, BE_E_INVALID, "be_cnn_adam: %s", msg);
  BE_ENTER_DEVICE(err, m->cv.device);
  CAdam p{};
  p.w = cnn_set(params); p.g = cnn_set(grads); p.m = cnn_set(exp_avg); p.v = cnn_set(exp_avg_sq);
  p.state = state; p.beta1 = beta1; p.beta2 = beta2; p.eps = eps;
  p.img = m->img; p.A = m->A;
  const dim3 grid((unsigned)((cnn_param_elems(m->A) + 255) / 256)), block(256);
  hipLaunchKernelGGL(cnn_adam_kernel, grid, block, 0, (hipStream_t)stream, p);
  if (int rc = be_launched(err)) return rc;
  return be_internal_optim_advance(err, state, true, beta1, beta2, losses, loss_log, 2, log_rows, stream);
}

int64_t be_cnn_bytes(const be_cnn* m) { return m ? (int64_t)CNN_TOTAL * 4 : 0; }

}  // extern "C"
