// cnn_grad.hip -- the learning half of the pixel agent: the REINFORCE loss of
// examples/ball_cnn_reinforce.py:98-117 (finish_episode: sum of -Categorical(probs).log_prob(a) * R^) over
// recorded rows and its gradients with respect to the conv net's 14 parameters, straight from the u8 images.
//
//   be_cnn_grad          forward (be_cnn_act's pinned arithmetic, per-image BatchNorm statistics), the row loss,
//                        backward, gradient sums over all rows (the computation include/ballenv.h pins)
//   be_observe_quadrant  the goal's quadrant of every env, the byte be_cnn_act computes when quadrant_in is NULL
//
// Three kernels, no float atomics, so the result is reproducible bit for bit (mlp_grad.hip's scheme):
//
//   cnn_grad_pack     the weights into the head of the workspace: be_cnn_act's packed image (cnn_host.h) for the
//                     forward, and conv2 / conv3 transposed (cnn_grad_host.h) for dy = W^T dconv
//   cnn_grad_kernel   one workgroup of 8 waves per CU, each looping over tiles of 2 rows (tile b, b + G, ...
//                     for workgroup b of G).  A tile's activations live in LDS: per layer the normalised map
//                     xhat and the output y = relu(gamma xhat + beta); the backward overwrites y with dy and
//                     xhat with dconv.  The weight-gradient accumulators stay in registers for the whole
//                     kernel; at the end every workgroup writes its sums to its slot of the workspace.
//   cnn_grad_reduce   one thread per gradient element: the slots added in workgroup order in f64 (a gradient
//                     held as several partial sums per slot: those in order), times scale, rounded once to f32;
//                     the conv biases exact +0; two threads do the same for the f64 losses.
//
// Every matrix product runs on v_mfma_f32_16x16x4_f32 (an exact f32 fma chain); lane l = 16 l4 + l15 holds
// A[row l15][k l4] and B[k l4][column l15] of a step and C[row 4 l4 + r][column l15], r = 0..3.  Per round,
// a workgroup barrier between the phases, e = a row of the tile:
//   F0  the images into LDS; quadrant, action, coef, valid of the rows
//   F1..F7  be_cnn_act's forward, the same operands in the same chains (cnn_policy.hip's phases 1..7 on
//       2 x 324, 2 x 49 and 2 x 4 columns), except that each BatchNorm writes xhat, y and the map's
//       1 / sqrt(var + eps), and that the head ends in policy_dist's softmax into LDS
//   B1  lane e of wave 0: the row loss and dz (16 values) -> LDS; dz_a = -c (sum of the other p_j, in action
//       order), which is c (p_a - 1) without its cancellation where p_a is near 1
//   B2  gW_head += dz (x) [y3, onehot]: A[j][k = e] = dz, B[k = e][f] = the feature, one step per round (k = 2, 3
//       zero); wave w the features 16 w .. 16 w + 15, wave 0 also the one-hot's four.  gb_head += dz: thread
//       16 e + j.  dy3 = W_head^T dz: A[f][k = j] = W_head[j][f] (registers), B[k = j][e] = dz, steps j / 4 in
//       order, wave w its 16 features; dy3 over y3
//   B3  bn3 backward, 4 threads per map (the sums as the forward's: interleaved partials, combined pairwise):
//       dyr = (xhat gamma + beta > 0) ? dy : 0, gbeta += sum dyr, ggamma += sum dyr xhat,
//       dconv = (gamma inv) ((dyr - (sum dyr) / n) - xhat ((sum dyr xhat) / n)) over xhat
//   B4  gW3 += dconv3 (x) y2 patches: A[co][k = position] = dconv3, B[k = position][(ci, tap)] = y2, one step
//       per row (4 positions), row 0 then row 1; accumulator tile q = 50 rt + ct (16 co x 16 of the 800 (ci, tap)),
//       wave w the tiles w, w + 8, ...
//   B5  dy2 = W3^T dconv3 over y2, the 7 x 7 positions split by the parity of (y, x): a class (py, px) takes the
//       taps ky = py + 2 m, kx = px + 2 n in (m, n) order and within a tap the steps co / 4 in order,
//       A[ci][k = co] = W3[co][ci][tap] (workspace), B[k = co][column] = dconv3[co][a - m][b - n] or 0 outside
//       the 2 x 2 map, column = (e, a, b) of y = 2 a + py, x = 2 b + px; one chain from 0 per output
//   B6  bn2 backward, 8 threads per map
//   B7  gW2 += dconv2 (x) y1 patches: 13 steps per row (positions 4 s + l4, zero behind 48), row 0's then row
//       1's; tile q = 25 rt + ct
//   B8  dy1 = W2^T dconv2 over y1, as B5 on 18 x 18 positions
//   B9  bn1 backward, 16 threads per map
//   B10 gW1 += dconv1 (x) image patches: 81 steps per row (positions 4 s + l4); wave w takes the steps w, w + 8,
//       ... of row 0, then of row 1, into its own partial of the 5 tiles (16 co x 75 (ci, tap))
// A row past `rows` is staged as a zero image and is inactive, like a row with valid = 0 or an action >=
// num_actions: its dz are exact zeros, so every product it adds is a zero.
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "ballenv.h"
#include "blocks_core.h"
#include "cnn_grad_host.h"
#include "cnn_host.h"
#include "internal.h"
#include "mlp_core.h"
#include "philox.h"
#include "policy_core.h"

namespace {

using namespace behost;

constexpr int GT = CNN_GRAD_TILE, GW = CNN_GRAD_WAVES, G_THREADS = 64 * GW;
static_assert(GW == 8 && GT == 2, "the phases' work split is written for 8 waves and 2 rows");
constexpr float CNN_EPS = 1e-5f;

struct GPack {
  const float* t[CNN_TENSORS];     // the running statistics' entries are NULL
  int32_t A;
};

__global__ __launch_bounds__(256) void cnn_grad_pack(GPack a, float* ws) {
  for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < CNN_G_PACK; i += (int)gridDim.x * 256) {
    int elem;
    const int src = i < CNN_TOTAL ? cnn_pack_source(i, a.A, &elem) : cnn_grad_pack_source(i - CNN_G_T2, &elem);
    float v = src == CNN_SRC_NEGINF ? -INFINITY : 0.0f;
    if (src >= 0) {
      const float* t = a.t[0];
#pragma unroll
      for (int k = 1; k < CNN_TENSORS; ++k) t = src == k ? a.t[k] : t;
      if (t) v = t[elem];
    }
    ws[i] = v;
  }
}

struct GParams {
  const float* pack;                 // the workspace's head
  const float* head_w;               // (A, 132)
  const uint8_t* images; const uint8_t* quadrants; const uint8_t* actions;
  const float* coef; const uint8_t* valid;      // may be NULL
  float* probs;                      // (rows, A) or NULL
  uint8_t* slots;
  int64_t rows, ntiles;
  int32_t A;
  CnnGradSlot S;
};

template <int P>
__device__ __forceinline__ float g_tree(float s) {
#pragma unroll
  for (int m = 1; m < P; m <<= 1) s = s + __shfl_xor(s, m);
  return s;
}

// BatchNorm + relu of one map (cnn_policy.hip's cnn_norm_map in sample mode, the same operations): conv in X
// -> xhat in X, y in Y, *invp = 1 / sqrt(var + eps)
template <int NPOS, int P>
__device__ __forceinline__ void g_norm_fwd(float* X, float* Y, float* invp, int j, float gamma, float beta) {
  constexpr int NI = (NPOS + P - 1) / P;
  float v[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) v[i] = X[min(j + P * i, NPOS - 1)];
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < NI; ++i) s = j + P * i < NPOS ? s + v[i] : s;
  const float mean = g_tree<P>(s) / (float)NPOS;
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const float d = v[i] - mean;
    q = j + P * i < NPOS ? q + d * d : q;
  }
  const float var = g_tree<P>(q) / (float)NPOS;
  const float inv = 1.0f / sqrtf(var + CNN_EPS);
  if (j == 0) *invp = inv;
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (j + P * i < NPOS) {
      const float xh = (v[i] - mean) * inv;
      X[j + P * i] = xh;
      Y[j + P * i] = fmaxf(xh * gamma + beta, 0.0f);
    }
}

// BatchNorm + relu backward of one map by P threads: xhat in X -> dconv in X, dy read from DY
template <int NPOS, int P>
__device__ __forceinline__ void g_norm_bwd(float* X, const float* DY, int j, float gamma, float beta, float inv,
                                           float& ggamma, float& gbeta) {
  constexpr int NI = (NPOS + P - 1) / P;
  float xh[NI], d[NI];
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int k = min(j + P * i, NPOS - 1);
    xh[i] = X[k];
    d[i] = (xh[i] * gamma + beta > 0.0f) ? DY[k] : 0.0f;
    if (j + P * i < NPOS) {
      s1 = s1 + d[i];
      s2 = s2 + d[i] * xh[i];
    }
  }
  s1 = g_tree<P>(s1);
  s2 = g_tree<P>(s2);
  gbeta = gbeta + s1;
  ggamma = ggamma + s2;
  const float k = gamma * inv, m1 = s1 / (float)NPOS, m2 = s2 / (float)NPOS;
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (j + P * i < NPOS) X[j + P * i] = k * ((d[i] - m1) - xh[i] * m2);
}

// conv2 for one wave (cnn_policy.hip's cnn_conv2 on GT rows): row tile rt, the NCT column tiles j0, j0 + 4, ...
template <int NCT>
__device__ __forceinline__ void g_conv2(const float* g2, const float* Y1, float* X2, const float* bias, int j0, int rt,
                                        int l15, int l4) {
  int base[NCT], p[NCT];
  f32x4 acc[NCT];
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    p[c] = 16 * (j0 + 4 * c) + l15;
    const int pc = min(p[c], GT * CNN_N2 - 1);
    const int env = pc / CNN_N2, pos = pc - CNN_N2 * env, oy = pos / CNN_S2, ox = pos - CNN_S2 * oy;
    base[c] = (env * CNN_C1 + l4) * CNN_N1 + 2 * oy * CNN_S1 + 2 * ox;
    acc[c] = *(const f32x4*)bias;
  }
  constexpr int ROWS = (CNN_C1 / 4) * CNN_KS;
  float a[2][CNN_KS];
#pragma unroll
  for (int kx = 0; kx < CNN_KS; ++kx) a[0][kx] = g2[kx * 128];
#pragma unroll 1
  for (int row = 0; row < ROWS; row += 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cur = row + h, nxt = min(cur + 1, ROWS - 1);
#pragma unroll
      for (int kx = 0; kx < CNN_KS; ++kx) a[h ^ 1][kx] = g2[(nxt * CNN_KS + kx) * 128];
      const int cg = cur / CNN_KS, ky = cur - CNN_KS * cg;
      const int off = cg * 4 * CNN_N1 + ky * CNN_S1;
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kx = 0; kx < CNN_KS; ++kx)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[c] = BE_MFMA(a[h][kx], Y1[base[c] + off + kx], acc[c]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    if (p[c] < GT * CNN_N2) {
      const int env = p[c] / CNN_N2, pos = p[c] - CNN_N2 * env;
#pragma unroll
      for (int r = 0; r < 4; ++r) X2[(env * CNN_C2 + 16 * rt + 4 * l4 + r) * CNN_N2 + pos] = acc[c][r];
    }
  }
}

// dy = W^T dconv of a 5 x 5 stride-2 convolution with 32 output channels: DC [GT][32][SOUT^2] -> DY
// [GT][CIN][SIN^2], every element written.  T: the transposed weights, [tap][co / 4][CIN / 16][64].
template <int CIN, int SIN, int SOUT>
__device__ __forceinline__ void g_dgrad(const float* T, const float* DC, float* DY, int wave, int lane) {
  constexpr int RT = CIN / 16, NA0 = (SIN + 1) / 2, NA1 = SIN / 2, SO2 = SOUT * SOUT, SI2 = SIN * SIN;
  constexpr int CTS = (GT * NA0 * NA0 + 15) / 16;              // column tiles of the largest class
  const int l15 = lane & 15, l4 = lane >> 4;
  for (int u = wave; u < 4 * RT * CTS; u += GW) {
    const int cls = u / (RT * CTS), v = u - cls * (RT * CTS), rt = v / CTS, ct = v - rt * CTS;
    const int py = cls >> 1, px = cls & 1;
    const int na = py ? NA1 : NA0, nb = px ? NA1 : NA0, ncols = GT * na * nb;
    if (16 * ct >= ncols) continue;
    const int col = 16 * ct + l15, cc = min(col, ncols - 1);
    const int env = cc / (na * nb), rem = cc - env * (na * nb), a = rem / nb, b = rem - a * nb;
    const int nm = py ? 2 : 3, nn = px ? 2 : 3;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int m = 0; m < nm; ++m)
      for (int n = 0; n < nn; ++n) {
        const int tap = (py + 2 * m) * CNN_KS + px + 2 * n, oy = a - m, ox = b - n;
        const bool ok = (unsigned)oy < (unsigned)SOUT && (unsigned)ox < (unsigned)SOUT;
        const float* dc = DC + (env * 32 + l4) * SO2 + (ok ? oy * SOUT + ox : 0);
        const float* t = T + ((tap * 8) * RT + rt) * 64 + lane;
        float af[8];
#pragma unroll
        for (int cs = 0; cs < 8; ++cs) af[cs] = t[cs * RT * 64];
#pragma unroll
        for (int cs = 0; cs < 8; ++cs) {
          const float bv = dc[4 * cs * SO2];
          acc = BE_MFMA(af[cs], ok ? bv : 0.0f, acc);
        }
      }
    if (col < ncols) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        DY[(env * CIN + 16 * rt + 4 * l4 + r) * SI2 + (2 * a + py) * SIN + 2 * b + px] = acc[r];
    }
  }
}

// the B operand's column offset of a weight-gradient tile: column = (ci, tap) -> ci * plane + ky * side + kx
__device__ __forceinline__ int g_coloff(int col, int plane, int side) {
  const int ci = col / CNN_TAPS, tap = col - CNN_TAPS * ci, ky = tap / CNN_KS;
  return ci * plane + ky * side + (tap - CNN_KS * ky);
}

constexpr int NT3 = 13, NT2 = 7, NT1 = 5;      // accumulator tiles per wave of gW3 (100), gW2 (50), gW1 (5, a partial)

__global__ __launch_bounds__(G_THREADS) void cnn_grad_kernel(GParams p) {
  extern __shared__ uint4 g_lds[];
  float* S = (float*)g_lds;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int A = p.A;
  stage_image<G_THREADS, 2>(g_lds, (const uint4*)p.pack, CNN_STAGED / 4, tid);
  if (tid < 256) S[CNN_GL_LUT + tid] = (float)tid / 255.0f;
  const float* LUT = S + CNN_GL_LUT;
  float* X1 = S + CNN_GL_X1;
  float* Y1 = S + CNN_GL_Y1;
  float* X2 = S + CNN_GL_X2;
  float* Y2 = S + CNN_GL_Y2;
  float* X3 = S + CNN_GL_X3;
  float* Y3 = S + CNN_GL_Y3;
  float* INV1 = S + CNN_GL_INV;
  float* INV2 = INV1 + GT * CNN_C1;
  float* INV3 = INV2 + GT * CNN_C2;
  float* P3 = S + CNN_GL_PART;
  float* Zs = S + CNN_GL_ZS;
  float* PR = S + CNN_GL_PR;
  float* DZ = S + CNN_GL_DZ;
  int* QD = (int*)(S + CNN_GL_ROW);
  uint8_t* IMG = (uint8_t*)(S + CNN_GL_IMG);
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  int off4[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = min(4 * q + l4, 14);
    off4[q] = (j / 5) * CNN_IMG * CNN_IMG + (j % 5) * CNN_IMG + 4;
  }
  const int rt = wave & 1, wq = wave >> 1;

  // W_head^T as the A fragments of dy3: A[f = 16 wave + l15][k = j = 4 s + l4]
  float wht[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j = 4 * s + l4;
    wht[s] = j < A ? p.head_w[j * CNN_HEAD_IN + 16 * wave + l15] : 0.0f;
  }
  f32x4 g3[NT3], g2[NT2], g1[NT1], gh = zero4, gh8 = zero4;
#pragma unroll
  for (int i = 0; i < NT3; ++i) g3[i] = zero4;
#pragma unroll
  for (int i = 0; i < NT2; ++i) g2[i] = zero4;
#pragma unroll
  for (int i = 0; i < NT1; ++i) g1[i] = zero4;
  float gG1 = 0.0f, gB1 = 0.0f, gG2 = 0.0f, gB2 = 0.0f, gG3 = 0.0f, gB3 = 0.0f, gbh = 0.0f;
  double ls = 0.0, cnt = 0.0;
  __syncthreads();

  for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int64_t e0 = tile * GT;
    const int nv = (int)(p.rows - e0 < GT ? p.rows - e0 : GT);

    // F0: the images (a row past the end is all zero bytes), the quadrants
    {
      const uint4* src = (const uint4*)(p.images + e0 * CNN_IMG_BYTES);
      constexpr int W16 = CNN_IMG_BYTES / 16;
      for (int k = tid; k < GT * W16; k += G_THREADS) ((uint4*)IMG)[k] = k < nv * W16 ? src[k] : uint4{0u, 0u, 0u, 0u};
      if (tid < GT) QD[tid] = tid < nv ? (p.quadrants[e0 + tid] & 3) : 0;
    }
    __syncthreads();

    // F1: conv1, two column tiles at a time (a pad column computes the last one's and writes nothing)
    constexpr int T1 = (GT * CNN_N1 + 15) / 16;
    for (int tA = wave; tA < T1; tA += 16) {
      const bool hasB = tA + 8 < T1;
      const int qA = 16 * tA + l15, qB = 16 * (hasB ? tA + 8 : tA) + l15;
      const int pA = min(qA, GT * CNN_N1 - 1), pB = min(qB, GT * CNN_N1 - 1);
      const int envA = pA / CNN_N1, posA = pA - CNN_N1 * envA, oyA = posA / CNN_S1, oxA = posA - CNN_S1 * oyA;
      const int envB = pB / CNN_N1, posB = pB - CNN_N1 * envB, oyB = posB / CNN_S1, oxB = posB - CNN_S1 * oyB;
      const uint8_t* iA = IMG + envA * CNN_IMG_BYTES + 2 * oyA * CNN_IMG + 2 * oxA;
      const uint8_t* iB = IMG + envB * CNN_IMG_BYTES + 2 * oyB * CNN_IMG + 2 * oxB;
      f32x4 accA = *(const f32x4*)(S + CNN_P1 + 4 * l4), accB = accA;
      // the steps in be_cnn_act's order; the first 15 as a loop (their offsets are linear in (ci, ky)), which
      // keeps the operands of a few steps in registers, not of all 19
#pragma unroll 1
      for (int ci = 0; ci < CNN_C0; ++ci) {
#pragma unroll
        for (int ky = 0; ky < CNN_KS; ++ky) {
          const int off = ci * CNN_IMG * CNN_IMG + ky * CNN_IMG + l4;
          const float a = S[CNN_F1 + (ci * CNN_KS + ky) * 64 + lane];
          accA = BE_MFMA(a, LUT[iA[off]], accA);
          accB = BE_MFMA(a, LUT[iB[off]], accB);
        }
      }
#pragma unroll
      for (int s = 15; s < CNN_K1; ++s) {
        const float a = S[CNN_F1 + s * 64 + lane];
        accA = BE_MFMA(a, LUT[iA[off4[s - 15]]], accA);
        accB = BE_MFMA(a, LUT[iB[off4[s - 15]]], accB);
      }
      if (qA < GT * CNN_N1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) X1[(envA * CNN_C1 + 4 * l4 + r) * CNN_N1 + posA] = accA[r];
      }
      if (hasB && qB < GT * CNN_N1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) X1[(envB * CNN_C1 + 4 * l4 + r) * CNN_N1 + posB] = accB[r];
      }
    }
    __syncthreads();

    // F2: bn1 + relu: map tid >> 3 = row * 16 + channel, 8 threads per map
    if (tid < GT * CNN_C1 * 8) {
      const int map = tid >> 3, ch = map & (CNN_C1 - 1);
      g_norm_fwd<CNN_N1, 8>(X1 + map * CNN_N1, Y1 + map * CNN_N1, INV1 + map, tid & 7, S[CNN_P1 + CNN_C1 + ch],
                            S[CNN_P1 + 2 * CNN_C1 + ch]);
    }
    __syncthreads();

    // F3: conv2: 7 column tiles of 2 x 49 columns
    {
      const float* gf = p.pack + CNN_F2 + 64 * rt + lane;
      const float* bias = S + CNN_P2 + 16 * rt + 4 * l4;
      if (wq < 3) g_conv2<2>(gf, Y1, X2, bias, wq, rt, l15, l4);
      else g_conv2<1>(gf, Y1, X2, bias, wq, rt, l15, l4);
    }
    __syncthreads();

    // F4: bn2 + relu: map tid >> 2 = row * 32 + channel, 4 threads per map
    if (tid < GT * CNN_C2 * 4) {
      const int map = tid >> 2, ch = map & (CNN_C2 - 1);
      g_norm_fwd<CNN_N2, 4>(X2 + map * CNN_N2, Y2 + map * CNN_N2, INV2 + map, tid & 3, S[CNN_P2 + CNN_C2 + ch],
                            S[CNN_P2 + 2 * CNN_C2 + ch]);
    }
    __syncthreads();

    // F5: conv3: column l15 & 7 = row * 4 + position (columns 8..15 repeat them); chains 2 wq and 2 wq + 1
    {
      const int env = (l15 >> 2) & 1, oy = (l15 >> 1) & 1, ox = l15 & 1;
      const int base = (env * CNN_C2 + 8 * wq + l4) * CNN_N2 + 2 * oy * CNN_S2 + 2 * ox;
      const float* gf = p.pack + CNN_F3 + (2 * wq * CNN_TAPS) * 128 + 64 * rt + lane;
      f32x4 k0 = wq == 0 ? *(const f32x4*)(S + CNN_P3 + 16 * rt + 4 * l4) : zero4, k1 = zero4;
      float a0[CNN_KS], a1[CNN_KS], n0[CNN_KS], n1[CNN_KS];
#pragma unroll
      for (int kx = 0; kx < CNN_KS; ++kx) { a0[kx] = gf[kx * 128]; a1[kx] = gf[(CNN_TAPS + kx) * 128]; }
#pragma unroll 1
      for (int ky = 0; ky < CNN_KS; ++ky) {
        const int nk = min(ky + 1, CNN_KS - 1);
#pragma unroll
        for (int kx = 0; kx < CNN_KS; ++kx) {
          n0[kx] = gf[(nk * CNN_KS + kx) * 128];
          n1[kx] = gf[(CNN_TAPS + nk * CNN_KS + kx) * 128];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kx = 0; kx < CNN_KS; ++kx) {
          const int off = ky * CNN_S2 + kx;
          k0 = BE_MFMA(a0[kx], Y2[base + off], k0);
          k1 = BE_MFMA(a1[kx], Y2[base + 4 * CNN_N2 + off], k1);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kx = 0; kx < CNN_KS; ++kx) { a0[kx] = n0[kx]; a1[kx] = n1[kx]; }
      }
      *(f32x4*)(P3 + ((rt * 8 + 2 * wq) * 64 + lane) * 4) = k0;
      *(f32x4*)(P3 + ((rt * 8 + 2 * wq + 1) * 64 + lane) * 4) = k1;
    }
    __syncthreads();

    // F6: the eight chains' sum, bn3 + relu: thread = (row * 32 + channel) * 4 + position
    if (tid < GT * CNN_C3 * 4) {
      const int env = tid >> 7, ch = (tid >> 2) & 31, pos = tid & 3, map = tid >> 2;
      const float* c = P3 + (((ch >> 4) * 8) * 64 + ((ch >> 2) & 3) * 16 + env * 4 + pos) * 4 + (ch & 3);
      X3[map * CNN_N3 + pos] = ((c[0] + c[256]) + (c[512] + c[768])) + ((c[1024] + c[1280]) + (c[1536] + c[1792]));
      g_norm_fwd<CNN_N3, 4>(X3 + map * CNN_N3, Y3 + map * CNN_N3, INV3 + map, pos, S[CNN_P3 + CNN_C3 + ch],
                            S[CNN_P3 + 2 * CNN_C3 + ch]);
    }
    __syncthreads();

    // F7 + B1: wave 0: the head (column l15 is row l15 & 1), the softmax, the row loss and dz
    if (wave == 0) {
      const int env = l15 & (GT - 1);
      f32x4 c[4] = {*(const f32x4*)(S + CNN_HBIAS + 4 * l4), zero4, zero4, zero4};
#pragma unroll
      for (int s = 0; s < CNN_KH - 1; ++s)
        c[s & 3] = BE_MFMA(S[CNN_FH + s * 64 + lane], Y3[env * CNN_FEAT + 4 * s + l4], c[s & 3]);
      c[0] = BE_MFMA(S[CNN_FH + (CNN_KH - 1) * 64 + lane], l4 == QD[env] ? 1.0f : 0.0f, c[0]);
      const f32x4 z = (c[0] + c[1]) + (c[2] + c[3]);
      if (l15 < GT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Zs[l15 * CNN_ZP + 4 * l4 + r] = z[r];
      }
      wave_sync();
      if (lane < GT) {
        float* pr = PR + lane * CNN_NO;
        (void)policy_dist<CNN_NO>(Zs + lane * CNN_ZP, S + CNN_HB, A, pr);
        int act = 255, vld = 0;
        float cf = 0.0f;
        if (lane < nv) {
          const int64_t e = e0 + lane;
          act = p.actions[e];
          cf = p.coef ? p.coef[e] : 1.0f;
          vld = p.valid ? p.valid[e] : 1;
          if (p.probs)
            for (int j = 0; j < A; ++j) p.probs[e * A + j] = pr[j];
        }
        const bool active = vld != 0 && act < A;
        bool pass = active;
        if (active) {
          const float pa = pr[act], lo = FLT_EPSILON, hi = 1.0f - FLT_EPSILON;
          ls += (double)(-(cf * logf(fminf(fmaxf(pa, lo), hi))));
          cnt += 1.0;
          pass = pa >= lo && pa <= hi;
        }
        // p_a - 1 as minus the sum of the other probabilities, in action order: p_a near 1 cancels nothing
        float rest = 0.0f;
        for (int j = 0; j < A; ++j) rest = j != act ? rest + pr[j] : rest;
        for (int j = 0; j < CNN_NO; ++j)
          DZ[lane * CNN_NO + j] = (pass && j < A) ? (j == act ? -(cf * rest) : cf * pr[j]) : 0.0f;
      }
    }
    __syncthreads();

    // B2: gW_head, gb_head, dy3 over y3
    {
      const float a = l4 < GT ? DZ[l4 * CNN_NO + l15] : 0.0f;                         // A[j][k = row]
      const float b = l4 < GT ? Y3[l4 * CNN_FEAT + 16 * wave + l15] : 0.0f;           // B[k = row][f]
      gh = BE_MFMA(a, b, gh);
      if (wave == 0) gh8 = BE_MFMA(a, (l4 < GT && l15 < 4 && QD[l4 & (GT - 1)] == l15) ? 1.0f : 0.0f, gh8);
      if (tid < GT * CNN_NO) gbh = gbh + DZ[tid];
      f32x4 d = zero4;
#pragma unroll
      for (int s = 0; s < 4; ++s) d = BE_MFMA(wht[s], DZ[(l15 & (GT - 1)) * CNN_NO + 4 * s + l4], d);
      if (l15 < GT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Y3[l15 * CNN_FEAT + 16 * wave + 4 * l4 + r] = d[r];
      }
    }
    __syncthreads();

    // B3: bn3 backward
    if (tid < GT * CNN_C3 * 4) {
      const int map = tid >> 2, ch = map & (CNN_C3 - 1);
      g_norm_bwd<CNN_N3, 4>(X3 + map * CNN_N3, Y3 + map * CNN_N3, tid & 3, S[CNN_P3 + CNN_C3 + ch],
                            S[CNN_P3 + 2 * CNN_C3 + ch], INV3[map], gG3, gB3);
    }
    __syncthreads();

    // B4: gW3 += dconv3 (x) y2 patches
    {
      const int po = 2 * (l4 >> 1) * CNN_S2 + 2 * (l4 & 1);
#pragma unroll
      for (int env = 0; env < GT; ++env) {
        const float a0 = X3[env * CNN_FEAT + l15 * CNN_N3 + l4], a1 = X3[env * CNN_FEAT + (16 + l15) * CNN_N3 + l4];
        const float* y = Y2 + env * CNN_C2 * CNN_N2 + po;
#pragma unroll
        for (int i = 0; i < NT3; ++i) {
          const bool hi = wave + GW * i >= 50;               // tiles 50..99: output channels 16..31
          const int q = min(wave + GW * i, 99);
          g3[i] = BE_MFMA(hi ? a1 : a0, y[g_coloff(16 * (q % 50) + l15, CNN_N2, CNN_S2)], g3[i]);
        }
      }
    }
    __syncthreads();

    // B5: dy2 over y2
    g_dgrad<CNN_C2, CNN_S2, CNN_S3>(p.pack + CNN_G_T3, X3, Y2, wave, lane);
    __syncthreads();

    // B6: bn2 backward: map tid >> 3, 8 threads per map
    {
      const int map = tid >> 3, ch = map & (CNN_C2 - 1);
      g_norm_bwd<CNN_N2, 8>(X2 + map * CNN_N2, Y2 + map * CNN_N2, tid & 7, S[CNN_P2 + CNN_C2 + ch],
                            S[CNN_P2 + 2 * CNN_C2 + ch], INV2[map], gG2, gB2);
    }
    __syncthreads();

    // B7: gW2 += dconv2 (x) y1 patches
#pragma unroll 1
    for (int env = 0; env < GT; ++env) {
#pragma unroll 1
      for (int s = 0; s < (CNN_N2 + 3) / 4; ++s) {
        const int pos = 4 * s + l4, pc = min(pos, CNN_N2 - 1), oy = pc / CNN_S2, ox = pc - CNN_S2 * oy;
        const float x0 = X2[(env * CNN_C2 + l15) * CNN_N2 + pc], x1 = X2[(env * CNN_C2 + 16 + l15) * CNN_N2 + pc];
        const float a0 = pos < CNN_N2 ? x0 : 0.0f, a1 = pos < CNN_N2 ? x1 : 0.0f;
        const float* y = Y1 + env * CNN_C1 * CNN_N1 + 2 * oy * CNN_S1 + 2 * ox;
#pragma unroll
        for (int i = 0; i < NT2; ++i) {
          const bool hi = wave + GW * i >= 25;
          const int q = min(wave + GW * i, 49);
          g2[i] = BE_MFMA(hi ? a1 : a0, y[g_coloff(16 * (q % 25) + l15, CNN_N1, CNN_S1)], g2[i]);
        }
      }
    }
    __syncthreads();

    // B8: dy1 over y1
    g_dgrad<CNN_C1, CNN_S1, CNN_S2>(p.pack + CNN_G_T2, X2, Y1, wave, lane);
    __syncthreads();

    // B9: bn1 backward: map tid >> 4, 16 threads per map
    {
      const int map = tid >> 4, ch = map & (CNN_C1 - 1);
      g_norm_bwd<CNN_N1, 16>(X1 + map * CNN_N1, Y1 + map * CNN_N1, tid & 15, S[CNN_P1 + CNN_C1 + ch],
                             S[CNN_P1 + 2 * CNN_C1 + ch], INV1[map], gG1, gB1);
    }
    __syncthreads();

    // B10: gW1 += dconv1 (x) image patches, this wave's steps
#pragma unroll 1
    for (int env = 0; env < GT; ++env) {
#pragma unroll 1
      for (int s = wave; s < CNN_N1 / 4; s += GW) {
        const int pos = 4 * s + l4, oy = pos / CNN_S1, ox = pos - CNN_S1 * oy;
        const float a = X1[(env * CNN_C1 + l15) * CNN_N1 + pos];
        const uint8_t* im = IMG + env * CNN_IMG_BYTES + 2 * oy * CNN_IMG + 2 * ox;
#pragma unroll
        for (int i = 0; i < NT1; ++i)
          g1[i] = BE_MFMA(a, LUT[im[g_coloff(min(16 * i + l15, CNN_C0 * CNN_TAPS - 1), CNN_IMG * CNN_IMG, CNN_IMG)]], g1[i]);
      }
    }
    __syncthreads();
  }

  // this workgroup's sums into its slot: every element of the slot is written
  const CnnGradSlot& L = p.S;
  float* slot = (float*)(p.slots + (int64_t)blockIdx.x * L.slot_bytes);
#pragma unroll
  for (int i = 0; i < NT3; ++i) {
    const int q = wave + GW * i;
    if (q < 100) {
#pragma unroll
      for (int r = 0; r < 4; ++r) slot[L.o_w3 + (16 * (q / 50) + 4 * l4 + r) * (CNN_C2 * CNN_TAPS) + 16 * (q % 50) + l15] = g3[i][r];
    }
  }
#pragma unroll
  for (int i = 0; i < NT2; ++i) {
    const int q = wave + GW * i;
    if (q < 50) {
#pragma unroll
      for (int r = 0; r < 4; ++r) slot[L.o_w2 + (16 * (q / 25) + 4 * l4 + r) * (CNN_C1 * CNN_TAPS) + 16 * (q % 25) + l15] = g2[i][r];
    }
  }
#pragma unroll
  for (int i = 0; i < NT1; ++i) {
    const int col = 16 * i + l15;
    if (col < CNN_C0 * CNN_TAPS) {
#pragma unroll
      for (int r = 0; r < 4; ++r) slot[L.o_w1 + wave * CNN_G_W1 + (4 * l4 + r) * (CNN_C0 * CNN_TAPS) + col] = g1[i][r];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = 4 * l4 + r;
    if (j < A) {
      slot[L.o_wh + j * CNN_HEAD_IN + 16 * wave + l15] = gh[r];
      if (wave == 0 && l15 < 4) slot[L.o_wh + j * CNN_HEAD_IN + CNN_FEAT + l15] = gh8[r];
    }
  }
  if (tid < GT * CNN_NO) slot[L.o_bh + tid] = gbh;
  if ((tid & 15) == 0) { slot[L.o_g1 + (tid >> 4)] = gG1; slot[L.o_b1 + (tid >> 4)] = gB1; }
  if ((tid & 7) == 0) { slot[L.o_g2 + (tid >> 3)] = gG2; slot[L.o_b2 + (tid >> 3)] = gB2; }
  if ((tid & 3) == 0 && tid < GT * CNN_C3 * 4) { slot[L.o_g3 + (tid >> 2)] = gG3; slot[L.o_b3 + (tid >> 2)] = gB3; }
  if (tid < GT) {
    double* out = (double*)(p.slots + (int64_t)blockIdx.x * L.slot_bytes + L.loss_off) + 2 * tid;
    out[0] = ls; out[1] = cnt;
  }
}

struct RParams {
  const uint8_t* slots; int32_t nslots, A; CnnGradSlot S; double scale;
  float* g[14]; double* losses;
};

__global__ __launch_bounds__(256) void cnn_grad_reduce(RParams p) {
  const CnnGradSlot& L = p.S;
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i < L.outputs) {
    const CnnGradOut o = cnn_grad_output(i, p.A);
    double s = 0.0;
    for (int sl = 0; sl < p.nslots; ++sl) {
      const float* slot = (const float*)(p.slots + (int64_t)sl * L.slot_bytes);
      for (int q = 0; q < o.parts; ++q) s += (double)slot[o.off + q * o.stride];
    }
    float* dst = p.g[0];
#pragma unroll
    for (int k = 1; k < 14; ++k) dst = o.tensor == k ? p.g[k] : dst;
    dst[o.elem] = o.parts ? (float)(s * p.scale) : 0.0f;
  } else if (i < L.outputs + 2) {
    const int k = i - L.outputs;
    double s = 0.0;
    for (int sl = 0; sl < p.nslots; ++sl)
      for (int q = 0; q < GT; ++q) s += ((const double*)(p.slots + (int64_t)sl * L.slot_bytes + L.loss_off))[2 * q + k];
    p.losses[k] = k == 0 ? s * p.scale : s;
  }
}

__global__ __launch_bounds__(256) void quadrant_kernel(const int32_t* agent, const int32_t* goal, uint8_t* out, int n) {
  const int e = (int)(blockIdx.x * 256 + threadIdx.x);
  if (e >= n) return;
  const int32_t a = agent[e], g = goal[e];                  // blocks_init's rule (blocks_core.h)
  const int dx = px(g) - px(a), dy = py(g) - py(a);
  out[e] = (uint8_t)(dx >= 0 ? (dy >= 0 ? 1 : 2) : (dy >= 0 ? 0 : 3));
}

// workgroups of the persistent grid = slots of the workspace: one per CU of ctx's device
int grad_slots(int device) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) return 0;
  return cus < CNN_GRAD_MAX_SLOTS ? cus : CNN_GRAD_MAX_SLOTS;
}

// cnn_grad_kernel's LDS is above the default limit: the attribute is set once per device, the first time
// be_cnn_grad_workspace_bytes (which every caller needs before be_cnn_grad) or be_cnn_grad runs on it -- so a
// be_cnn_grad under stream capture makes no such call.  The current device is `device`.
hipError_t grad_lds_attribute(int device) {
  static bool done[64] = {};
  if (device >= 0 && device < 64 && done[device]) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)cnn_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           CNN_GRAD_LDS_BYTES);
  if (e == hipSuccess && device >= 0 && device < 64) done[device] = true;
  return e;
}

}  // namespace

extern "C" {

int64_t be_cnn_grad_workspace_bytes(be_ctx* ctx, int32_t num_actions) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  if (num_actions < 1 || num_actions > CNN_MAXA)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_cnn_grad_workspace_bytes: num_actions must be in [1, 15]");
  const be_ctx_view cv = be_ctx_get(ctx);
  const int slots = grad_slots(cv.device);
  if (slots < 1) return be_ctx_fail(ctx, BE_E_HIP, "be_cnn_grad: cannot query the device's compute units");
  BE_ENTER_DEVICE(be_ctx_err(ctx), cv.device);
  BE_HIP_TRY(be_ctx_err(ctx), grad_lds_attribute(cv.device));
  return cnn_grad_workspace_bytes(slots, num_actions);
}

int be_cnn_grad(be_ctx* ctx, const uint8_t* images, const uint8_t* quadrants, const uint8_t* actions, const float* coef,
                const uint8_t* valid, int64_t rows, double scale, const be_cnn_weights* w, int32_t num_actions,
                void* workspace, int64_t workspace_bytes, const be_cnn_grads* g, void* stream) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  const be_ctx_view cv = be_ctx_get(ctx);
  const int slots = grad_slots(cv.device);
  if (slots < 1) return be_ctx_fail(ctx, BE_E_HIP, "be_cnn_grad: cannot query the device's compute units");
  const char* field = nullptr;
  if (const char* msg = cnn_grad_args_error(images, quadrants, actions, rows, w, num_actions, workspace, workspace_bytes,
                                            g, slots, &field))
    return be_fail(be_ctx_err(ctx), BE_E_INVALID, msg, field);
  BE_ENTER_DEVICE(be_ctx_err(ctx), cv.device);
  BE_HIP_TRY(be_ctx_err(ctx), grad_lds_attribute(cv.device));
  hipStream_t hs = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const GPack pk{{w->conv1_weight, w->conv1_bias, w->bn1_weight, w->bn1_bias, nullptr, nullptr,
                  w->conv2_weight, w->conv2_bias, w->bn2_weight, w->bn2_bias, nullptr, nullptr,
                  w->conv3_weight, w->conv3_bias, w->bn3_weight, w->bn3_bias, nullptr, nullptr,
                  w->head_weight, w->head_bias},
                 num_actions};
  hipLaunchKernelGGL(cnn_grad_pack, dim3((unsigned)((CNN_G_PACK + 255) / 256)), dim3(256), 0, hs, pk, ws);
  if (int rc = be_launched(be_ctx_err(ctx))) return rc;
  const CnnGradSlot S = cnn_grad_slot(num_actions);
  const int64_t ntiles = (rows + GT - 1) / GT;
  const int grid = (int)(ntiles < 1 ? 1 : (ntiles < slots ? ntiles : slots));
  GParams p{};
  p.pack = ws; p.head_w = w->head_weight;
  p.images = images; p.quadrants = quadrants; p.actions = actions; p.coef = coef; p.valid = valid;
  p.probs = g->probs;
  p.slots = (uint8_t*)(ws + CNN_G_PACK);
  p.rows = rows; p.ntiles = ntiles; p.A = num_actions; p.S = S;
  hipLaunchKernelGGL(cnn_grad_kernel, dim3((unsigned)grid), dim3(G_THREADS), (size_t)CNN_GRAD_LDS_BYTES, hs, p);
  if (int rc = be_launched(be_ctx_err(ctx))) return rc;
  RParams r{};
  r.slots = p.slots; r.nslots = grid; r.A = num_actions; r.S = S; r.scale = scale;
  cnn_grad_pointers(g, r.g);
  r.losses = g->losses;
  hipLaunchKernelGGL(cnn_grad_reduce, dim3((unsigned)((S.outputs + 2 + 255) / 256)), dim3(256), 0, hs, r);
  return be_launched(be_ctx_err(ctx));
}

int be_observe_quadrant(be_ctx* ctx, const be_state* st, uint8_t* out, void* stream) {
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (!out) return be_ctx_fail(ctx, BE_E_INVALID, "be_observe_quadrant: out is NULL");
  const be_ctx_view cv = be_ctx_get(ctx);
  BE_ENTER_DEVICE(be_ctx_err(ctx), cv.device);
  hipLaunchKernelGGL(quadrant_kernel, dim3((unsigned)((cv.num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     st->agent, st->goal, out, cv.num_envs);
  return be_launched(be_ctx_err(ctx));
}

}  // extern "C"
