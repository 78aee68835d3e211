// mlp_policy.hip -- on-GPU select_action of the reference's REINFORCE / supervised agents
// (DESIGN §3.14): the block-count MLP on the 29-wide prep_state2 observation, straight from the
// env state, plus the Categorical draw -- one launch for every env.
//
// Reference:
//   examples/ball_env_reinforce.py:57-85   Policy (affine1 29->128, affine2, affine3 -> 9; relu on
//                                          every layer, the last included :70) and select_action
//   examples/test_model.py:57-85           the same network, evaluated
//   examples/train_supervise.py:11-26      Model: the same layers, no relu on the last
//   examples/ball_env_reinforce.py:130-172 prep_state2, the input (blocks_core.h)
//
//   be_mlp_load   one launch: the f32 state_dict arrays into the padded image the kernel stages
//   be_mlp_act    one launch: [prep_state2 ->] forward -> softmax -> draw, the arithmetic
//                 include/ballenv.h pins
//   be_mlp_rollout  `steps` steps of be_mlp_act + be_step: one launch of ballenv.hip's mlp_rollout_kernel and
//                 the observe kernel, or that loop where no fused instance applies
//   be_mlp_opt    two launches: optimizer.step() of both training loops (Adam, ball_env_reinforce.py:196;
//                 SGD, train_supervise.py:75) on the state_dict tensors in place, fused with be_mlp_load's
//                 pack of the new weights; then the one-wave state kernel it shares with
//                 be_a2c_adam (be_internal_optim_advance)
//
// The image's layout and the forward itself are mlp_core.h's, shared with the fused rollout.
// Every product runs on v_mfma_f32_16x16x4_f32 (an exact f32 fma chain) as D = W . x^T: the
// weights are the A operand (row = output unit), a tile of 16 envs the B operand (column = env),
// so lane (c = lane & 15, g = lane >> 4) ends a layer holding units 16 t + 4 g + r (r = 0..3) of
// env c in accumulator t.  Those registers ARE the next layer's B operand: a k step of an MFMA
// may take the inputs in any order as long as A and B agree, so step (t, r) of the next layer
// multiplies the weight columns 16 t + 4 g + r, which is how be_mlp_load lays the A fragments
// out.  No activation goes through LDS, and no product has a shape test: hidden sizes are padded
// to the instance's 128 and the actions to 16 with zero weights and biases (relu(0) = 0 adds
// nothing), the 29 inputs to 32.
//
// A persistent grid, one workgroup of 8 waves per CU; the image (89 KB in f32 at 128/128/9) is staged
// once per workgroup in LDS, fragment-major (one conflict-free 4-byte read per lane and MFMA), then
// wave w of workgroup b of G takes the 16-env tiles b + G w, + 8 G, ... with no block barrier (a batch
// of up to 16 G envs runs one wave per CU: the 4-wave build's time at 4 096 envs).  Per tile:
//   1  prep_state2 of the 16 envs: lane group g takes obstacles g, g + 4, ..., the four partial rows
//      are summed with permlane swaps (byte counters cannot carry); or the caller's rows
//   2  the layers, the bias in the accumulator's start
//   3  the 16 logits of each env through the wave's LDS slice to lanes 0..15: softmax, draw,
//      log_prob (policy_core.h's policy_finish, the tail of be_policy_act)
#include <hip/hip_runtime.h>

#include <math.h>
#include <new>
#include <stdint.h>
#include <stdlib.h>

#include "ballenv.h"
#include "blocks_core.h"
#include "host_logic.h"
#include "internal.h"
#include "mlp_core.h"
#include "optim_core.h"
#include "philox.h"
#include "policy_core.h"

namespace {

constexpr int MLP_THREADS = 64 * MLP_NW;
constexpr int MLP_TILE = 16;                 // envs per wave and tile
constexpr int MLP_CH = 5;                    // obstacles per lane and load chunk (4 groups: 20 per pass)

struct MPack {               // device f32 weights in torch state_dict layout; wl / bl: the last layer
  const float *w1, *b1, *w2, *b2, *wl, *bl;
  int H1, H2, A;
};

__global__ __launch_bounds__(256) void mlp_pack_kernel(MPack a, float* img, MlpLayout L) {
  const int HL = L.layers == 3 ? a.H2 : a.H1;
  for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < L.total; i += (int)gridDim.x * 256) {
    float v = 0.0f;
    if (i < L.b1) {
      const int lane = i & 63, t = i >> 6, ht = t % L.HT1, kk = t / L.HT1;
      const int m = 16 * ht + (lane & 15), k = 4 * kk + (lane >> 4);
      if (m < a.H1 && k < BLK_ROW) v = a.w1[m * BLK_ROW + k];
    } else if (i < L.f2) {
      const int m = i - L.b1;
      if (m < a.H1) v = a.b1[m];
    } else if (i < L.b2) {
      const int j = i - L.f2, lane = j & 63, t = j >> 6, mt = t % L.HT2, s = t / L.HT2;
      const int m = 16 * mt + (lane & 15), k = 16 * (s >> 2) + 4 * (lane >> 4) + (s & 3);
      if (m < a.H2 && k < a.H1) v = a.w2[m * a.H1 + k];
    } else if (i < L.f3) {
      const int m = i - L.b2;
      if (m < a.H2) v = a.b2[m];
    } else if (i < L.b3) {
      const int j = i - L.f3, lane = j & 63, s = j >> 6;
      const int m = lane & 15, k = 16 * (s >> 2) + 4 * (lane >> 4) + (s & 3);
      if (m < a.A && k < HL) v = a.wl[m * HL + k];
    } else if (i < L.hb) {
      const int m = i - L.b3;
      if (m < a.A) v = a.bl[m];
    } else {
      const int m = i - L.hb;
      v = (m < a.A || m == MLP_NO - 1) ? 0.0f : -INFINITY;
    }
    img[i] = v;
  }
}

// be_mlp_opt: the optimiser step on the four or six tensors and the pack above, inverted.  Thread i
// takes source element i of w1 | b1 | w2 | b2 | wl | bl laid end to end (w2 / b2: the second hidden
// layer, empty with 2 layers; wl / bl: the last layer), so a wave reads w, g, m, v and writes w, m, v
// as consecutive floats, and scatters its new weight to the one image index that mlp_pack_kernel fills
// from that element:
//   f1       (m, k) -> kk = k >> 2, ht = m >> 4, lane = (k & 3) << 4 | (m & 15)
//   f2 / f3  (m, k) -> s = (k >> 4) << 2 | (k & 3), l4 = (k >> 2) & 3, mt = m >> 4, lane = l4 << 4 | (m & 15)
// The map is a bijection onto the image's non-pad part: no element has two writers and no thread reads
// what another writes.  Pad entries are zero since be_mlp_create (every be_mlp_load rewrites them as
// zeros, and the shape never changes); the last 16 threads write hb, which completes an image that was
// never loaded.
struct MSix { float *w1, *b1, *w2, *b2, *wl, *bl; };

struct OParams {
  MSix w, g, m, v;           // params, grads (read only), exp_avg, exp_avg_sq (Adam only)
  const double* state;       // [t, beta1^t, beta2^t, lr] before the call
  double beta1, beta2, eps;
  float* img;
  MlpLayout L;
  int32_t H1, H2, A;
  int32_t e0, e1, e2, e3, e4, e5;      // the running ends of the six tensors in the element order
};

template <int KIND>
__global__ __launch_bounds__(256) void mlp_opt_kernel(OParams p) {
  const MlpLayout& L = p.L;
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= p.e5 + MLP_NO) return;
  if (i >= p.e5) {
    const int m = i - p.e5;
    p.img[L.hb + m] = (m < p.A || m == MLP_NO - 1) ? 0.0f : -INFINITY;
    return;
  }
  const int HL = L.layers == 3 ? p.H2 : p.H1;
  float *w, *m1p, *m2p;
  const float* g;
  int j, dst;
  if (i < p.e0) {
    j = i;
    const int m = j / BLK_ROW, k = j - m * BLK_ROW;
    dst = L.f1 + (((k >> 2) * L.HT1 + (m >> 4)) << 6) + (((k & 3) << 4) | (m & 15));
    w = p.w.w1; g = p.g.w1; m1p = p.m.w1; m2p = p.v.w1;
  } else if (i < p.e1) {
    j = i - p.e0;
    dst = L.b1 + j;
    w = p.w.b1; g = p.g.b1; m1p = p.m.b1; m2p = p.v.b1;
  } else if (i < p.e2) {
    j = i - p.e1;
    const int m = j / p.H1, k = j - m * p.H1, s = ((k >> 4) << 2) | (k & 3);
    dst = L.f2 + ((s * L.HT2 + (m >> 4)) << 6) + ((((k >> 2) & 3) << 4) | (m & 15));
    w = p.w.w2; g = p.g.w2; m1p = p.m.w2; m2p = p.v.w2;
  } else if (i < p.e3) {
    j = i - p.e2;
    dst = L.b2 + j;
    w = p.w.b2; g = p.g.b2; m1p = p.m.b2; m2p = p.v.b2;
  } else if (i < p.e4) {
    j = i - p.e3;
    const int m = j / HL, k = j - m * HL, s = ((k >> 4) << 2) | (k & 3);
    dst = L.f3 + (s << 6) + ((((k >> 2) & 3) << 4) | m);
    w = p.w.wl; g = p.g.wl; m1p = p.m.wl; m2p = p.v.wl;
  } else {
    j = i - p.e4;
    dst = L.b3 + j;
    w = p.w.bl; g = p.g.bl; m1p = p.m.bl; m2p = p.v.bl;
  }
  // the pinned arithmetic of include/ballenv.h (optim_core.h)
  if constexpr (KIND == BE_MLP_OPT_ADAM)
    p.img[dst] = adam_elem(adam_step(p.state, p.beta1, p.beta2, p.eps), g, m1p, m2p, w, j);
  else
    p.img[dst] = sgd_elem(p.state[3], g, w, j);
}

// the first pointer of a tensor set that is NULL or misaligned where the layer count needs it, or set
// where it does not (w3 / b3 with 2 layers), as "<set>-><field>", or nullptr
const char* mlp_bad_field(const be_mlp_tensors* t, int layers, const char* const (&names)[6]) {
  const float* const ptrs[6] = {t->w1, t->b1, t->w2, t->b2, t->w3, t->b3};
  for (int i = 0; i < 6; ++i) {
    if (i >= 4 && layers == 2) {
      if (ptrs[i]) return names[i];
    } else if (!ptrs[i] || ((uintptr_t)ptrs[i] & 3)) {
      return names[i];
    }
  }
  return nullptr;
}
#define BE_MLP_NAMES(set) {set "->w1", set "->b1", set "->w2", set "->b2", set "->w3", set "->b3"}
const char* const MN_PARAMS[6] = BE_MLP_NAMES("params");
const char* const MN_GRADS[6] = BE_MLP_NAMES("grads");
const char* const MN_AVG[6] = BE_MLP_NAMES("exp_avg");
const char* const MN_SQ[6] = BE_MLP_NAMES("exp_avg_sq");

// a tensor set in the kernel's order: with 2 layers the caller's w2 / b2 are the last layer
MSix mlp_six(const be_mlp_tensors* t, int layers) {
  if (!t) return MSix{};
  return layers == 3 ? MSix{t->w1, t->b1, t->w2, t->b2, t->w3, t->b3}
                     : MSix{t->w1, t->b1, nullptr, nullptr, t->w2, t->b2};
}

struct MParams {
  const float* img;
  const int32_t* agent; const int32_t* goal; const int32_t* static_obs; const int32_t* dyn_obs;
  const uint32_t* episode;   // (N) Philox key words (be_state.episode / ep_len)
  const int32_t* ep_len;
  const uint8_t* blocks_in;  // (N, 29) or NULL: prep_state2 of the state
  uint8_t* blocks_out;       // (N, 29) or NULL
  uint8_t* action;           // (N)
  float* log_prob;           // (N) or NULL
  float* probs;              // (N, A) or NULL
  unsigned long long seed;
  int32_t n, ns, nd, ntiles, A, gid0, final_relu;
};

template <int LAYERS, int HT1, int HT2>
__global__ __launch_bounds__(MLP_THREADS) void mlp_act_kernel(MParams p) {
  extern __shared__ uint4 mlp_lds[];
  constexpr MlpLayout L = mlp_layout(LAYERS, HT1, HT2);
  static_assert(L.total % 4 == 0, "the image is staged in 16-byte words");
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  stage_image<MLP_THREADS, 6>(mlp_lds, (const uint4*)p.img, L.total / 4, tid);
  __syncthreads();
  const float* W = (const float*)mlp_lds;
  float* Zs = (float*)mlp_lds + L.total + wave * MLP_SLICE;
  uint8_t* rows = (uint8_t*)(Zs + 16 * MLP_ZP);
  const bool from_state = p.blocks_in == nullptr;
  const int nobs = p.ns + p.nd;

  for (int tile = (int)blockIdx.x + (int)gridDim.x * wave; tile < p.ntiles; tile += (int)gridDim.x * MLP_NW) {
    const int e0 = tile * MLP_TILE, env = e0 + l15;
    const int ic = env < p.n ? env : p.n - 1;     // a clamped env computes and writes nothing
    // the draw's Philox key words (lane c < 16 finishes env e0 + c)
    const uint32_t episode = lane < 16 ? p.episode[ic] : 0u;
    const int32_t len = lane < 16 ? p.ep_len[ic] : 0;

    // 1: the B operand of layer 1: x[k] = input 4 k + l4 of env l15
    float x[MLP_KS1];
    if (from_state || p.blocks_out) {
      const int32_t a = p.agent[ic], gl = p.goal[ic];
      const int ax = px(a), ay = py(a);
      uint32_t w8[BLK_WORDS];
      blocks_init(w8, a, gl);
#pragma unroll
      for (int q = 0; q < BLK_WORDS; ++q) w8[q] = l4 == 0 ? w8[q] : 0u;
      // every load of a chunk is issued before the first is used (clamped to a real obstacle, the
      // extra slots masked), as in blocks_kernel
      for (int k0 = 0; k0 < nobs; k0 += 4 * MLP_CH) {
        int32_t o[MLP_CH];
#pragma unroll
        for (int j = 0; j < MLP_CH; ++j) {
          const int k = min(k0 + 4 * j + l4, nobs - 1);
          const int32_t* src = k < p.ns ? p.static_obs + (int64_t)k * p.n : p.dyn_obs + (int64_t)(k - p.ns) * p.n;
          o[j] = src[ic];
        }
#pragma unroll
        for (int j = 0; j < MLP_CH; ++j) blocks_add(w8, ax, ay, o[j], k0 + 4 * j + l4 < nobs);
      }
#pragma unroll
      for (int q = 0; q < BLK_WORDS; ++q) w8[q] = sum_groups_u32(w8[q]);
      if (p.blocks_out) {      // the tile's rows are one contiguous run of the output
        // lane group g writes bytes 8 g .. 8 g + 7 of its env's row: words 2 g and 2 g + 1, picked with
        // selects (an indexed w8 would live in scratch memory); group 3 ends at byte 28
        const uint32_t lo = l4 == 0 ? w8[0] : (l4 == 1 ? w8[2] : (l4 == 2 ? w8[4] : w8[6]));
        const uint32_t hi = l4 == 0 ? w8[1] : (l4 == 1 ? w8[3] : (l4 == 2 ? w8[5] : w8[7]));
        uint8_t* rb = rows + l15 * BLK_ROW + 8 * l4;
#pragma unroll
        for (int j = 0; j < 4; ++j) rb[j] = (uint8_t)(lo >> (8 * j));
        rb[4] = (uint8_t)hi;
        if (l4 < 3) {
#pragma unroll
          for (int j = 1; j < 4; ++j) rb[4 + j] = (uint8_t)(hi >> (8 * j));
        }
        wave_sync();
        const int nbytes = min(MLP_TILE, p.n - e0) * BLK_ROW;
        uint8_t* dst = p.blocks_out + (int64_t)e0 * BLK_ROW;
        for (int b = lane; b < nbytes; b += 64) dst[b] = rows[b];
        wave_sync();
      }
#pragma unroll
      for (int k = 0; k < MLP_KS1; ++k) x[k] = (float)((w8[k] >> (8 * l4)) & 0xFFu);
    }
    if (!from_state) {
      const uint8_t* row = p.blocks_in + (int64_t)ic * BLK_ROW;
#pragma unroll
      for (int k = 0; k < MLP_KS1; ++k) {
        const int col = 4 * k + l4;
        const uint8_t v = row[min(col, BLK_ROW - 1)];
        x[k] = col < BLK_ROW ? (float)v : 0.0f;
      }
    }

    // 2: the layers (mlp_core.h)
    // (layer 1 keeps its inline text here: moved into a helper in mlp_core.h, the kernel's schedule changes)
    f32x4 h1[HT1];
#pragma unroll
    for (int t = 0; t < HT1; ++t) h1[t] = *(const f32x4*)(W + L.b1 + 16 * t + 4 * l4);
#pragma unroll
    for (int k = 0; k < MLP_KS1; ++k)
#pragma unroll
      for (int t = 0; t < HT1; ++t) h1[t] = BE_MFMA(W[L.f1 + (k * HT1 + t) * 64 + lane], x[k], h1[t]);
#pragma unroll
    for (int t = 0; t < HT1; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) h1[t][r] = fmaxf(h1[t][r], 0.0f);
    f32x4 z;
    if constexpr (LAYERS == 3) {
      f32x4 h2[HT2];
      mlp_hidden<HT1, HT2>(W + L.f2, W + L.b2, h1, lane, h2);
      z = mlp_last<HT2>(W + L.f3, W + L.b3, h2, lane);
    } else {
      z = mlp_last<HT1>(W + L.f3, W + L.b3, h1, lane);
    }

    // 3: logits 4 l4 + r of env l15 -> the slice; lane c < 16 finishes env e0 + c
#pragma unroll
    for (int r = 0; r < 4; ++r) Zs[l15 * MLP_ZP + 4 * l4 + r] = p.final_relu ? fmaxf(z[r], 0.0f) : z[r];
    wave_sync();
    if (lane < 16 && env < p.n) {
      float lp, val;
      const int act = policy_finish<MLP_NO>(Zs + lane * MLP_ZP, W + L.hb, p.A, (uint32_t)(p.gid0 + env), episode,
                                            (uint32_t)len, p.seed, p.probs ? p.probs + (int64_t)env * p.A : nullptr,
                                            lp, val);
      p.action[env] = (uint8_t)act;
      if (p.log_prob) p.log_prob[env] = lp;
    }
    wave_sync();
  }
}

}  // namespace

struct be_mlp {
  be_ctx* ctx;
  be_ctx_view cv;
  int layers, H1, H2, A, final_relu, cus;
  MlpLayout L;
  float* img;
  bool loaded;
  int roll_waves;            // BALLENV_MLP_ROLLOUT_WAVES at be_mlp_create (-1: host_logic.h's rule)
};

extern "C" {

int be_mlp_create(be_ctx* ctx, int32_t layers, int32_t hidden1, int32_t hidden2, int32_t num_actions,
                  int32_t final_relu, be_mlp** out) {
  if (!ctx || !out) return be_ctx_fail(ctx, BE_E_INVALID, "bad arguments to be_mlp_create");
  *out = nullptr;
  if (layers != 2 && layers != 3) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_create: layers must be 2 or 3");
  if (hidden1 < 1 || hidden1 > MLP_MAXH) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_create: hidden1 must be in [1, 128]");
  if (layers == 3 && (hidden2 < 1 || hidden2 > MLP_MAXH))
    return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_create: hidden2 must be in [1, 128]");
  if (layers == 2 && hidden2 != 0) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_create: hidden2 must be 0 with 2 layers");
  if (num_actions < 1 || num_actions > POL_MAXA)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_create: num_actions must be in [1, 15]");
  be_mlp* m = new (std::nothrow) be_mlp();
  if (!m) return be_ctx_fail(ctx, BE_E_NOMEM, "out of host memory");
  m->ctx = ctx; m->cv = be_ctx_get(ctx);
  m->layers = layers; m->H1 = hidden1; m->H2 = hidden2; m->A = num_actions; m->final_relu = final_relu ? 1 : 0;
  m->L = mlp_layout(layers, MLP_HT, MLP_HT);
  m->roll_waves = behost::mlp_rollout_waves_env(getenv("BALLENV_MLP_ROLLOUT_WAVES"));   // (A/B runs and tests)
  const DeviceGuard dg(m->cv.device);   // the caller's current device is restored on return
  hipError_t e = dg.err;
  if (e == hipSuccess) e = hipDeviceGetAttribute(&m->cus, hipDeviceAttributeMultiprocessorCount, m->cv.device);
  if (e == hipSuccess) e = hipMalloc(&m->img, (size_t)m->L.total * 4);
  if (e == hipSuccess) e = hipMemset(m->img, 0, (size_t)m->L.total * 4);
  if (e != hipSuccess || m->cus < 1) {
    if (m->img) (void)hipFree(m->img);
    delete m;
    if (e == hipSuccess) return be_ctx_fail(ctx, BE_E_HIP, "be_mlp_create: cannot query the device's compute units");
    return be_hip_fail(be_ctx_err(ctx), e);
  }
  *out = m;
  return BE_OK;
}

int be_mlp_destroy(be_mlp* m) {
  if (!m) return BE_OK;
  const DeviceGuard dg(m->cv.device);
  if (m->img) (void)hipFree(m->img);
  delete m;
  return BE_OK;
}

int be_mlp_load(be_mlp* m, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                const float* b3, void* stream) {
  if (!m) return be_ctx_fail(nullptr, BE_E_INVALID, "be_mlp_load: mlp is NULL");
  be_ctx* ctx = m->ctx;
  if (!w1 || !b1 || !w2 || !b2) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_load: a weight pointer is NULL");
  if (m->layers == 3 && (!w3 || !b3)) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_load: 3 layers need w3 and b3");
  if (m->layers == 2 && (w3 || b3)) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_load: w3 and b3 must be NULL with 2 layers");
  BE_ENTER_DEVICE(be_ctx_err(ctx), m->cv.device);
  const MPack a = m->layers == 3 ? MPack{w1, b1, w2, b2, w3, b3, m->H1, m->H2, m->A}
                                 : MPack{w1, b1, nullptr, nullptr, w2, b2, m->H1, 0, m->A};
  hipLaunchKernelGGL(mlp_pack_kernel, dim3((unsigned)((m->L.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a,
                     m->img, m->L);
  if (int rc = be_launched(be_ctx_err(ctx))) return rc;
  m->loaded = true;
  return BE_OK;
}

int be_mlp_opt(be_mlp* m, int32_t kind, const be_mlp_tensors* params, const be_mlp_tensors* grads,
               const be_mlp_tensors* exp_avg, const be_mlp_tensors* exp_avg_sq, double* state, double beta1,
               double beta2, double eps, const double* losses, double* loss_log, int32_t log_rows, void* stream) {
  if (!m) return be_ctx_fail(nullptr, BE_E_INVALID, "be_mlp_opt: mlp is NULL");
  be_ctx* ctx = m->ctx;
  char* err = be_ctx_err(ctx);
  const bool adam = kind == BE_MLP_OPT_ADAM;
  if (!adam && kind != BE_MLP_OPT_SGD)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_opt: kind must be BE_MLP_OPT_ADAM or BE_MLP_OPT_SGD");
  if (!params) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_opt: params is NULL");
  if (!grads) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_opt: grads is NULL");
  if (adam && !exp_avg) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_opt: exp_avg is NULL (BE_MLP_OPT_ADAM needs it)");
  if (adam && !exp_avg_sq)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_opt: exp_avg_sq is NULL (BE_MLP_OPT_ADAM needs it)");
  if (!adam && (exp_avg || exp_avg_sq))
    return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_opt: exp_avg and exp_avg_sq must be NULL with BE_MLP_OPT_SGD");
  const struct { const be_mlp_tensors* t; const char* const (&names)[6]; } sets[4] = {
      {params, MN_PARAMS}, {grads, MN_GRADS}, {exp_avg, MN_AVG}, {exp_avg_sq, MN_SQ}};
  for (const auto& s : sets) {
    if (!s.t) continue;
    if (const char* name = mlp_bad_field(s.t, m->layers, s.names))
      return be_fail(err, BE_E_INVALID,
                     "be_mlp_opt: %s is NULL or not 4-byte aligned (w3 and b3: set with 3 layers, NULL with 2)", name);
  }
  if (const char* msg = behost::optim_args_error(state, adam, beta1, beta2, eps, losses, loss_log, log_rows))
    return be_fail(err, BE_E_INVALID, "be_mlp_opt: %s", msg);
  BE_ENTER_DEVICE(err, m->cv.device);
  OParams p{};
  p.w = mlp_six(params, m->layers); p.g = mlp_six(grads, m->layers);
  p.m = mlp_six(exp_avg, m->layers); p.v = mlp_six(exp_avg_sq, m->layers);
  p.state = state; p.beta1 = beta1; p.beta2 = beta2; p.eps = eps;
  p.img = m->img; p.L = m->L; p.H1 = m->H1; p.H2 = m->H2; p.A = m->A;
  const int HL = m->layers == 3 ? m->H2 : m->H1;
  p.e0 = m->H1 * BLK_ROW;
  p.e1 = p.e0 + m->H1;
  p.e2 = p.e1 + (m->layers == 3 ? m->H2 * m->H1 : 0);
  p.e3 = p.e2 + (m->layers == 3 ? m->H2 : 0);
  p.e4 = p.e3 + m->A * HL;
  p.e5 = p.e4 + m->A;
  const dim3 grid((unsigned)((p.e5 + MLP_NO + 255) / 256)), block(256);
  hipStream_t hs = (hipStream_t)stream;
  if (adam) hipLaunchKernelGGL((mlp_opt_kernel<BE_MLP_OPT_ADAM>), grid, block, 0, hs, p);
  else hipLaunchKernelGGL((mlp_opt_kernel<BE_MLP_OPT_SGD>), grid, block, 0, hs, p);
  if (int rc = be_launched(err)) return rc;
  if (int rc = be_internal_optim_advance(err, state, adam, beta1, beta2, losses, loss_log, 2, log_rows, stream)) return rc;
  m->loaded = true;
  return BE_OK;
}

int be_mlp_act(be_mlp* m, const be_state* st, const uint8_t* blocks_in, uint8_t* blocks_out, const be_act_out* out,
               uint64_t seed, void* stream) {
  if (!m) return be_ctx_fail(nullptr, BE_E_INVALID, "be_mlp_act: mlp is NULL");
  be_ctx* ctx = m->ctx;
  if (!m->loaded) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_act before be_mlp_load");
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (!out || !out->action) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_act needs out->action");
  if (out->value) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_act: out->value must be NULL (this network has no value head)");
  BE_ENTER_DEVICE(be_ctx_err(ctx), m->cv.device);
  MParams p{};
  p.img = m->img;
  p.agent = st->agent; p.goal = st->goal; p.static_obs = st->static_obs; p.dyn_obs = st->dyn_obs;
  p.episode = st->episode; p.ep_len = st->ep_len;
  p.blocks_in = blocks_in; p.blocks_out = blocks_out;
  p.action = out->action; p.log_prob = out->log_prob; p.probs = out->probs;
  p.seed = (unsigned long long)seed;
  p.n = m->cv.num_envs; p.ns = m->cv.num_static; p.nd = m->cv.num_dynamic;
  p.ntiles = (p.n + MLP_TILE - 1) / MLP_TILE;
  p.A = m->A; p.gid0 = (int32_t)(uint32_t)m->cv.env_offset; p.final_relu = m->final_relu;
  // tiles go to the workgroups first, then to their waves: a small batch runs one wave on every CU
  const dim3 grid((unsigned)(p.ntiles < m->cus ? p.ntiles : m->cus)), block(MLP_THREADS);
  if (m->layers == 3)
    hipLaunchKernelGGL((mlp_act_kernel<3, MLP_HT, MLP_HT>), grid, block, (size_t)m->L.lds, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL((mlp_act_kernel<2, MLP_HT, 0>), grid, block, (size_t)m->L.lds, (hipStream_t)stream, p);
  return be_launched(be_ctx_err(ctx));
}

// ball_env_reinforce.py's episode loop (:309-336: prep_state2, select_action, env.step, the reward appended)
// for every env, `steps` steps per call.
int be_mlp_rollout(be_mlp* m, const be_state* st, uint8_t* obs_last, uint8_t* blocks_out, int32_t steps,
                   const be_out* out, const be_act_out* act, uint64_t seed, void* stream) {
  if (!m) return be_ctx_fail(nullptr, BE_E_INVALID, "be_mlp_rollout: mlp is NULL");
  be_ctx* ctx = m->ctx;
  if (!m->loaded) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_rollout before be_mlp_load");
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (const char* msg = behost::mlp_rollout_args_error(obs_last, steps, out, act)) return be_ctx_fail(ctx, BE_E_INVALID, msg);
  if (steps == 0) return BE_OK;
  BE_ENTER_DEVICE(be_ctx_err(ctx), m->cv.device);
  const int waves = behost::mlp_rollout_waves(m->cv.num_envs, m->cus, m->layers, m->roll_waves);
  if (waves > 0) {
    const be_mlp_rollout_args r{m->img, m->layers, waves, m->A, m->final_relu, (unsigned long long)seed,
                                obs_last, blocks_out, steps, out, act};
    const int rc = be_internal_mlp_rollout(ctx, st, &r, stream);
    if (rc != 0) return rc < 0 ? rc : BE_OK;
  }
  // no fused kernel for this shape: be_mlp_act + be_step per step (the same trajectory)
  const int64_t N = m->cv.num_envs, F = 4 + (int64_t)m->cv.window * m->cv.window;
  for (int32_t s = 0; s < steps; ++s) {
    const be_act_out ao{act->action + s * N, act->log_prob ? act->log_prob + s * N : nullptr, nullptr, nullptr};
    if (int e = be_mlp_act(m, st, nullptr, blocks_out ? blocks_out + s * N * BLK_ROW : nullptr, &ao, seed, stream)) return e;
    be_out o = behost::be_out_at(*out, s, N, F);
    o.obs = obs_last;
    if (int e = be_step(ctx, st, ao.action, nullptr, nullptr, &o, stream)) return e;
  }
  return BE_OK;
}

const char* be_mlp_rollout_kernel(const be_mlp* m) {
  if (!m) return nullptr;
  const int waves = behost::mlp_rollout_waves(m->cv.num_envs, m->cus, m->layers, m->roll_waves);
  return waves > 0 ? be_internal_mlp_rollout_name(m->ctx, m->layers, waves) : nullptr;
}

int64_t be_mlp_bytes(const be_mlp* m) { return m ? (int64_t)m->L.total * 4 : 0; }

}  // extern "C"
