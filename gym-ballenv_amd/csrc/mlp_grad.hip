// mlp_grad.hip -- the learning half of the block-count MLP: the loss of the reference's
// two training loops for this network over recorded rows and its gradients with respect to the
// four or six weight arrays, straight from the u8 block counts:
//
//   examples/ball_env_reinforce.py:88-108   finish_episode: sum of -Categorical(probs).log_prob(a) * R^
//   examples/train_supervise.py:66-101      mean CrossEntropyLoss on the logits
//
//   be_mlp_grad   forward (affine1 -> relu [-> affine2 -> relu] -> last layer [-> relu]), softmax, the row
//                 loss of the chosen kind, backward, gradient sums over all rows (the computation
//                 include/ballenv.h pins)
//
// Two kernels, no float atomics, so the result is reproducible bit for bit (a2c_grad.hip's scheme):
//
//   mlp_grad_kernel   one workgroup of 4 waves per CU, each looping over tiles of 64 rows (tile b,
//                     b + G, ... for workgroup b of G).  A tile's rows are staged in LDS as the bytes they
//                     are; every matrix product runs on v_mfma_f32_16x16x4_f32 (an exact f32 fma chain).
//                     Hidden sizes are padded to 128, the inputs to 32 and the actions to 16 with zero
//                     weights, so no MFMA loop has a shape test.  Wave w owns the hidden tiles w and
//                     w + 4 of both hidden layers: its slices of W1 and W2 (as the B fragments of the
//                     forward and of dh1 = dpre2 W2) and its gradient accumulators stay in registers
//                     for the whole kernel; the activations live in LDS, row-major with the column
//                     XOR-swizzled by the row (hidx), so that both the reads with the row on the MFMA's
//                     i axis (forward, dh) and those with the row on its k axis (the outer products)
//                     are free of bank conflicts:
//                       1  h1 = relu(b1 + W1 x) -> LDS                     own columns, all 64 rows
//                       2  h2 = relu(b2 + W2 h1) -> LDS                    (3 layers) own columns
//                       3  zp = b_last + W_last h -> LDS                   wave w: rows 16w .. 16w+15
//                       4  softmax, row loss, dzp -> LDS                   one lane per row
//                       5  gW_last += dzp^T h, gb_last += dzp^T 1, dh = dzp W_last,
//                          dpre = h > 0 ? dh : 0 over h in LDS             own columns
//                       6  gW2 += dpre2^T h1, gb2 += dpre2^T 1             (3 layers) own rows of gW2
//                       7  dh1 = dpre2 W2, dpre1 = h1 > 0 ? dh1 : 0 over h1 in LDS   (3 layers)
//                       8  gW1 += dpre1^T x, gb1 += dpre1^T 1
//                     The next tile's rows are fetched into registers before step 1 and written to LDS
//                     after step 8.  At the end every workgroup writes its sums to its slot of the workspace.
//   mlp_grad_reduce   one thread per gradient element: the slots added in workgroup order in f64, times
//                     scale, rounded once to f32; two threads do the same for the f64 losses.
//
// Rows past `rows` in the last tile are staged as zeros and are inactive, like rows with valid = 0
// or an action >= num_actions: their dzp are exact zeros, so they add +0 to every sum.
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "ballenv.h"
#include "host_logic.h"
#include "internal.h"

namespace {

using behost::MlpGradSlot;

constexpr int THREADS = 256, NW = 4;
constexpr int R = 64;                       // rows per tile
constexpr int F = 29;                       // prep_state2's row
constexpr int MT = 2;                       // hidden tiles of 16 per wave: hidden sizes are padded to 16 NW MT = 128
constexpr int HT = NW * MT;                 // hidden tiles
constexpr int KT1 = 8, FTM = 2;             // k steps of 4 of affine1 (29 -> 32), feature tiles of 16 of gW1
constexpr int KTH = 4 * HT;                 // k steps of 4 over a hidden layer
constexpr int HP = 16 * HT + 16;            // row stride of h1 / h2 / the W_last image: 16 (mod 32) floats
constexpr int ZP = 17;                      // row stride of the zp / dzp tiles
constexpr int XD = 2;                       // dwords of a tile's rows per thread
constexpr int MAX_SLOTS = 1024;
static_assert(R * F <= 4 * THREADS * XD && (R * F) % 16 == 0, "a tile's rows fit XD dwords per thread");
static_assert(R == 16 * NW, "step 3 gives each wave one 16-row tile");
static_assert(F <= 4 * KT1 && F <= 16 * FTM, "the padded input covers the row");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// LDS (bytes); h2 is there with 3 layers only
constexpr int L_X = 0, L_H1 = R * F, L_HBYTES = R * HP * 4, L_ZBYTES = R * ZP * 4;
__host__ __device__ constexpr int lds_wl(int layers) { return L_H1 + (layers == 3 ? 2 : 1) * L_HBYTES; }
__host__ __device__ constexpr int lds_z(int layers) { return lds_wl(layers) + 16 * HP * 4; }
__host__ __device__ constexpr int lds_dz(int layers) { return lds_z(layers) + L_ZBYTES; }
__host__ __device__ constexpr int lds_red(int layers) { return lds_dz(layers) + L_ZBYTES; }
__host__ __device__ constexpr int lds_bytes(int layers) { return lds_red(layers) + R * 2 * 8; }
static_assert(L_H1 % 16 == 0 && L_ZBYTES % 16 == 0 && lds_bytes(3) <= 160 * 1024, "aligned, and within a CU's LDS");

struct GParams {
  const uint8_t* __restrict__ blocks; const uint8_t* __restrict__ actions;
  const float* __restrict__ coef; const uint8_t* __restrict__ valid;          // coef, valid: may be NULL
  const float* __restrict__ w1; const float* __restrict__ b1; const float* __restrict__ w2;
  const float* __restrict__ b2; const float* __restrict__ wl; const float* __restrict__ bl;   // wl, bl: the last layer
  uint8_t* ws;
  int64_t rows, ntiles;
  int32_t aligned;           // blocks is 4-byte aligned: whole dwords of a tile are loaded as such
  int32_t H1, H2, A, final_relu, loss;
  MlpGradSlot S;
};

struct RParams {
  const uint8_t* ws; int32_t nslots; MlpGradSlot S; double scale;
  float *w1, *b1, *w2, *b2, *w3, *b3; double* losses;
};

// element (row, col) of an activation tile (or of the W_last image): the column's bits 1..3 are
// XORed with the row's, so 16 rows at one column and 16 columns at one row both spread over the banks
__device__ __forceinline__ int hidx(int row, int col) { return row * HP + (col ^ (((row >> 1) & 7) << 1)); }
// hidx for the three ways the MFMA fragments walk a tile, as a few lane-dependent bases plus offsets that
// are compile-time constants after unrolling (hidx itself would cost one address register per access):
//   i1(rb, ks)     = hidx(rb + l15, 4 ks + l4)            row on the i axis, k step ks; rb a multiple of 16
//   i2(kk, c)      = hidx(4 kk + l4, c + l15)             row on the k axis, k step kk; c a multiple of 16
//   ic(rb, r, c)   = hidx(rb + 4 l4 + r, c + l15)         an accumulator's element r; rb, c multiples of 16
struct Swz {
  int p1[4], p2[4], pc[2];
  __device__ __forceinline__ Swz(int l15, int l4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      p1[q] = l15 * HP + ((4 * q + l4) ^ (((l15 >> 1) & 7) << 1));
      p2[q] = l4 * HP + (l15 ^ (l4 & 2) ^ (4 * q));
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) pc[b] = 4 * l4 * HP + (l15 ^ (4 * l4) ^ (2 * b));
  }
  __device__ __forceinline__ int i1(int rb, int ks) const { return rb * HP + 16 * (ks >> 2) + p1[ks & 3]; }
  __device__ __forceinline__ int i2(int kk, int c) const { return 4 * kk * HP + c + p2[kk & 3]; }
  __device__ __forceinline__ int ic(int rb, int r, int c) const { return (rb + r) * HP + c + pc[r >> 1]; }
};

// element (row, f) of the staged tile as an MFMA operand; for f >= F some other byte of the tile
__device__ __forceinline__ float xval(const uint8_t* Xb, int row, int f) {
  return (float)Xb[min(row * F + f, R * F - 1)];
}

// tile `tile`'s rows (R * F bytes, zeros past `rows`) into registers
__device__ __forceinline__ void fetch_tile(const GParams& p, int64_t tile, int tid, uint32_t (&d)[XD]) {
  const int64_t row0 = tile * R, left = p.rows - row0;
  const int nbytes = left >= R ? R * F : (left > 0 ? (int)left * F : 0);
  const uint8_t* src = p.blocks + (nbytes > 0 ? row0 * F : 0);
#pragma unroll
  for (int i = 0; i < XD; ++i) {
    const int o = 4 * (tid + THREADS * i);
    uint32_t v = 0;
    if (p.aligned && o + 4 <= nbytes) {
      v = *(const uint32_t*)(src + o);
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (o + b < nbytes) v |= (uint32_t)src[o + b] << (8 * b);
    }
    d[i] = v;
  }
}

__device__ __forceinline__ void store_tile(uint8_t* Xb, int tid, const uint32_t (&d)[XD]) {
#pragma unroll
  for (int i = 0; i < XD; ++i) {
    const int o = 4 * (tid + THREADS * i);
    if (o < R * F) *(uint32_t*)(Xb + o) = d[i];          // R * F is a multiple of 4
  }
}

#define BE_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

template <int LAYERS>
__global__ __launch_bounds__(THREADS) void mlp_grad_kernel(GParams p) {
  extern __shared__ __align__(16) uint8_t smem[];
  constexpr bool L3 = LAYERS == 3;
  const MlpGradSlot& S = p.S;
  const int H1 = p.H1, H2 = p.H2, A = p.A, HL = L3 ? H2 : H1;
  uint8_t* Xb = smem + L_X;
  float* H1s = (float*)(smem + L_H1);
  float* H2s = (float*)(smem + L_H1 + L_HBYTES);        // 3 layers
  float* Hl = L3 ? H2s : H1s;                            // the last layer's input
  float* Wl = (float*)(smem + lds_wl(LAYERS));
  float* Zs = (float*)(smem + lds_z(LAYERS));
  float* DZs = (float*)(smem + lds_dz(LAYERS));
  double* red = (double*)(smem + lds_red(LAYERS));
  const int tid = (int)threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int l15 = lane & 15, l4 = lane >> 4;
  const Swz sw(l15, l4);

  // W_last as a (16, HP) LDS image, zero past A and HL
  for (int i = tid; i < 16 * HT * 16; i += THREADS) {
    const int j = i / (16 * HT), h = i - j * (16 * HT);
    Wl[hidx(j, h)] = (j < A && h < HL) ? p.wl[j * HL + h] : 0.0f;
  }
  // this wave's slice of W1 as the B fragments of step 1: B[k = f][col = h]
  float w1f[MT][KT1], b1f[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int h = 16 * (wave + NW * m) + l15;
    b1f[m] = h < H1 ? p.b1[h] : 0.0f;
#pragma unroll
    for (int kk = 0; kk < KT1; ++kk) {
      const int f = 4 * kk + l4;
      w1f[m][kk] = (h < H1 && f < F) ? p.w1[h * F + f] : 0.0f;
    }
  }
  // 3 layers: this wave's slices of W2 as the B fragments of step 2, B[k = h1][col = h2], and of
  // step 7, B[k = h2][col = h1]
  float w2f[L3 ? MT : 1][L3 ? KTH : 1], w2b[L3 ? MT : 1][L3 ? KTH : 1], b2f[MT];
  if constexpr (L3) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int c = 16 * (wave + NW * m) + l15;
      b2f[m] = c < H2 ? p.b2[c] : 0.0f;
#pragma unroll
      for (int kk = 0; kk < KTH; ++kk) {
        const int k = 4 * kk + l4;
        w2f[m][kk] = (c < H2 && k < H1) ? p.w2[c * H1 + k] : 0.0f;
        w2b[m][kk] = (k < H2 && c < H1) ? p.w2[k * H1 + c] : 0.0f;
      }
    }
  }
  const float bz = l15 < A ? p.bl[l15] : 0.0f;

  uint32_t xd[XD];
  int64_t tile = blockIdx.x;
  fetch_tile(p, tile, tid, xd);
  store_tile(Xb, tid, xd);
  __syncthreads();

  // W_last as the B fragments of dh in step 5: B[k = j][col = h]
  float whf[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) whf[m][kk] = Wl[sw.i2(kk, 16 * (wave + NW * m))];

  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 g1[MT][FTM], g1b[MT], gl[MT], gbl = zero4;
  f32x4 g2[L3 ? MT : 1][L3 ? HT : 1], g2b[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    gl[m] = zero4;
    g1b[m] = zero4;
    g2b[m] = zero4;
#pragma unroll
    for (int ft = 0; ft < FTM; ++ft) g1[m][ft] = zero4;
    if constexpr (L3) {
#pragma unroll
      for (int t = 0; t < HT; ++t) g2[m][t] = zero4;
    }
  }
  double ls = 0.0, cnt = 0.0;

  for (; tile < p.ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    fetch_tile(p, tile + gridDim.x, tid, xd);
    int act = 255, vld = 0;
    float cf = 0.0f;
    {
      const int64_t gr = row0 + 16 * wave + lane;
      if (lane < 16 && gr < p.rows) {
        act = p.actions[gr];
        cf = p.coef ? p.coef[gr] : 1.0f;
        vld = p.valid ? p.valid[gr] : 1;
      }
    }

    // 1: h1 = relu(W1 x + b1), this wave's hidden tiles of all 64 rows
    for (int rt = 0; rt < R / 16; ++rt) {
      f32x4 acc[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m] = f32x4{b1f[m], b1f[m], b1f[m], b1f[m]};
#pragma unroll
      for (int kk = 0; kk < KT1; ++kk) {
        const float a = xval(Xb, 16 * rt + l15, 4 * kk + l4);          // A[i = row][k = f]
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = BE_MFMA(a, w1f[m][kk], acc[m]);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          H1s[sw.ic(16 * rt, r, 16 * (wave + NW * m))] = fmaxf(acc[m][r], 0.0f);
    }
    __syncthreads();

    // 2: h2 = relu(W2 h1 + b2), this wave's hidden tiles of all 64 rows
    if constexpr (L3) {
      for (int rt = 0; rt < R / 16; ++rt) {
        f32x4 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = f32x4{b2f[m], b2f[m], b2f[m], b2f[m]};
#pragma unroll
        for (int kk = 0; kk < KTH; ++kk) {
          const float a = H1s[sw.i1(16 * rt, kk)];                     // A[i = row][k = h1]
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m] = BE_MFMA(a, w2f[m][kk], acc[m]);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            H2s[sw.ic(16 * rt, r, 16 * (wave + NW * m))] = fmaxf(acc[m][r], 0.0f);
      }
      __syncthreads();
    }

    // 3: zp of rows 16 wave .. 16 wave + 15; four fma chains (k mod 4)
    {
      f32x4 z0 = {bz, bz, bz, bz}, z1 = zero4, z2 = zero4, z3 = zero4;
      const float* ha = Hl + 16 * wave * HP;                           // A[i = row][k = h]
#pragma unroll 2
      for (int t = 0; t < HT; ++t) {                                   // B[k = h][col = j]
        z0 = BE_MFMA(ha[16 * t + sw.p1[0]], Wl[16 * t + sw.p1[0]], z0);
        z1 = BE_MFMA(ha[16 * t + sw.p1[1]], Wl[16 * t + sw.p1[1]], z1);
        z2 = BE_MFMA(ha[16 * t + sw.p1[2]], Wl[16 * t + sw.p1[2]], z2);
        z3 = BE_MFMA(ha[16 * t + sw.p1[3]], Wl[16 * t + sw.p1[3]], z3);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) Zs[(16 * wave + 4 * l4 + r) * ZP + l15] = (z0[r] + z1[r]) + (z2[r] + z3[r]);
    }
    __syncthreads();

    // 4: one lane per row
    if (lane < 16) {
      const int row = 16 * wave + lane;
      const float* zp = Zs + row * ZP;
      const bool active = vld != 0 && act < A;
      const bool fr = p.final_relu != 0;
      float mx = fr ? fmaxf(zp[0], 0.0f) : zp[0];
      for (int j = 1; j < A; ++j) mx = fmaxf(mx, fr ? fmaxf(zp[j], 0.0f) : zp[j]);
      float s = 0.0f;
      for (int j = 0; j < A; ++j) s += expf((fr ? fmaxf(zp[j], 0.0f) : zp[j]) - mx);
      bool pass = active;             // the row's dz is not cut off by Categorical's clamp
      if (active) {
        const float za = fr ? fmaxf(zp[act], 0.0f) : zp[act];
        float loss;
        if (p.loss == BE_MLP_LOSS_REINFORCE) {
          const float pa = expf(za - mx) / s, lo = FLT_EPSILON, hi = 1.0f - FLT_EPSILON;
          loss = -(cf * logf(fminf(fmaxf(pa, lo), hi)));
          pass = pa >= lo && pa <= hi;
        } else {
          loss = -(cf * ((za - mx) - logf(s)));
        }
        ls += (double)loss;
        cnt += 1.0;
      }
      for (int j = 0; j < 16; ++j) {
        float g = 0.0f;
        if (pass && j < A) {
          const float z = fr ? fmaxf(zp[j], 0.0f) : zp[j];
          g = cf * (expf(z - mx) / s - (j == act ? 1.0f : 0.0f));
          if (fr && zp[j] <= 0.0f) g = 0.0f;
        }
        DZs[row * ZP + j] = g;
      }
    }
    __syncthreads();

    // 5: gW_last += dzp^T h, gb_last += dzp^T 1 (wave 0), then dpre over this wave's columns of h
    for (int k4 = 0; k4 < R / 16; ++k4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float a = DZs[(16 * k4 + 4 * q + l4) * ZP + l15];          // A[i = j][k = row]
#pragma unroll
        for (int m = 0; m < MT; ++m)
          gl[m] = BE_MFMA(a, Hl[16 * k4 * HP + sw.i2(q, 16 * (wave + NW * m))], gl[m]);   // B[k = row][col = h]
        gbl = BE_MFMA(a, 1.0f, gbl);                           // every wave; wave 0's is written
      }
    }
    for (int rt = 0; rt < R / 16; ++rt) {
      float af[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) af[kk] = DZs[(16 * rt + l15) * ZP + 4 * kk + l4];    // A[i = row][k = j]
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        f32x4 d = zero4;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) d = BE_MFMA(af[kk], whf[m][kk], d);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* hp = Hl + sw.ic(16 * rt, r, 16 * (wave + NW * m));
          *hp = *hp > 0.0f ? d[r] : 0.0f;
        }
      }
    }

    if constexpr (L3) {
      __syncthreads();               // dpre2 is complete in every column
      // 6: gW2 += dpre2^T h1 (this wave's rows of gW2, every column), gb2 += dpre2^T 1
      for (int k4 = 0; k4 < R / 16; ++k4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float* h1r = H1s + 16 * k4 * HP;
          const float* h2r = H2s + 16 * k4 * HP;
          float bf[HT];
#pragma unroll
          for (int t = 0; t < HT; ++t) bf[t] = h1r[sw.i2(q, 16 * t)];                 // B[k = row][col = h1]
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const float a = h2r[sw.i2(q, 16 * (wave + NW * m))];                      // A[i = h2][k = row]
#pragma unroll
            for (int t = 0; t < HT; ++t) g2[m][t] = BE_MFMA(a, bf[t], g2[m][t]);
            g2b[m] = BE_MFMA(a, 1.0f, g2b[m]);
          }
        }
      }
      __syncthreads();               // every wave has read h1 in every column
      // 7: dh1 = dpre2 W2, dpre1 over this wave's columns of h1
      for (int rt = 0; rt < R / 16; ++rt) {
        f32x4 d[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) d[m] = zero4;
#pragma unroll
        for (int kk = 0; kk < KTH; ++kk) {
          const float a = H2s[sw.i1(16 * rt, kk)];                     // A[i = row][k = h2]
#pragma unroll
          for (int m = 0; m < MT; ++m) d[m] = BE_MFMA(a, w2b[m][kk], d[m]);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* hp = H1s + sw.ic(16 * rt, r, 16 * (wave + NW * m));
            *hp = *hp > 0.0f ? d[m][r] : 0.0f;
          }
      }
    }

    // 8: gW1 += dpre1^T x, gb1 += dpre1^T 1
    for (int k4 = 0; k4 < R / 16; ++k4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * k4 + 4 * q + l4;
        float bf[FTM];
#pragma unroll
        for (int ft = 0; ft < FTM; ++ft) bf[ft] = xval(Xb, row, 16 * ft + l15);       // B[k = row][col = f]
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const float a = H1s[16 * k4 * HP + sw.i2(q, 16 * (wave + NW * m))];         // A[i = h1][k = row]
#pragma unroll
          for (int ft = 0; ft < FTM; ++ft) g1[m][ft] = BE_MFMA(a, bf[ft], g1[m][ft]);
          g1b[m] = BE_MFMA(a, 1.0f, g1b[m]);
        }
      }
    }
    __syncthreads();
    store_tile(Xb, tid, xd);
    __syncthreads();
  }

  // this workgroup's sums into its slot: every element of the slot is written
  float* slot = (float*)(p.ws + (int64_t)blockIdx.x * S.slot_bytes);
  const int o_wl = L3 ? S.o_w3 : S.o_w2, o_bl = L3 ? S.o_b3 : S.o_b2;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int ht = wave + NW * m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = 16 * ht + 4 * l4 + r;               // gW1 / gW2 tiles: C[i = h][col]
      if (h < H1) {
#pragma unroll
        for (int ft = 0; ft < FTM; ++ft) {
          const int f = 16 * ft + l15;
          if (f < F) slot[h * F + f] = g1[m][ft][r];
        }
        if (l15 == 0) slot[S.o_b1 + h] = g1b[m][r];
      }
      if constexpr (L3) {
        if (h < H2) {
#pragma unroll
          for (int t = 0; t < HT; ++t) {
            const int c = 16 * t + l15;
            if (c < H1) slot[S.o_w2 + h * H1 + c] = g2[m][t][r];
          }
          if (l15 == 0) slot[S.o_b2 + h] = g2b[m][r];
        }
      }
      const int j = 4 * l4 + r, hh = 16 * ht + l15;     // gW_last tile: C[i = j][col = h]
      if (hh < HL && j < A) slot[o_wl + j * HL + hh] = gl[m][r];
    }
  }
  if (wave == 0 && l15 == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 4 * l4 + r;
      if (j < A) slot[o_bl + j] = gbl[r];
    }
  }
  if (lane < 16) {
    double* q = red + 2 * (16 * wave + lane);
    q[0] = ls; q[1] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    double s0 = 0.0, s1 = 0.0;
    for (int i = 0; i < R; ++i) { s0 += red[2 * i]; s1 += red[2 * i + 1]; }
    double* out = (double*)(p.ws + (int64_t)blockIdx.x * S.slot_bytes + S.loss_off);
    out[0] = s0; out[1] = s1;
  }
}

__global__ __launch_bounds__(256) void mlp_grad_reduce(RParams p) {
  const MlpGradSlot& S = p.S;
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i < S.P) {
    double s = 0.0;
    for (int sl = 0; sl < p.nslots; ++sl) s += (double)((const float*)(p.ws + (int64_t)sl * S.slot_bytes))[i];
    const float v = (float)(s * p.scale);
    if (i < S.o_b1) p.w1[i] = v;
    else if (i < S.o_w2) p.b1[i - S.o_b1] = v;
    else if (i < S.o_b2) p.w2[i - S.o_w2] = v;
    else if (i < S.o_w3) p.b2[i - S.o_b2] = v;
    else if (i < S.o_b3) p.w3[i - S.o_w3] = v;
    else p.b3[i - S.o_b3] = v;
  } else if (i < S.P + 2) {
    const int k = i - S.P;
    double s = 0.0;
    for (int sl = 0; sl < p.nslots; ++sl) s += ((const double*)(p.ws + (int64_t)sl * S.slot_bytes + S.loss_off))[k];
    p.losses[k] = k == 0 ? s * p.scale : s;
  }
}

// workgroups of the persistent grid = slots of the workspace: one per CU of ctx's device
int grad_slots(int device) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) return 0;
  return cus < MAX_SLOTS ? cus : MAX_SLOTS;
}

}  // namespace

extern "C" {

int64_t be_mlp_grad_workspace_bytes(be_ctx* ctx, int32_t layers, int32_t hidden1, int32_t hidden2,
                                    int32_t num_actions) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  if (const char* msg = behost::mlp_grad_shape_error(layers, hidden1, hidden2, num_actions))
    return be_ctx_fail(ctx, BE_E_INVALID, msg);
  const int slots = grad_slots(be_ctx_get(ctx).device);
  if (slots < 1) return be_ctx_fail(ctx, BE_E_HIP, "be_mlp_grad: cannot query the device's compute units");
  return (int64_t)slots * behost::mlp_grad_slot(layers, hidden1, hidden2, num_actions).slot_bytes;
}

int be_mlp_grad(be_ctx* ctx, const uint8_t* blocks, const uint8_t* actions, const float* coef, const uint8_t* valid,
                int64_t rows, int32_t loss, double scale, const be_mlp_weights* w, void* workspace,
                int64_t workspace_bytes, const be_mlp_grads* g, void* stream) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  if (!blocks) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_grad: blocks is NULL");
  if (!actions) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_grad: actions is NULL");
  if (rows < 0) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_grad: rows must be >= 0");
  if (loss != BE_MLP_LOSS_REINFORCE && loss != BE_MLP_LOSS_XENT)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_grad: loss must be BE_MLP_LOSS_REINFORCE or BE_MLP_LOSS_XENT");
  if (!w) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_grad: weights is NULL");
  if (!g) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_grad: grads is NULL");
  if (const char* msg = behost::mlp_grad_shape_error(w->layers, w->hidden1, w->hidden2, w->num_actions))
    return be_ctx_fail(ctx, BE_E_INVALID, msg);
  if (!w->w1 || !w->b1 || !w->w2 || !w->b2) return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_grad: a weight pointer is NULL");
  if (!g->w1 || !g->b1 || !g->w2 || !g->b2 || !g->losses)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_grad: a gradient pointer or losses is NULL");
  if (const char* msg = behost::mlp_grad_last_layer_error(w->layers, w->w3, w->b3)) return be_ctx_fail(ctx, BE_E_INVALID, msg);
  if (const char* msg = behost::mlp_grad_last_layer_error(w->layers, g->w3, g->b3)) return be_ctx_fail(ctx, BE_E_INVALID, msg);
  const be_ctx_view cv = be_ctx_get(ctx);
  const int slots = grad_slots(cv.device);
  if (slots < 1) return be_ctx_fail(ctx, BE_E_HIP, "be_mlp_grad: cannot query the device's compute units");
  const bool l3 = w->layers == 3;
  const MlpGradSlot S = behost::mlp_grad_slot(w->layers, w->hidden1, w->hidden2, w->num_actions);
  if (!workspace || ((uintptr_t)workspace & 7))
    return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_grad: workspace is NULL or not 8-byte aligned");
  if (workspace_bytes < (int64_t)slots * S.slot_bytes)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_mlp_grad: workspace is smaller than be_mlp_grad_workspace_bytes");
  BE_ENTER_DEVICE(be_ctx_err(ctx), cv.device);
  const int64_t ntiles = (rows + R - 1) / R;
  const int grid = (int)(ntiles < 1 ? 1 : (ntiles < slots ? ntiles : slots));
  GParams p{blocks, actions, coef, valid, w->w1, w->b1, l3 ? w->w2 : nullptr, l3 ? w->b2 : nullptr,
            l3 ? w->w3 : w->w2, l3 ? w->b3 : w->b2, (uint8_t*)workspace, rows, ntiles,
            ((uintptr_t)blocks & 3) == 0 ? 1 : 0, w->hidden1, l3 ? w->hidden2 : 0, w->num_actions,
            w->final_relu ? 1 : 0, loss, S};
  hipStream_t hs = (hipStream_t)stream;
  const dim3 gd((unsigned)grid), bd(THREADS);
  if (l3) hipLaunchKernelGGL(mlp_grad_kernel<3>, gd, bd, (size_t)lds_bytes(3), hs, p);
  else hipLaunchKernelGGL(mlp_grad_kernel<2>, gd, bd, (size_t)lds_bytes(2), hs, p);
  if (int rc = be_launched(be_ctx_err(ctx))) return rc;
  RParams r{(const uint8_t*)workspace, grid, S, scale, g->w1, g->b1, g->w2, g->b2, g->w3, g->b3, g->losses};
  hipLaunchKernelGGL(mlp_grad_reduce, dim3((unsigned)((S.P + 2 + 255) / 256)), dim3(256), 0, hs, r);
  return be_launched(be_ctx_err(ctx));
}

}  // extern "C"
