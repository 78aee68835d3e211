// a2c_grad.hip -- the second half of the batched A2C finish_episode (examples/ball_cnn_ac3.py:233-244,
// SURVEY §8(f) rank 1): the policy and value losses of Policy(W) over recorded rows and their
// gradients with respect to the six weight arrays, straight from the u8 observations:
//
//   be_a2c_grad   forward (fc1 -> relu -> action / value head), log-softmax, smooth-L1, backward,
//                 gradient sums over all rows (the computation include/ballenv.h pins)
//
// Two kernels, no float atomics, so the result is reproducible bit for bit:
//
//   a2c_grad_kernel   one workgroup of 4 waves per CU, each looping over tiles of 64 rows (tile
//                     b, b + G, ... for workgroup b of G).  A tile's observations are staged in LDS
//                     as the bytes they are; every matrix product runs on v_mfma_f32_16x16x4_f32
//                     (an exact f32 fma chain):
//                       1  pre = b1 + W1 x, h = relu(pre) -> LDS   the accumulator starts at the bias
//                       2  z, v = [Wa; Wv] h + [ba; bv] -> LDS     wave w: rows 16w .. 16w+15
//                       3  log-softmax, losses, dz, dv -> LDS      one lane per row
//                       4  g[Wa; Wv] += dzv^T h, g[ba; bv] += dzv^T 1, dh = dzv [Wa; Wv],
//                          dpre = h > 0 ? dh : 0 over h in LDS
//                       5  gW1 += dpre^T x, gb1 += dpre^T 1
//                     The observation operands are read from the staged bytes with a clamped address and
//                     no test on the column: past F step 1 multiplies them by zero weights and step 5's
//                     columns are never written (a test here became a branch around every LDS read).
//                     Wave w owns the hidden tiles w, w+4, w+8, w+12 in steps 1, 4 and 5: its slice of
//                     W1 (as MFMA B fragments) and its gW1 / g[Wa; Wv] accumulators stay in registers
//                     for the whole kernel, and between steps 3 and 5 it reads and writes only its own
//                     columns of h, so those steps need no barrier.  The next tile's observations are
//                     fetched into registers before step 1 and written to LDS after step 5.
//                     At the end every workgroup writes its sums to its slot of the workspace.
//   a2c_grad_reduce   one thread per gradient element: the slots added in workgroup order in f64,
//                     rounded once to f32; three threads do the same for the f64 losses.
//
// Rows past `rows` in the last tile are staged as zeros and are inactive, like rows with valid = 0
// or an action >= num_actions: their dz and dv are exact zeros, so they add +0 to every sum.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <initializer_list>

#include "ballenv.h"
#include "internal.h"

namespace {

constexpr int THREADS = 256, NW = 4;
constexpr int R = 64;                       // rows per tile
constexpr int MAXF = 128, MAXH = 256, MAXA = 15;   // be_policy_create's bounds
// The kernel's template arguments are the padded shape (registers and trip counts are sized by them;
// the hot loops have no shape tests: what lies past H or F is zeros in the operands):
//   MT   hidden tiles of 16 per wave                 (H <= 64 MT)
//   FTM  feature tiles of 16 of gW1 (F <= 16 FTM), KT1 k steps of 4 of fc1 (F <= 4 KT1)
//   W1R  this wave's slice of W1 stays in registers (else step 1 reads it from global memory: L2)
// Policy(10) (H = 208: 13 tiles, so wave 0 has 4 and sets the pace either way) and Policy(5) have
// exact instances; any other shape runs the smallest instance that covers it.
#ifndef BE_A2C_GRAD_SKIP
#define BE_A2C_GRAD_SKIP 0   // -DBE_A2C_GRAD_SKIP=n: timing builds that leave step n out (wrong results;
#endif                       // what each step costs: profiles/a2c_grad_ab.json)
constexpr int SKIP = BE_A2C_GRAD_SKIP;
constexpr int ZP = 17;                      // row stride of the z / dz tiles
constexpr int XD = 8;                       // dwords of a tile's observations per thread
constexpr int MAX_SLOTS = 1024;
static_assert(MAXH <= 64 * 4 && MAXF <= 4 * 32 && MAXF <= 16 * 8, "the widest kernel instance covers the bounds");
static_assert(R * MAXF <= 4 * THREADS * XD, "a tile's observations must fit XD dwords per thread");
static_assert(R == 16 * NW, "step 2 gives each wave one 16-row tile");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Layout {            // of one workgroup's slot in the workspace (offsets in floats) and of LDS (bytes)
  int32_t F, H, A, HT, HP;
  int32_t o_b1, o_wa, o_ba, o_wv, o_bv, P;      // gW1 at 0; P gradient elements
  int32_t loss_off, slot_bytes;                 // the three f64 losses follow the gradients
  int32_t l_h, l_wh, l_z, l_dz, l_red, lds;
};

struct Instance { int MT, FTM, KT1; };
constexpr Instance INST_W5{2, 2, 8}, INST_W10{4, 7, 26}, INST_ANY{4, 8, 32};

Instance pick_instance(int F, int H) {
  for (const Instance& in : {INST_W5, INST_W10})
    if (H <= 16 * NW * in.MT && F <= 4 * in.KT1 && F <= 16 * in.FTM) return in;
  return INST_ANY;
}

Layout make_layout(int F, int H, int A) {
  Layout L{};
  L.F = F; L.H = H; L.A = A;
  L.HT = (H + 15) / 16;
  L.HP = 16 * NW * pick_instance(F, H).MT + 16; // row stride of h: every wave's MT tiles, 16 (mod 32) floats
  L.o_b1 = H * F; L.o_wa = L.o_b1 + H; L.o_ba = L.o_wa + A * H; L.o_wv = L.o_ba + A; L.o_bv = L.o_wv + H;
  L.P = L.o_bv + 1;
  L.loss_off = (L.P * 4 + 7) / 8 * 8;
  L.slot_bytes = L.loss_off + 3 * 8;
  const int xb = (R * F + 15) / 16 * 16;
  L.l_h = xb;
  L.l_wh = L.l_h + R * L.HP * 4;
  L.l_z = L.l_wh + 16 * L.HP * 4;
  L.l_dz = L.l_z + (R * ZP * 4 + 15) / 16 * 16;
  L.l_red = L.l_dz + (R * ZP * 4 + 15) / 16 * 16;
  L.lds = L.l_red + R * 3 * 8;
  return L;
}

struct GParams {
  const uint8_t* __restrict__ obs; const uint8_t* __restrict__ actions;
  const float* __restrict__ rn; const uint8_t* __restrict__ valid;
  const float* __restrict__ w1; const float* __restrict__ b1; const float* __restrict__ wa;
  const float* __restrict__ ba; const float* __restrict__ wv; const float* __restrict__ bv;
  uint8_t* ws;
  int64_t rows, ntiles;
  int32_t obs_aligned;       // obs is 4-byte aligned: whole dwords of a tile are loaded as such
  Layout L;
};

struct RParams {
  const uint8_t* ws; int32_t nslots; Layout L;
  float *w1, *b1, *wa, *ba, *wv, *bv; double* losses;
};

// element (row, f) of the staged tile as an MFMA operand; for f >= F some other byte of the tile
__device__ __forceinline__ float xval(const uint8_t* Xb, int row, int f, int F) {
  return (float)Xb[min(row * F + f, R * F - 1)];
}

// tile `tile`'s observations (R * F bytes, zeros past `rows`) into registers
__device__ __forceinline__ void fetch_tile(const GParams& p, int64_t tile, int tid, uint32_t (&d)[XD]) {
  const int F = p.L.F;
  const int64_t row0 = tile * R, left = p.rows - row0;
  const int nbytes = left >= R ? R * F : (left > 0 ? (int)left * F : 0);
  const uint8_t* src = p.obs + (nbytes > 0 ? row0 * F : 0);
#pragma unroll
  for (int i = 0; i < XD; ++i) {
    const int o = 4 * (tid + THREADS * i);
    uint32_t v = 0;
    if (p.obs_aligned && o + 4 <= nbytes) {
      v = *(const uint32_t*)(src + o);
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (o + b < nbytes) v |= (uint32_t)src[o + b] << (8 * b);
    }
    d[i] = v;
  }
}

__device__ __forceinline__ void store_tile(uint8_t* Xb, int F, int tid, const uint32_t (&d)[XD]) {
#pragma unroll
  for (int i = 0; i < XD; ++i) {
    const int o = 4 * (tid + THREADS * i);
    if (o < R * F) *(uint32_t*)(Xb + o) = d[i];          // R * F is a multiple of 4
  }
}

#define BE_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

template <int MT, int FTM, int KT1, bool W1R>
__global__ __launch_bounds__(THREADS) void a2c_grad_kernel(GParams p) {
  extern __shared__ __align__(16) uint8_t smem[];
  const Layout& L = p.L;
  const int F = L.F, H = L.H, A = L.A, HT = L.HT, HP = L.HP;
  uint8_t* Xb = smem;
  float* Hs = (float*)(smem + L.l_h);
  float* Wh = (float*)(smem + L.l_wh);
  float* Zs = (float*)(smem + L.l_z);
  float* DZs = (float*)(smem + L.l_dz);
  double* red = (double*)(smem + L.l_red);
  const int tid = (int)threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int l15 = lane & 15, l4 = lane >> 4;

  // [Wa; Wv; 0] as a (16, HP) LDS image, zero past H
  for (int i = tid; i < 16 * HP; i += THREADS) {
    const int j = i / HP, h = i - j * HP;
    float v = 0.0f;
    if (h < H) v = j < A ? p.wa[j * H + h] : (j == A ? p.wv[h] : 0.0f);
    Wh[i] = v;
  }
  // this wave's slice of [W1 | b1] as the B fragments of step 1: B[k = f][col = h]
  auto w1val = [&](int m, int kk) __attribute__((always_inline)) {
    const int ht = wave + NW * m, h = 16 * ht + l15, f = 4 * kk + l4;
    float v = 0.0f;
    if (h < H && f < F) v = p.w1[h * F + f];
    return v;
  };
  float w1f[W1R ? MT : 1][W1R ? KT1 : 1];
  if (W1R) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int kk = 0; kk < KT1; ++kk) w1f[m][kk] = w1val(m, kk);
  }
  float b1f[MT];            // b1 of this lane's column of each hidden tile
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int h = 16 * (wave + NW * m) + l15;
    b1f[m] = h < H ? p.b1[h] : 0.0f;
  }
  const float bz = l15 < A ? p.ba[l15] : (l15 == A ? p.bv[0] : 0.0f);

  uint32_t xd[XD];
  int64_t tile = blockIdx.x;
  fetch_tile(p, tile, tid, xd);
  store_tile(Xb, F, tid, xd);
  __syncthreads();

  // [Wa; Wv] as the B fragments of dh in step 4: B[k = j][col = h]
  float whf[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int ht = wave + NW * m;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) whf[m][kk] = Wh[(4 * kk + l4) * HP + 16 * ht + l15];
  }

  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 g1[MT][FTM], g1b[MT], gh[MT], gbh = zero4;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    gh[m] = zero4;
    g1b[m] = zero4;
#pragma unroll
    for (int ft = 0; ft < FTM; ++ft) g1[m][ft] = zero4;
  }
  double pl = 0.0, vl = 0.0, cnt = 0.0;

  for (; tile < p.ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    fetch_tile(p, tile + gridDim.x, tid, xd);
    int act = 255, vld = 0;
    float rnv = 0.0f;
    {
      const int64_t gr = row0 + 16 * wave + lane;
      if (lane < 16 && gr < p.rows) {
        act = p.actions[gr];
        rnv = p.rn[gr];
        vld = p.valid[gr];
      }
    }

    // 1: h = relu(W1 x + b1), this wave's hidden tiles of all 64 rows
    constexpr int U1 = W1R ? KT1 : 2;      // W1 from memory: a short body, or its loads fill the registers
    for (int rt = 0; rt < R / 16; ++rt) {
      f32x4 acc[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m] = f32x4{b1f[m], b1f[m], b1f[m], b1f[m]};
#pragma unroll U1
      for (int kk = 0; kk < (SKIP == 1 ? 0 : KT1); ++kk) {
        const float a = xval(Xb, 16 * rt + l15, 4 * kk + l4, F);      // A[i = row][k = f]
#pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[m] = BE_MFMA(a, W1R ? w1f[W1R ? m : 0][W1R ? kk : 0] : w1val(m, kk), acc[m]);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int ht = wave + NW * m;
#pragma unroll
        for (int r = 0; r < 4; ++r) Hs[(16 * rt + 4 * l4 + r) * HP + 16 * ht + l15] = fmaxf(acc[m][r], 0.0f);
      }
    }
    __syncthreads();

    // 2: z (columns 0 .. A-1) and v (column A) of rows 16 wave .. 16 wave + 15; four fma chains (k mod 4)
    {
      f32x4 z0 = {bz, bz, bz, bz}, z1 = zero4, z2 = zero4, z3 = zero4;
      const float* ha = Hs + (16 * wave + l15) * HP + l4;     // A[i = row][k = h]
      const float* wb = Wh + l15 * HP + l4;                   // B[k = h][col = j]
      for (int kk = 0; kk < (SKIP == 2 ? 0 : 4 * HT); kk += 4) {
        z0 = BE_MFMA(ha[4 * kk], wb[4 * kk], z0);
        z1 = BE_MFMA(ha[4 * kk + 4], wb[4 * kk + 4], z1);
        z2 = BE_MFMA(ha[4 * kk + 8], wb[4 * kk + 8], z2);
        z3 = BE_MFMA(ha[4 * kk + 12], wb[4 * kk + 12], z3);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) Zs[(16 * wave + 4 * l4 + r) * ZP + l15] = (z0[r] + z1[r]) + (z2[r] + z3[r]);
    }
    __syncthreads();

    // 3: one lane per row
    if (lane < 16 && SKIP != 3) {
      const int row = 16 * wave + lane;
      const float* z = Zs + row * ZP;
      const bool active = vld != 0 && act < A;
      float mx = z[0];
      for (int j = 1; j < A; ++j) mx = fmaxf(mx, z[j]);
      float s = 0.0f;
      for (int j = 0; j < A; ++j) s += expf(z[j] - mx);
      const float lse = mx + logf(s);
      float adv = 0.0f, dv = 0.0f;
      if (active) {
        const float v = z[A], logp = z[act] - lse;
        adv = rnv - v;
        pl += (double)(-(logp * adv));
        const float d = v - rnv, ad = fabsf(d);
        vl += (double)(ad < 1.0f ? 0.5f * d * d : ad - 0.5f);
        dv = ad < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f);
        cnt += 1.0;
      }
      for (int j = 0; j < 16; ++j) {
        float g = 0.0f;
        if (active) {
          if (j < A) g = adv * (expf(z[j] - lse) - (j == act ? 1.0f : 0.0f));
          else if (j == A) g = dv;
        }
        DZs[row * ZP + j] = g;
      }
    }
    __syncthreads();

    // 4: g[Wa; Wv] += dzv^T h, g[ba; bv] += dzv^T 1 (wave 0), then dpre over this wave's columns of h
#pragma unroll 2
    for (int kk = 0; kk < (SKIP == 4 ? 0 : R / 4); ++kk) {
      const float a = DZs[(4 * kk + l4) * ZP + l15];          // A[i = j][k = row]
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int ht = wave + NW * m;
        gh[m] = BE_MFMA(a, Hs[(4 * kk + l4) * HP + 16 * ht + l15], gh[m]);   // B[k = row][col = h]
      }
      gbh = BE_MFMA(a, 1.0f, gbh);                             // every wave; wave 0's is written
    }
    for (int rt = 0; rt < (SKIP == 4 ? 0 : R / 16); ++rt) {
      float af[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) af[kk] = DZs[(16 * rt + l15) * ZP + 4 * kk + l4];    // A[i = row][k = j]
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int ht = wave + NW * m;
        f32x4 d = zero4;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) d = BE_MFMA(af[kk], whf[m][kk], d);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* hp = Hs + (16 * rt + 4 * l4 + r) * HP + 16 * ht + l15;
          *hp = *hp > 0.0f ? d[r] : 0.0f;
        }
      }
    }

    // 5: gW1 += dpre^T x
    for (int kk = 0; kk < (SKIP == 5 ? 0 : R / 4); ++kk) {
      const int row = 4 * kk + l4;
      float bf[FTM];
#pragma unroll
      for (int ft = 0; ft < FTM; ++ft) bf[ft] = xval(Xb, row, 16 * ft + l15, F);   // B[k = row][col = f]
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const float a = Hs[row * HP + 16 * (wave + NW * m) + l15];       // A[i = h][k = row]
#pragma unroll
        for (int ft = 0; ft < FTM; ++ft) g1[m][ft] = BE_MFMA(a, bf[ft], g1[m][ft]);
        g1b[m] = BE_MFMA(a, 1.0f, g1b[m]);
      }
    }
    __syncthreads();
    store_tile(Xb, F, tid, xd);
    __syncthreads();
  }

  // this workgroup's sums into its slot: every element of the slot is written
  float* slot = (float*)(p.ws + (int64_t)blockIdx.x * L.slot_bytes);
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int ht = wave + NW * m;
    {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = 16 * ht + 4 * l4 + r;               // gW1 tile: C[i = h][col = f]
        if (h < H) {
#pragma unroll
          for (int ft = 0; ft < FTM; ++ft) {
            const int f = 16 * ft + l15;
            if (f < F) slot[h * F + f] = g1[m][ft][r];
          }
          if (l15 == 0) slot[L.o_b1 + h] = g1b[m][r];
        }
        const int j = 4 * l4 + r, hh = 16 * ht + l15;     // g[Wa; Wv] tile: C[i = j][col = h]
        if (hh < H) {
          if (j < A) slot[L.o_wa + j * H + hh] = gh[m][r];
          else if (j == A) slot[L.o_wv + hh] = gh[m][r];
        }
      }
    }
  }
  if (wave == 0 && l15 == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 4 * l4 + r;
      if (j < A) slot[L.o_ba + j] = gbh[r];
      else if (j == A) slot[L.o_bv] = gbh[r];
    }
  }
  if (lane < 16) {
    double* q = red + 3 * (16 * wave + lane);
    q[0] = pl; q[1] = vl; q[2] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < R; ++i) { s0 += red[3 * i]; s1 += red[3 * i + 1]; s2 += red[3 * i + 2]; }
    double* out = (double*)(p.ws + (int64_t)blockIdx.x * L.slot_bytes + L.loss_off);
    out[0] = s0; out[1] = s1; out[2] = s2;
  }
}

__global__ __launch_bounds__(256) void a2c_grad_reduce(RParams p) {
  const Layout& L = p.L;
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i < L.P) {
    double s = 0.0;
    for (int sl = 0; sl < p.nslots; ++sl) s += (double)((const float*)(p.ws + (int64_t)sl * L.slot_bytes))[i];
    const float v = (float)s;
    if (i < L.o_b1) p.w1[i] = v;
    else if (i < L.o_wa) p.b1[i - L.o_b1] = v;
    else if (i < L.o_ba) p.wa[i - L.o_wa] = v;
    else if (i < L.o_wv) p.ba[i - L.o_ba] = v;
    else if (i < L.o_bv) p.wv[i - L.o_wv] = v;
    else p.bv[0] = v;
  } else if (i < L.P + 3) {
    const int k = i - L.P;
    double s = 0.0;
    for (int sl = 0; sl < p.nslots; ++sl) s += ((const double*)(p.ws + (int64_t)sl * L.slot_bytes + L.loss_off))[k];
    p.losses[k] = s;
  }
}

// workgroups of the persistent grid = slots of the workspace: one per CU of ctx's device
int grad_slots(int device) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) return 0;
  return cus < MAX_SLOTS ? cus : MAX_SLOTS;
}

const char* check_shape(int F, int hidden, int num_actions) {
  if (F > MAXF) return "be_a2c_grad: the observation 4+W*W must be <= 128 (W <= 11)";
  if (hidden < 1 || hidden > MAXH) return "be_a2c_grad: hidden must be in [1, 256]";
  if (num_actions < 1 || num_actions > MAXA) return "be_a2c_grad: num_actions must be in [1, 15]";
  return nullptr;
}

}  // namespace

extern "C" {

int64_t be_a2c_grad_workspace_bytes(be_ctx* ctx, int32_t hidden, int32_t num_actions) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  const be_ctx_view cv = be_ctx_get(ctx);
  const int F = 4 + cv.window * cv.window;
  if (const char* msg = check_shape(F, hidden, num_actions)) return be_ctx_fail(ctx, BE_E_INVALID, msg);
  const int slots = grad_slots(cv.device);
  if (slots < 1) return be_ctx_fail(ctx, BE_E_HIP, "be_a2c_grad: cannot query the device's compute units");
  return (int64_t)slots * make_layout(F, hidden, num_actions).slot_bytes;
}

int be_a2c_grad(be_ctx* ctx, const uint8_t* obs, const uint8_t* actions, const float* returns_norm,
                const uint8_t* valid, int64_t rows, const be_a2c_weights* w, void* workspace,
                int64_t workspace_bytes, const be_a2c_grads* g, void* stream) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  if (!obs) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: obs is NULL");
  if (!actions) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: actions is NULL");
  if (!returns_norm) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: returns_norm is NULL");
  if (!valid) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: valid is NULL");
  if (rows < 0) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: rows must be >= 0");
  if (!w) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: weights is NULL");
  if (!g) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: grads is NULL");
  if (!w->fc1_weight || !w->fc1_bias || !w->action_head_weight || !w->action_head_bias || !w->value_head_weight ||
      !w->value_head_bias)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: a weight pointer is NULL");
  if (!g->fc1_weight || !g->fc1_bias || !g->action_head_weight || !g->action_head_bias || !g->value_head_weight ||
      !g->value_head_bias || !g->losses)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: a gradient pointer or losses is NULL");
  const be_ctx_view cv = be_ctx_get(ctx);
  const int F = 4 + cv.window * cv.window;
  if (const char* msg = check_shape(F, w->hidden, w->num_actions)) return be_ctx_fail(ctx, BE_E_INVALID, msg);
  const int slots = grad_slots(cv.device);
  if (slots < 1) return be_ctx_fail(ctx, BE_E_HIP, "be_a2c_grad: cannot query the device's compute units");
  const Layout L = make_layout(F, w->hidden, w->num_actions);
  if (!workspace || ((uintptr_t)workspace & 7))
    return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: workspace is NULL or not 8-byte aligned");
  if (workspace_bytes < (int64_t)slots * L.slot_bytes)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: workspace is smaller than be_a2c_grad_workspace_bytes");
  if (L.lds > 160 * 1024) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_grad: the tile exceeds the LDS budget");
  BE_ENTER_DEVICE(be_ctx_err(ctx), cv.device);
  const int64_t ntiles = (rows + R - 1) / R;
  const int grid = (int)(ntiles < 1 ? 1 : (ntiles < slots ? ntiles : slots));
  GParams p{obs, actions, returns_norm, valid, w->fc1_weight, w->fc1_bias, w->action_head_weight,
            w->action_head_bias, w->value_head_weight, w->value_head_bias, (uint8_t*)workspace, rows, ntiles,
            ((uintptr_t)obs & 3) == 0 ? 1 : 0, L};
  hipStream_t hs = (hipStream_t)stream;
  const dim3 gd((unsigned)grid), bd(THREADS);
  const Instance in = pick_instance(F, w->hidden);
  if (in.MT == INST_W5.MT)
    hipLaunchKernelGGL((a2c_grad_kernel<INST_W5.MT, INST_W5.FTM, INST_W5.KT1, true>), gd, bd, (size_t)L.lds, hs, p);
  else if (in.KT1 == INST_W10.KT1)
    hipLaunchKernelGGL((a2c_grad_kernel<INST_W10.MT, INST_W10.FTM, INST_W10.KT1, true>), gd, bd, (size_t)L.lds, hs, p);
  else
    hipLaunchKernelGGL((a2c_grad_kernel<INST_ANY.MT, INST_ANY.FTM, INST_ANY.KT1, false>), gd, bd, (size_t)L.lds, hs, p);
  if (int rc = be_launched(be_ctx_err(ctx))) return rc;
  RParams r{(const uint8_t*)workspace, grid, L, g->fc1_weight, g->fc1_bias, g->action_head_weight,
            g->action_head_bias, g->value_head_weight, g->value_head_bias, g->losses};
  hipLaunchKernelGGL(a2c_grad_reduce, dim3((unsigned)((L.P + 3 + 255) / 256)), dim3(256), 0, hs, r);
  return be_launched(be_ctx_err(ctx));
}

}  // extern "C"
