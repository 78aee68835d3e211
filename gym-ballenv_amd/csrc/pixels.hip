// pixels.hip -- the pixel agent's observation (sibling observation formats, with features.hip):
//
//   be_observe_pixels   extract_patch of examples/ball_cnn_reinforce.py:120-163: the frame of
//                       BallEnv.render (gym_ballenv/envs/ballenv_env.py:357-386) padded with white,
//                       the 100 x 100 patch centred on the agent, PIL's bicubic resize to 40 x 40
//                       and ToTensor's / 255 -- for every env, from the SoA state on the device.
//
// One wave per env at a time (a wave strides over the envs; eight waves a workgroup), every stage
// wave-local under wave barriers; the only workgroup barrier stands behind the tables all eight
// waves share.  The patch has four colours, so it never exists as pixels:
//   1. masks   lane = patch row.  Each channel of a row is 100 bits (1 = 255): white to begin with,
//              then every object in render.draw's order sets or clears its row span, clipped to the
//              screen and the patch.  Spans are exact in integers on the doubled pixel centre
//              (X, Y) = (2x + 1, 2y + 1): a disk covers |X - 2cx| <= isqrt(4r^2 - (Y - 2cy)^2).
//              An object whose box misses the patch is skipped by the whole wave.
//   2. rows    the horizontal pass.  A channel value is 0 or 255, so an output of PIL's pass is a
//              function of the <= 10 mask bits under its filter: one byte of a 1024-entry LDS table
//              per distinct coefficient row (six of them).  Into the u8 intermediate (100, 40) of
//              one channel.
//   3. columns the vertical pass, the arithmetic that is left: 1600 outputs a channel x <= 10 taps in
//              PIL's int accumulator, four neighbouring outputs a lane from one dword per tap.  A lane's
//              four bytes (or, through a 256-entry v / 255 table, its four floats: 16 bytes) go straight
//              out; 60 lanes write 240 (960) contiguous bytes an instruction.
//   2 and 3 run once per channel: the intermediate of one channel (4 000 B) and the masks (4 800 B) are
//   all a wave keeps, so sixteen waves fit a compute unit's LDS -- the kernel is bound by vector
//   instruction issue, and that occupancy is what keeps the issue slots filled.
//   The patch, if asked for, is expanded from the masks in 16-byte stores.
// All integer but the f32 table (one IEEE division an entry) and the isqrt's f32 estimate, which two
// integer corrections make exact.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "ballenv.h"
#include "internal.h"
#include "pixels_host.h"

using namespace behost;

namespace {

struct PParams {
  const int32_t* agent; const int32_t* goal; const int32_t* static_obs; const int32_t* dyn_obs;
  uint8_t* patch; uint8_t* out; float* out_f32;
  int32_t n, ns, nd, sw, sh, ra, ro;
  PixCoeffs c;
};

// The workgroup's dynamic LDS (bytes): the shared tables, then one slice per wave.
struct PixLds {
  static constexpr int WAVES = 8;
  static constexpr int TAB = 0;                                  // u8 [PIX_ROWS][1024]: horizontal outputs by window bits
  static constexpr int F32 = TAB + PIX_ROWS * 1024;              // f32 [256]: v / 255
  static constexpr int KSTRIDE = 12;                             // ints a coefficient row (10 taps, 16-byte aligned rows)
  static constexpr int KK = F32 + 256 * 4;                       // i32 [PIX_ROWS][KSTRIDE]
  static constexpr int SLICE0 = KK + PIX_ROWS * KSTRIDE * 4;
  // a wave's slice
  static constexpr int MASK = 0;                                 // u32 [100][3][4]: row masks
  static constexpr int MASK_BYTES = PIX_PATCH * 3 * 16;
  static constexpr int MID = MASK_BYTES;                         // u8 [100][40]: the horizontal pass's output, one channel
  static constexpr int SLICE = MID + PIX_PATCH * PIX_OUT;
  static constexpr int TOTAL = SLICE0 + WAVES * SLICE;
  static constexpr int IMG_BYTES = 3 * PIX_OUT * PIX_OUT;        // (not LDS: an env's image in memory)
};
static_assert(PixLds::SLICE0 % 16 == 0 && PixLds::SLICE % 16 == 0 && PixLds::MID % 16 == 0, "16-byte aligned slices");
static_assert(PixLds::TOTAL <= 80 * 1024, "two workgroups a compute unit");
static_assert(PIX_PATCH * PIX_PATCH * 3 % 16 == 0 && PixLds::IMG_BYTES % 16 == 0, "whole 16-byte chunks an env");
static_assert(PIX_OUT / 4 * 6 <= 64, "a wave's lanes as 10 output quads x 6 rows");

__device__ __forceinline__ int lo16(int32_t p) { return (int)(int16_t)(p & 0xFFFF); }
__device__ __forceinline__ int hi16(int32_t p) { return p >> 16; }
// PIL's clip8: clamp(v >> 22, 0, 255).  Clamped ahead of the shift -- the same value -- so that four of
// them pack with plain shifts: from shift-then-clamp the compiler forms v_ashr_pk_u8_i32 for two bytes and
// ORs the other two into its result, and with that form bytes 2 and 3 of every packed dword came out wrong
// on gfx950.
__device__ __forceinline__ uint32_t clip8(int v) { return (uint32_t)min(max(v, 0), (256 << PIX_BITS) - 1) >> PIX_BITS; }

// 100 bits of a patch row, one channel
struct Bits { uint64_t lo, hi; };
__device__ __forceinline__ uint64_t ones(int nbits) { return nbits <= 0 ? 0ull : nbits >= 64 ? ~0ull : (1ull << nbits) - 1ull; }
// bits j0..j1 (none if j0 > j1); 0 <= j0, j1 < 128
__device__ __forceinline__ Bits span_bits(int j0, int j1) {
  Bits b;
  b.lo = ones(j1 + 1) & ~ones(j0);
  b.hi = ones(j1 + 1 - 64) & ~ones(j0 - 64);
  return b;
}

// One patch row's channels while the objects are drawn over it.
struct RowPaint {
  Bits r, g, b;
  int Y;             // doubled centre 2y + 1 of this row's world y
  int x0;            // world x of patch column 0
  int cl, cr;        // the row's columns inside the screen (cl > cr: none)
  __device__ __forceinline__ Bits clipped(int xa, int xb) const { return span_bits(max(xa - x0, cl), min(xb - x0, cr)); }
  // colour: bit 0 red, bit 1 green (black 0, red 1, green 2)
  __device__ __forceinline__ void paint(const Bits s, int colour) {
    r.lo = (colour & 1) ? r.lo | s.lo : r.lo & ~s.lo; r.hi = (colour & 1) ? r.hi | s.hi : r.hi & ~s.hi;
    g.lo = (colour & 2) ? g.lo | s.lo : g.lo & ~s.lo; g.hi = (colour & 2) ? g.hi | s.hi : g.hi & ~s.hi;
    b.lo &= ~s.lo; b.hi &= ~s.hi;
  }
  // the disk of radius rad at (cx, cy): |X - 2cx| <= isqrt(4 rad^2 - (Y - 2cy)^2), X odd
  __device__ __forceinline__ void disk(int cx, int cy, int rad, int colour) {
    const int dy = Y - 2 * cy, ady = dy < 0 ? -dy : dy;
    if (ady > 2 * rad) return;                       // (also keeps dy * dy inside int for far-away obstacles)
    const int m = 4 * rad * rad - dy * dy;
    int h = (int)__builtin_sqrtf((float)m);
    if (h * h > m) --h;
    if ((h + 1) * (h + 1) <= m) ++h;
    if (h < 1) return;
    const int ho = (h - 1) | 1;                      // the largest odd |X - 2cx|
    paint(clipped(cx - (ho + 1) / 2, cx + (ho - 1) / 2), colour);
  }
  // the goal's fan, u = X - 2gx, v = Y - 2gy: (u <= 10, v <= 10, u + v >= 0) or (v <= 10, u >= -10, v >= u)
  __device__ __forceinline__ void goal(int gx, int gy) {
    const int v = Y - 2 * gy;
    if (v > 10 || v < -10) return;
    paint(clipped(gx + ((-v - 1) >> 1), gx + 4), 0);
    paint(clipped(gx - 5, gx + ((v - 1) >> 1)), 0);
  }
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(64 * PixLds::WAVES) void pixels_kernel(PParams p) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint8_t* tab = smem + PixLds::TAB;
  float* f32tab = reinterpret_cast<float*>(smem + PixLds::F32);
  int32_t* kk = reinterpret_cast<int32_t*>(smem + PixLds::KK);

  // ---- the tables all eight waves read
#pragma unroll
  for (int r = 0; r < PIX_ROWS; ++r) {
    for (int win = tid; win < 1024; win += 64 * PixLds::WAVES) {
      int acc = 1 << (PIX_BITS - 1);
#pragma unroll
      for (int t = 0; t < PIX_TAPS; ++t) acc += ((win >> t) & 1) ? 255 * p.c.k[r][t] : 0;
      tab[r * 1024 + win] = (uint8_t)clip8(acc);
    }
  }
  if (tid < 256) f32tab[tid] = (float)tid / 255.0f;
  if (tid == 0) {
#pragma unroll
    for (int r = 0; r < PIX_ROWS; ++r)
#pragma unroll
      for (int t = 0; t < PixLds::KSTRIDE; ++t) kk[r * PixLds::KSTRIDE + t] = t < PIX_TAPS ? p.c.k[r][t] : 0;
  }
  __syncthreads();

  uint8_t* slice = smem + PixLds::SLICE0 + w * PixLds::SLICE;
  uint32_t* mask = reinterpret_cast<uint32_t*>(slice + PixLds::MASK);
  uint32_t* mid = reinterpret_cast<uint32_t*>(slice + PixLds::MID);
  // passes 2 and 3: lane = (output quad xq, row r0 of six); its four outputs' table rows and window
  // positions in a mask row are the same for every env
  constexpr int QUADS = PIX_OUT / 4;
  const int xq = lane % QUADS, r0 = lane / QUADS;
  const bool worker = r0 < 6;
  uint32_t tbase[4], word[4], shift[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int first = pix_first_of(4 * xq + s);
    tbase[s] = (uint32_t)pix_row_of(4 * xq + s) * 1024u;
    word[s] = (uint32_t)first >> 5;                 // <= 2: the window never leaves the mask
    shift[s] = (uint32_t)first & 31u;
  }
  const int nobs = p.ns + p.nd;

  for (int e = (int)blockIdx.x * PixLds::WAVES + w; e < p.n; e += (int)gridDim.x * PixLds::WAVES) {
    // ---- 1. row masks
    const int32_t a = p.agent[e], gl = p.goal[e];
    const int ax = lo16(a), ay = hi16(a), gx = lo16(gl), gy = hi16(gl);
    // lane k holds obstacle k (statics, then dynamics), lane k of o1 obstacle 64 + k
    int32_t o0 = 0, o1 = 0;
    if (lane < nobs) o0 = lane < p.ns ? p.static_obs[(int64_t)lane * p.n + e] : p.dyn_obs[(int64_t)(lane - p.ns) * p.n + e];
    if (lane + 64 < nobs) {
      const int k = lane + 64;
      o1 = k < p.ns ? p.static_obs[(int64_t)k * p.n + e] : p.dyn_obs[(int64_t)(k - p.ns) * p.n + e];
    }
    const int reach = PIX_PATCH / 2 + p.ro;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int i = lane + 64 * half;                // patch row (rows 100..127: computed, not stored)
      RowPaint row;
      row.r = row.g = row.b = Bits{~0ull, ~0ull};
      const int y = ay + PIX_PATCH / 2 - 1 - i;
      row.Y = 2 * y + 1;
      row.x0 = ax - PIX_PATCH / 2;
      const bool in_y = y >= 0 && y < p.sh;
      row.cl = max(0, -row.x0);
      row.cr = in_y ? min(PIX_PATCH - 1, p.sw - 1 - row.x0) : -1;
      row.disk(ax, ay, p.ra, 0);
      row.goal(gx, gy);
      for (int k = 0; k < nobs; ++k) {
        const int32_t o = __builtin_amdgcn_readlane(k < 64 ? o0 : o1, k & 63);
        const int cx = lo16(o), cy = hi16(o);
        if (cx - ax > reach || ax - cx > reach || cy - ay > reach || ay - cy > reach) continue;   // wave-uniform
        row.disk(cx, cy, p.ro, k < p.ns ? 1 : 2);
      }
      if (i < PIX_PATCH) {
        uint4* m = reinterpret_cast<uint4*>(mask + i * 12);
        m[0] = make_uint4((uint32_t)row.r.lo, (uint32_t)(row.r.lo >> 32), (uint32_t)row.r.hi, (uint32_t)(row.r.hi >> 32));
        m[1] = make_uint4((uint32_t)row.g.lo, (uint32_t)(row.g.lo >> 32), (uint32_t)row.g.hi, (uint32_t)(row.g.hi >> 32));
        m[2] = make_uint4((uint32_t)row.b.lo, (uint32_t)(row.b.lo >> 32), (uint32_t)row.b.hi, (uint32_t)(row.b.hi >> 32));
      }
    }
    wave_sync();

    // ---- the patch, (100, 100, 3) u8: byte b is channel b % 3 of pixel b / 3
    if (p.patch) {
      uint4* dst = reinterpret_cast<uint4*>(p.patch + (int64_t)e * (PIX_PATCH * PIX_PATCH * 3));
      for (int q = lane; q < PIX_PATCH * PIX_PATCH * 3 / 16; q += 64) {
        int px = (16 * q) / 3, c = 16 * q - 3 * px;
        int i = px / PIX_PATCH, j = px - PIX_PATCH * i;
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          const uint32_t bit = (mask[i * 12 + c * 4 + (j >> 5)] >> (j & 31)) & 1u;
          v[b >> 2] |= (bit ? 255u : 0u) << (8 * (b & 3));
          if (++c == 3) { c = 0; if (++j == PIX_PATCH) { j = 0; ++i; } }
        }
        dst[q] = make_uint4(v[0], v[1], v[2], v[3]);
      }
      wave_sync();     // (a patch-only call: the next env's masks overwrite what these lanes read)
    }

    if (p.out || p.out_f32) {
      uint32_t* out32 = reinterpret_cast<uint32_t*>(p.out + (p.out ? (int64_t)e * PixLds::IMG_BYTES : 0));
      float4* outf4 = reinterpret_cast<float4*>(p.out_f32 + (p.out_f32 ? (int64_t)e * PixLds::IMG_BYTES : 0));
      for (int c = 0; c < 3; ++c) {
        // ---- 2. horizontal pass of channel c: two LDS round trips a row -- its 128-bit mask, then the
        // four table bytes (the windows are cut out of the mask in registers)
        if (worker) {
          for (int i = r0; i < PIX_PATCH; i += 6) {
            const uint4 m = reinterpret_cast<const uint4*>(mask + i * 12)[c];
            uint32_t hv = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const uint32_t lo = word[s] == 0 ? m.x : word[s] == 1 ? m.y : m.z;
              const uint32_t hi = word[s] == 0 ? m.y : word[s] == 1 ? m.z : m.w;
              hv |= (uint32_t)tab[tbase[s] + (__builtin_amdgcn_alignbit(hi, lo, shift[s]) & 1023u)] << (8 * s);
            }
            mid[i * QUADS + xq] = hv;
          }
        }
        wave_sync();

        // ---- 3. vertical pass of channel c, and out
        if (worker) {
          for (int yy = r0; yy < PIX_OUT; yy += 6) {
            const int first = pix_first_of(yy), rid = pix_row_of(yy);
            int acc[4] = {1 << (PIX_BITS - 1), 1 << (PIX_BITS - 1), 1 << (PIX_BITS - 1), 1 << (PIX_BITS - 1)};
#pragma unroll
            for (int t = 0; t < PIX_TAPS; ++t) {
              // a row cut by the patch's edge has zero coefficients behind its taps: any row in range will do
              const uint32_t v = mid[min(first + t, PIX_PATCH - 1) * QUADS + xq];
              const int32_t k = kk[rid * PixLds::KSTRIDE + t];
#pragma unroll
              for (int s = 0; s < 4; ++s) acc[s] += __mul24((int)((v >> (8 * s)) & 255u), k);   // |k| < 2^23 (pix_coeffs)
            }
            const uint32_t b0 = clip8(acc[0]), b1 = clip8(acc[1]), b2 = clip8(acc[2]), b3 = clip8(acc[3]);
            const int at = (c * PIX_OUT + yy) * QUADS + xq;
            if (p.out) out32[at] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
            if (p.out_f32) outf4[at] = make_float4(f32tab[b0], f32tab[b1], f32tab[b2], f32tab[b3]);
          }
        }
        wave_sync();     // the next channel's (or env's) writes overwrite what this pass read
      }
    }
  }
}

const PixCoeffs* coeffs() {
  static const struct Packed { PixCoeffs c; bool ok; Packed() { ok = pix_coeffs_pack(&c); } } packed;
  return packed.ok ? &packed.c : nullptr;
}

}  // namespace

extern "C" {

int be_pixels_coeffs(int32_t* kk, int32_t* bounds) {
  if (!kk || !bounds) return be_ctx_fail(nullptr, BE_E_INVALID, "be_pixels_coeffs needs kk and bounds");
  int32_t k[PIX_OUT][PIX_TAPS], b[PIX_OUT][2];
  if (!pix_coeffs(k, b)) return be_ctx_fail(nullptr, BE_E_INVALID, "be_pixels_coeffs: the coefficients overflow the int accumulator");
  memcpy(kk, k, sizeof k);
  memcpy(bounds, b, sizeof b);
  return BE_OK;
}

int be_observe_pixels(be_ctx* ctx, const be_state* st, uint8_t* patch, uint8_t* out, float* out_f32, void* stream) {
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  const be_ctx_view cv = be_ctx_get(ctx);
  if (const char* msg = pixels_args_error(patch, out, out_f32, cv.radius_agent, cv.radius_obstacle))
    return be_ctx_fail(ctx, BE_E_INVALID, msg);
  const PixCoeffs* c = coeffs();
  if (!c) return be_ctx_fail(ctx, BE_E_INVALID, "be_observe_pixels: the resize coefficients are not the six expected rows");
  BE_ENTER_DEVICE(be_ctx_err(ctx), cv.device);
  int cus = 0;
  BE_HIP_TRY(be_ctx_err(ctx), hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cv.device));
  PParams p{st->agent, st->goal, st->static_obs, st->dyn_obs, patch, out, out_f32, cv.num_envs, cv.num_static, cv.num_dynamic,
            cv.screen_width, cv.screen_height, cv.radius_agent, cv.radius_obstacle, *c};
  // two workgroups fit a compute unit's LDS; past that a wave takes several envs, which spreads the tables' cost
  const int64_t want = ((int64_t)cv.num_envs + PixLds::WAVES - 1) / PixLds::WAVES, cap = 2 * (int64_t)(cus > 0 ? cus : 1);
  const unsigned grid = (unsigned)(want < cap ? want : cap);
  hipLaunchKernelGGL(pixels_kernel, dim3(grid), dim3(64 * PixLds::WAVES), (size_t)PixLds::TOTAL, (hipStream_t)stream, p);
  return be_launched(be_ctx_err(ctx));
}

}  // extern "C"
