// a2c.hip -- the targets of the batched A2C finish_episode (examples/ball_cnn_ac3.py:222-246,
// SURVEY §8(f) rank 1) from a recorded (T, N) rollout:
//
//   be_a2c_targets   discounted return R_t (f64, cut at every done), its f32 rounding, the
//                    per-episode mean / unbiased std normalisation, advantage and the
//                    "episode has >= 2 steps" mask.
//
// One lane per env (the env index is the unit-stride axis of every (T, N) array, so every row
// access is coalesced); every lane walks its own column, all lanes of a wave at the same row.
// The arithmetic and its order are pinned (include/ballenv.h), so the result is reproducible bit
// for bit: no atomics, no cross-lane sums.
//
// Three sweeps over t, each a stream of whole rows in load groups of ROWS rows: a group's loads
// are in flight while the group before it runs through the serial chain:
//
//   1 (t = T-1 .. 0)  R, r32 = (float)R into returns_norm (the f32 scratch between the sweeps),
//                     the episode's sum in decreasing t.  When the walk passes an episode's first
//                     step its mean is known:
//                       L == 1        zeros / valid = 0 are written
//                       2 <= L <= 16  finished on the spot by its lane (<= 16 rows just written)
//                       L > 16        the f64 mean is parked in valid[s .. s+7], one byte a row
//   2 (t = 0 .. T-1)  episodes of L > 16: ss = sum (r32 - mean)^2 in increasing t; at the last
//                     step sqrt(ss / (L-1)) is parked in valid[s+8 .. s+15]
//   3 (t = 0 .. T-1)  episodes of L > 16: returns_norm, advantage, valid = 1 (the rows of shorter
//                     episodes are stored again as they stand: see Park)
//
// The parked bytes need no scratch buffer and no per-episode storage of unknown size: an episode
// of more than 16 steps owns 16 bytes of `valid` that sweep 3 overwrites last.  Sweeps 2 and 3
// read them (and the dones) 16 rows ahead through shift registers -- valid[t .. t+15] in two
// 64-bit words, "row ends an episode" for t .. t+15 in a 16-bit mask -- so an episode's first row
// finds its mean, its std and "more than 16 steps" in registers and no lane ever waits on a
// load of its own.  A wave with no episode of more than 16 steps skips sweeps 2 and 3.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "ballenv.h"
#include "internal.h"

namespace {

#ifndef BE_A2C_ROWS
#define BE_A2C_ROWS 8       // -DBE_A2C_ROWS=n: A/B builds (profiles/a2c_targets.json)
#endif
constexpr int ROWS = BE_A2C_ROWS;   // rows per load group
constexpr int PARK = 16;    // episodes of more than PARK steps park mean / std in `valid`

struct AParams {
  const double* __restrict__ rewards; const uint8_t* __restrict__ dones; const float* __restrict__ values;
  const double* __restrict__ bootstrap;
  double* __restrict__ returns; float* rn; float* __restrict__ adv; uint8_t* valid;
  int32_t n, steps;
  double gamma, eps;
};

__device__ __forceinline__ void park8(uint8_t* valid, int64_t row0, int64_t n, double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
#pragma unroll
  for (int k = 0; k < 8; ++k) valid[(row0 + k) * n] = (uint8_t)(b >> (8 * k));
}

// an episode of 2 <= L <= PARK steps whose r32 stand in rn[s .. s+L-1]: steps 3-5 by its own lane
__device__ __forceinline__ void finish_short(const AParams& p, int i, int s, int L, double sum) {
  const int64_t n = p.n, o0 = (int64_t)s * n + i;
  const double mean = sum / (double)L;
  double ss = 0.0;
  for (int j = 0; j < L; ++j) {
    const double dl = (double)p.rn[o0 + j * n] - mean;
    ss = ss + dl * dl;
  }
  const double den = sqrt(ss / (double)(L - 1)) + p.eps;
  for (int j = 0; j < L; ++j) {
    const int64_t o = o0 + j * n;
    const float z = (float)(((double)p.rn[o] - mean) / den);
    p.rn[o] = z;
    if (p.adv) p.adv[o] = z - p.values[o];
    p.valid[o] = 1;
  }
}

// the episode [s, s+L-1] that the backward walk has just left (L == 0: none yet)
__device__ __forceinline__ bool close_episode(const AParams& p, int i, int s, int L, double sum) {
  if (L == 1) {
    const int64_t o = (int64_t)s * p.n + i;
    p.rn[o] = 0.0f;
    if (p.adv) p.adv[o] = 0.0f;
    p.valid[o] = 0;
  } else if (L >= 2 && L <= PARK) {
    finish_short(p, i, s, L, sum);
  } else if (L > PARK) {
    park8(p.valid + i, s, p.n, sum / (double)L);
    return true;
  }
  return false;
}

// A park in progress: the 8 bytes of `bits` go to valid rows row0 .. row0+7 one per processed row,
// through the one byte store every row issues anyway (a lane that has nothing to park stores a
// byte that changes nothing).  The counted vmcnt waits hipcc places in front of a load group's
// first use assume the fewest stores any path issues; a store inside a branch makes the wait
// stricter than the loads need (the wave then sits out that store's round trip), so the streaming
// loops keep every lane's memory operations the same whatever the episodes look like.
struct Park { uint64_t bits = 0; int row0 = 0, left = 0; };

__device__ __forceinline__ void park_step(Park& pk, uint8_t* valid, int i, int64_t n, int idle_row, uint8_t idle_byte) {
  const bool on = pk.left > 0;
  const int k = pk.left - 1;
  const int row = on ? pk.row0 + k : idle_row;
  valid[(int64_t)row * n + i] = on ? (uint8_t)(pk.bits >> (8 * (k & 7))) : idle_byte;
  pk.left -= on ? 1 : 0;
}

__device__ __forceinline__ void park_flush(Park& pk, uint8_t* valid, int i, int64_t n) {
  while (pk.left > 0) park_step(pk, valid, i, n, 0, 0);
}

struct Back { double r[ROWS]; uint8_t d[ROWS]; };

__device__ __forceinline__ void load_back(const AParams& p, int i, int t0, Back& b) {
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    const int64_t o = (int64_t)max(t0 - j, 0) * p.n + i;     // rows below 0: row 0 again, unused
    b.r[j] = p.rewards[o];
    b.d[j] = p.dones[o];
  }
}

// sweeps 2 and 3 read row t + PARK of dones / valid and row t of r32 (and values) at stream index t
struct Fwd { float x[ROWS]; float v[ROWS]; uint8_t d[ROWS]; uint8_t b[ROWS]; };

template <bool LAST, bool ADV>
__device__ __forceinline__ void load_fwd(const AParams& p, int i, int t0, Fwd& f) {
  const int T = p.steps;
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    const int t = t0 + j;
    const int64_t oa = (int64_t)min(t + PARK, T - 1) * p.n + i;   // rows past T-1: the last row, overridden
    const int64_t o = (int64_t)min(max(t, 0), T - 1) * p.n + i;
    f.d[j] = p.dones[oa];
    f.b[j] = p.valid[oa];
    f.x[j] = p.rn[o];
    if (LAST && ADV) f.v[j] = p.values[o];
  }
}

// Two register sets, each reloaded right after its rows ran, so a set's loads fly while the other
// set runs (a `cur = nxt` copy makes hipcc drain every load and store before the next group's
// loads).  Groups that lie wholly inside [0, T) run without the per-row range test: a branch
// around a row's stores would again leave the waits nothing to count on.
#define BE_A2C_PINGPONG(LOAD, ROWS_FN, T0, STEP, INSIDE, MORE)              \
  for (; (MORE) && !(INSIDE); T0 += 2 * (STEP)) {                          \
    LOAD(b, T0 + (STEP)); ROWS_FN(a, T0, std::true_type{});                \
    LOAD(a, T0 + 2 * (STEP)); ROWS_FN(b, T0 + (STEP), std::true_type{});   \
  }                                                                        \
  for (; (MORE) && (INSIDE); T0 += 2 * (STEP)) {                           \
    LOAD(b, T0 + (STEP)); ROWS_FN(a, T0, std::false_type{});               \
    LOAD(a, T0 + 2 * (STEP)); ROWS_FN(b, T0 + (STEP), std::false_type{});  \
  }                                                                        \
  for (; (MORE); T0 += 2 * (STEP)) {                                       \
    LOAD(b, T0 + (STEP)); ROWS_FN(a, T0, std::true_type{});                \
    LOAD(a, T0 + 2 * (STEP)); ROWS_FN(b, T0 + (STEP), std::true_type{});   \
  }

template <bool LAST, bool ADV>
__device__ __forceinline__ void forward_sweep(const AParams& p, int i) {
  const int T = p.steps;
  const int64_t n = p.n;
  uint64_t lo = 0, hi = 0;     // valid[t .. t+7], valid[t+8 .. t+15]
  uint32_t ends = 0;           // bit k: row t+k is the last of its episode (done, or T-1)
  bool start = true, parked = false;
  double mean = 0.0, ss = 0.0, den = 1.0;
  int s = 0;
  Park pk;
  // one load group through the serial chain (stream indices t0 .. t0+ROWS-1)
  auto rows = [&](const Fwd& cur, int t0, auto guard) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const int t = t0 + j;
      if (!decltype(guard)::value || (t >= 0 && t < T)) {
        const bool end = ends & 1u;
        const uint8_t vb = (uint8_t)lo;          // valid[t] as it stands
        if (start) {
          parked = (ends & 0xFFFFu) == 0;        // no end in t .. t+15: more than PARK steps
          mean = parked ? __longlong_as_double((long long)lo) : mean;
          if (LAST) den = parked ? __longlong_as_double((long long)hi) + p.eps : den;
          ss = 0.0;
          s = t;
        }
        const int64_t o = (int64_t)t * n + i;
        const double dl = (double)cur.x[j] - mean;
        if (LAST) {
          // every row is stored: rows of shorter episodes get back what they hold (their advantage
          // recomputed by the same f32 subtraction)
          const float z = parked ? (float)(dl / den) : cur.x[j];
          const bool ok = parked || vb != 0;
          p.rn[o] = z;
          if (ADV) p.adv[o] = ok ? z - cur.v[j] : 0.0f;
          p.valid[o] = ok ? 1 : 0;
        } else {
          ss = ss + dl * dl;
          if (parked && end) {
            pk.bits = (uint64_t)__double_as_longlong(sqrt(ss / (double)(t - s)));
            pk.row0 = s + 8;
            pk.left = 8;
          }
          park_step(pk, p.valid, i, n, t, vb);
        }
        if (end) parked = false;
        start = end;
      }
      const uint32_t e16 = (cur.d[j] != 0 || t + PARK >= T - 1) ? 1u : 0u;
      lo = (lo >> 8) | (hi << 56);
      hi = (hi >> 8) | ((uint64_t)cur.b[j] << 56);
      ends = (ends >> 1) | (e16 << (PARK - 1));
    }
  };
  Fwd a{}, b{};
  int t0 = -PARK;
  load_fwd<LAST, ADV>(p, i, t0, a);
#define BE_LOAD_F(buf, t) load_fwd<LAST, ADV>(p, i, t, buf)
  BE_A2C_PINGPONG(BE_LOAD_F, rows, t0, ROWS, t0 >= 0 && t0 + 2 * ROWS <= T, t0 < T)
#undef BE_LOAD_F
  if (!LAST) park_flush(pk, p.valid, i, n);
}

template <bool RET, bool ADV>
__global__ __launch_bounds__(64) void a2c_targets_kernel(AParams p) {
  const int i = blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= p.n) return;
  const int T = p.steps;
  const int64_t n = p.n;
  double acc = p.bootstrap ? p.bootstrap[i] : 0.0, sum = 0.0;
  int L = 0;
  bool any_parked = false;
  Park pk;
  auto rows = [&](const Back& cur, int t0, auto guard) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const int t = t0 - j;
      if (!decltype(guard)::value || t >= 0) {
        if (cur.d[j]) {                        // row t ends an episode: the one above it is complete
          if (L > PARK) {
            pk.bits = (uint64_t)__double_as_longlong(sum / (double)L);
            pk.row0 = t + 1;
            pk.left = 8;
            any_parked = true;
          } else {
            close_episode(p, i, t + 1, L, sum);
          }
          acc = 0.0;
          sum = 0.0;
          L = 0;
        }
        const double ga = p.gamma * acc;       // one f64 multiply, then one f64 add (-ffp-contract=off)
        acc = cur.r[j] + ga;
        const int64_t o = (int64_t)t * n + i;
        if (RET) p.returns[o] = acc;
        const float r32 = (float)acc;
        p.rn[o] = r32;
        park_step(pk, p.valid, i, n, t, 0);    // idle: valid[t] = 0 for now, its episode is still open
        sum = sum + (double)r32;
        ++L;
      }
    }
  };
  Back a, b;
  int t0 = T - 1;
  load_back(p, i, t0, a);
#define BE_LOAD_B(buf, t) load_back(p, i, t, buf)
  BE_A2C_PINGPONG(BE_LOAD_B, rows, t0, -ROWS, t0 - 2 * ROWS + 1 >= 0, t0 >= 0)
#undef BE_LOAD_B
  park_flush(pk, p.valid, i, n);
  any_parked |= close_episode(p, i, 0, L, sum);
  if (!__any(any_parked)) return;              // wave-uniform: no episode of more than PARK steps
  forward_sweep<false, ADV>(p, i);
  forward_sweep<true, ADV>(p, i);
}

}  // namespace

extern "C" {

int be_a2c_targets(be_ctx* ctx, const double* rewards, const uint8_t* dones, const float* values,
                   const double* bootstrap, int32_t steps, double gamma, double eps, const be_a2c_out* out,
                   void* stream) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  if (!rewards || !dones) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_targets needs rewards and dones");
  if (!out) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_targets: out is NULL");
  if (!out->returns_norm || !out->valid)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_targets needs out->returns_norm and out->valid");
  if (out->advantage && !values) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_targets: advantage needs values");
  if (steps < 1) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_targets: steps must be >= 1");
  if (!isfinite(gamma)) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_targets: gamma must be finite");
  if (!(eps >= 0.0)) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_targets: eps must be >= 0");
  const be_ctx_view cv = be_ctx_get(ctx);
  BE_ENTER_DEVICE(be_ctx_err(ctx), cv.device);
  AParams p{rewards, dones, values, bootstrap, out->returns, out->returns_norm, out->advantage, out->valid,
            cv.num_envs, steps, gamma, eps};
  const dim3 grid((unsigned)((cv.num_envs + 63) / 64)), block(64);
  hipStream_t hs = (hipStream_t)stream;
  if (out->returns) {
    if (out->advantage) hipLaunchKernelGGL((a2c_targets_kernel<true, true>), grid, block, 0, hs, p);
    else hipLaunchKernelGGL((a2c_targets_kernel<true, false>), grid, block, 0, hs, p);
  } else {
    if (out->advantage) hipLaunchKernelGGL((a2c_targets_kernel<false, true>), grid, block, 0, hs, p);
    else hipLaunchKernelGGL((a2c_targets_kernel<false, false>), grid, block, 0, hs, p);
  }
  return be_launched(be_ctx_err(ctx));
}

}  // extern "C"
