// step_types.h -- what the step engine's two translation units share: the kernel argument blocks,
// the per-context tables, the autoreset pool's layout (pool_layout.h), the fixed-shape limits and the dispatch
// interface.  Host and device, no kernels.
//   csrc/ballenv.hip  the kernels and their dispatcher (defines the interface at the end of this file)
//   csrc/abi.hip      be_ctx and every C entry point (calls it; names no kernel)
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "ballenv.h"
#include "pool_layout.h"

namespace bestep {

constexpr int HW_MAX = 63;   // largest collision radius R with a half-width table

enum Mode { MODE_STEP = 0, MODE_RESET = 1, MODE_OBSERVE = 2 };

// Per-context tables: a device buffer staged into LDS once per block.
struct Tables {
  int32_t goal[BE_MAX_GOALS];                 // packed goal xy
  int32_t action[BE_MAX_ACTIONS];             // packed (dx, dy)
  int32_t speed[BE_MAX_DYNAMIC];              // obstacle_speed
  int32_t strip_obs_x, strip_obs_y, strip_goal_x, strip_goal_y, strip_agent_x, strip_agent_y;
  int32_t radius_obstacle, radius_agent;
  uint8_t n_other[BE_MAX_GOALS];              // goals with a different value than goal g
  uint8_t other[BE_MAX_GOALS][BE_MAX_GOALS];  // pick -> goal index, per current goal g (newGoalList)
  uint8_t hw[HW_MAX + 1];                     // floor(sqrt(R^2 - d^2)), d = 0..R (only when R <= HW_MAX)
};

// The fixed-shape step kernels' 64-bit row-span table (span_fits: W-1+2R <= 63): span[j] holds the cells an obstacle
// at window column C = W-1+R lights in a row at distance |j - J0| (J0 = R+K-1): bits C-hw .. C+hw,
// 0 past R.  A near entry at window (f, e) lights row k with span[e - k + J0] >> (C - f), clipped to
// W bits -- one LDS read, one shift and one OR per row (raster_rows_span).  It follows Tables in the
// same device buffer; only the fixed-shape step kernels stage it.
constexpr int SPAN_N = 72;
struct TablesX {
  Tables t;
  uint64_t span[SPAN_N];
};
static_assert(sizeof(Tables) % 16 == 0 && sizeof(TablesX) % 16 == 0, "16-byte table staging");
__host__ __device__ constexpr bool span_fits(int W, int R) {   // W >= 2: K = W-1 rows, J0 = R+W-2
  return W >= 2 && R >= 0 && W - 1 + 2 * R <= 63 && 2 * R + 2 * (W - 1) - 1 <= SPAN_N;
}

// Kernel arguments: hot fields first, 64-byte lines (see the latency notes at the top of ballenv.hip).
struct KParams {
  // line 0
  int32_t* agent; int32_t* goal; double* prev_dist; double* total_dist;
  double* ep_return; int32_t* ep_len; uint32_t* episode; int32_t* static_obs;
  // line 1
  int32_t* dyn_obs; uint8_t* dyn_goal; uint8_t* obs; float* obs_f32;
  double* reward; uint8_t* done; const uint8_t* actions; const Tables* tables;
  // line 2
  int32_t n, window, ns, nd, R, speed_x, speed_y, screen_w;
  int32_t screen_h, goal_change, certainty, time_limit, num_actions, autoreset, gid0, dbg;
  // line 3
  double threshold_goal, time_penalty, static_penalty, dynamic_penalty, min_spawn_dist;
  double inv_g1;               // 1 / (goal_change + 1): counter = ep_len mod (G+1) without an integer divide
  unsigned long long seed;
  int* status;
  // line 4 (cold)
  const int16_t* deltas; const int16_t* tape; const uint8_t* mask; const int16_t* reset_tape;
  uint8_t* truncated; uint8_t* terminal_obs; double* final_return; int32_t* final_len;
  // line 5 (cold)
  double* stats;               // (slots, 8): one slot per wave / block of the step kernel (be_stats_slots)
  int32_t reset_tape_len;
  int32_t min_spawn_d2;        // integer d2: sqrt(d2) < min_spawn_dist  <=>  d2 < min_spawn_d2
  // fixed-shape kernels only (pick_kernel checks the preconditions):
  uint32_t amx, amy;           // action a's (dx+1, dy+1) at bits 2a..2a+1 (every move in {-1,0,1})
  int32_t num_goals;           // goals pairwise distinct: newGoalList(g)[pick] = pick + (pick >= g)
  int32_t prev_read;           // 1: read prev_dist; 0 (A/B only, when no reset can re-sample the agent,
                               // Q9): prev_dist == calc_dist(goal, agent), recomputed
  int32_t steps;               // rollout_kernel: steps per launch (actions / outputs are (steps, N, ...))
  // fused policy rollouts (rollout_kernel with HT > 0, be_policy_rollout)
  int32_t pol_bytes, pol_actions;
  const uint8_t* pol_img;      // packed Policy(W) image (policy_core.h PolLayout)
  const uint8_t* obs_in;       // (N, F) obs of the current state: step 0's policy input
  uint8_t* obs_last;           // (N, F) obs after the last step, or NULL
  uint8_t* act_out; float* logp_out; float* value_out;   // (steps, N)
  unsigned long long pol_seed;
  // the autoreset pool (pool_layout.h; nullptr: every reset is drawn inline)
  uint32_t* pool;
};

// mlp_rollout_kernel's own arguments, beside the KParams of the call (be_mlp_rollout)
struct MlpRollParams {
  const float* img;            // packed block-MLP image (mlp_core.h MlpLayout)
  uint8_t* blocks_out;         // (steps, N, 29) or NULL: the counts each action was drawn from
  uint8_t* action;             // (steps, N)
  float* log_prob;             // (steps, N) or NULL
  unsigned long long seed;
  int32_t num_actions, final_relu;
};

// step2_kernel's arguments (launch_kernel fills all three from the one KParams of the call):
//  * 14 dwords of leading scalars.  gfx950's dispatcher preloads them into user SGPRs while the
//    wave launches (-amdgpu-kernarg-preload-count, build.py; a by-value struct is not preloaded),
//    so the loads through them -- the tables, episode / ep_len, every obstacle -- issue at once,
//    with no scalar load from the kernarg segment in front of them;
//  * KHot: what the prologue's other loads go through, one 64-byte line of the kernarg segment.
//    Its scalar load is issued first of all and is the only one the prologue waits for;
//  * KParams, as every other kernel takes it: read after the prologue's loads are in flight.
// (Stamps and A/B: DESIGN 3.3, profiles/r08_*.)
struct alignas(64) KHot {
  int32_t* agent; int32_t* goal; double* prev_dist; double* total_dist; double* ep_return;
  const uint8_t* actions; double* stats; int32_t prev_read, goal_change;
};
static_assert(sizeof(KHot) == 64, "one line of the kernarg segment");

#ifndef BE_S2_CT
#define BE_S2_CT 256        // step2_kernel: threads per block (A/B)
#endif
constexpr int S2_CT = BE_S2_CT;
constexpr int BLOCK_THREADS = 256;   // be_kernel, rollout_kernel: threads (and envs) per block

// Fixed-shape step kernels for the reference's default obstacle counts (ball_cnn_ac3.py:40-41).
constexpr int FIX_NS = 13, FIX_ND = 5;
// The fixed-shape kernels address per-env arrays as a uniform base + a 32-bit byte offset (ld_s /
// st_ws): element i of an 8-byte array needs i < 2^29.  Larger batches (~150 GB of state and outputs)
// take the generic kernels, which index in 64 bits.
constexpr int64_t FIX_MAX_ENVS = 1ll << 29;

// ------------------------------------------------------------------ dispatch interface
// The kernel unit describes what it picked; the ABI unit decides from the description and hands it
// back to launch_kernel.  Nothing outside csrc/ballenv.hip names a kernel.
using KFn = void (*)(KParams);
// step2_kernel: its leading scalar arguments (preloaded into SGPRs), KHot, then the KParams
using KFn2 = void (*)(const Tables*, uint32_t*, int32_t*, int32_t*, uint8_t*, int32_t*, int32_t, int32_t, KHot, KParams);
using KFnMlp = void (*)(KParams, MlpRollParams);   // mlp_rollout_kernel
enum Kind {
  KIND_NONE = 0,         // no kernel for this config (Launch::ok() is false)
  KIND_GENERIC,          // be_kernel<W or 0, mode>: any config, step / reset / observe
  KIND_FIXED1,           // be_kernel<W, STEP, 13, 5>: fixed shape, one lane per env
  KIND_STEP2,            // step2_kernel: fixed shape at W = 10, two lanes per env
  KIND_LANES,            // stepw_kernel / rolloutw_kernel: fixed shape at W = 5, 4 or 8 lanes per env
  KIND_ROLLOUT,          // rollout_kernel: the fused multi-step rollout
  KIND_POLICY_ROLLOUT,   // rollout_kernel with the policy in the loop
  KIND_MLP_ROLLOUT,      // mlp_rollout_kernel: the block-count policy and the step in one kernel
  KIND_POOL_FILL         // pool_fill_kernel
};
struct Launch {
  KFn fn = nullptr;
  KFn2 fn2 = nullptr;            // step2_kernel (fn is nullptr then)
  KFn2 fn2_recompute = nullptr;  // its KParams::prev_read = 0 instance (A/B only; launch_kernel picks by the flag)
  KFn2 fn2_wide = nullptr;       // its wide-row-load instance (be_step takes it per call: behost::step2_wide)
  KFnMlp fnm = nullptr;          // mlp_rollout_kernel (fn and fn2 are nullptr then; launch_mlp_rollout)
  int kind = KIND_NONE;
  int epb = BLOCK_THREADS;       // envs per block
  int threads = BLOCK_THREADS;
  int lds = 0;                   // dynamic LDS bytes: the kernel's own layout (its *Lds struct)
  bool consumes_pool = false;    // a step kernel whose `pool` instance copies autoreset-pool entries
  char name[48] = {0};
  bool ok() const { return fn || fn2 || fnm; }
  // the device function, for hipFuncGetAttributes
  const void* entry() const {
    return fn ? reinterpret_cast<const void*>(fn) : (fn2 ? reinterpret_cast<const void*>(fn2) : reinterpret_cast<const void*>(fnm));
  }
};
#define BE_HIDDEN __attribute__((visibility("hidden")))
// fixed_ok: the context's part of the fixed-shape preconditions (unit moves, pairwise-distinct goals,
// no BALLENV_GENERIC_KERNELS) and, per launch, actions given and no draw tape; the config's part
// (13 / 5 obstacles, unit speeds, R <= HW_MAX, N < FIX_MAX_ENVS) is checked here.
// lanes10 / lpe5: lanes per env of the fixed step kernel at W = 10 (1, 2) / W = 5 (1, 4, 8).
// pool: the instance that copies finished envs' resets from the autoreset pool (the context passes it
// only with a pool allocated).
BE_HIDDEN Launch pick_kernel(const be_config& c, int mode, bool fixed_ok = false, int lanes10 = 1, int lpe5 = 0,
                             bool pool = false);
// The fused rollout for the fixed shapes, and the fused policy rollout for the select_action
// kernel's Policy(W) shapes (H 208 / W 10 and H 128 / W 5, 9 actions); !ok(): not applicable.
BE_HIDDEN Launch pick_rollout(const be_config& c, bool fixed_ok, int lpe5 = 0);
BE_HIDDEN Launch pick_policy_rollout(const be_config& c, bool fixed_ok, int HT, int KS, int NO);
// The fused block-policy rollout for the fixed env shape (any window: it writes no observation), one
// instance per layer count (2, 3) and waves per workgroup (1, 2, 4, 8); !ok(): not applicable.
BE_HIDDEN Launch pick_mlp_rollout(const be_config& c, bool fixed_ok, int layers, int waves);
BE_HIDDEN void launch_mlp_rollout(const Launch& L, const KParams& a, const MlpRollParams& q, hipStream_t stream);
BE_HIDDEN Launch pick_pool_fill(int window);   // window 10 or 5 (the kernels with consumes_pool)
// The one place a step-engine kernel is launched: ceil(a.n / L.epb) blocks of L.threads, L.lds bytes.
// wide: step2_kernel's wide-row-load instance (the caller has checked behost::step2_wide for a's arrays;
// the prev_read = 0 A/B instance has no wide twin and ignores it).
BE_HIDDEN void launch_kernel(const Launch& L, const KParams& a, hipStream_t stream, bool wide = false);
BE_HIDDEN void launch_sample_actions(uint8_t* out, int32_t n, int32_t steps, int64_t env_offset, int32_t num_actions,
                                     unsigned long long seed, hipStream_t stream);

}  // namespace bestep
