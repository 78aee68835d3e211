/*
 * ballenv.h -- C ABI of the MI355X batched BallEnv step engine (libballenv.so).
 *
 * The reference (ranok92/gym-ballenv) is pure Python; the "FFI" this library
 * stands behind is the gym.Env protocol that examples/ball_cnn_ac3.py drives:
 *
 *   be_config            <- BallEnv.__init__ constants + customize_environment(args)
 *                           (gym_ballenv/envs/ballenv_env.py:11-18, 43-85, 87-109;
 *                            argparse defaults examples/ball_cnn_ac3.py:37-59)
 *   be_reset             <- BallEnv.reset()            (ballenv_env.py:113-167)
 *   be_step              <- BallEnv.step(action)       (ballenv_env.py:232-289, incl.
 *                           move_obstacles :323-353, calculate_reward :200-229,
 *                           check_overlap :185-191) followed by
 *                           prep_state4(state, W)      (examples/ball_cnn_ac3.py:384-412,
 *                           quadrant prep_state2 :330-352) and the gym TimeLimit
 *                           registered with timestep_limit=1000 (gym_ballenv/__init__.py:4-11)
 *   be_observe           <- prep_state4(state, W) on the current state
 *
 * Conventions
 *   - Plain C: no C++ types, no exceptions cross this boundary.  Every entry
 *     point returns BE_OK (0) or a negative BE_E* code; be_last_error() gives
 *     the message for the last failing call on that context (or, for a NULL
 *     context, the last process-wide failure).
 *   - All per-env device buffers are allocated and owned by the CALLER
 *     (PyTorch tensors); the library owns one word of device scratch (the
 *     status word).  Every compute call is asynchronous and
 *     ordered on the hipStream_t the caller passes (as void*).
 *   - Layout is struct-of-arrays with the env index as the unit-stride axis:
 *     an (x, y) position is two int16 in one 32-bit word (x low, y high),
 *     i.e. an (N, 2) int16 array; per-obstacle arrays are (K, N, 2) int16.
 *   - One context per (device, config).  No internal threads.  Every entry point
 *     makes the context's device current for the call and restores the calling
 *     thread's current device before it returns: no be_* call changes which GPU
 *     the caller's later HIP / torch calls use.
 *   - Randomness (perf mode): Philox4x32-10 keyed by cfg.seed with counter
 *     (global env id, episode, ep_len, purpose|sub).  Every draw is a pure
 *     function of per-env state, so results do not depend on launch order,
 *     graph replay, or how the batch is split across GPUs.
 */
#ifndef BALLENV_H
#define BALLENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BE_ABI_VERSION 7

#define BE_MAX_STATIC   64
#define BE_MAX_DYNAMIC  32
#define BE_MAX_GOALS    16
#define BE_MAX_ACTIONS  16
#define BE_MAX_WINDOW   64

enum {
  BE_OK = 0,
  BE_E_INVALID = -1,   /* bad argument / config */
  BE_E_HIP = -2,       /* HIP runtime error */
  BE_E_NOMEM = -3,
  BE_E_DEVICE = -4     /* device-side status word reported a failure */
};

/* Device-side status bits (be_status). */
enum {
  BE_STATUS_RESET_TAPE_EXHAUSTED = 1,  /* a reset consumed more draws than its tape held */
  BE_STATUS_REJECTION_LIMIT = 2,       /* a reset rejection loop hit its bound */
  BE_STATUS_BAD_ACTION = 4,            /* action index >= num_actions */
  BE_STATUS_COORD_RANGE = 8,           /* a dynamic obstacle left the int16 range; the stored
                                          coordinate wraps (two's complement int16).  The
                                          reference's obstacles are unbounded ints (ballenv_env.py
                                          :334-347).  be_config_check rejects configs that can get
                                          here within an episode (autoreset with a time limit);
                                          with time_limit 0 or autoreset 0 poll be_status. */
  BE_STATUS_NO_GOAL = 16               /* goal change with no other goal (reference raises) */
};

typedef struct be_config {
  int32_t num_envs;          /* N on this device */
  int32_t window;            /* W of prep_state4 (1..BE_MAX_WINDOW) */
  int64_t env_offset;        /* global id of local env 0 (rank * N); keys the Philox streams */
  uint64_t seed;             /* Philox key for resets / obstacle moves / sampled actions */

  /* field and spawn strips, ballenv_env.py:11-18 */
  int32_t screen_width, screen_height;                 /* 500, 500 */
  int32_t strip_obs_x, strip_obs_y;                    /* 0, 20 */
  int32_t strip_goal_x, strip_goal_y;                  /* 500, 20 */
  int32_t strip_agent_x, strip_agent_y;                /* 500, 10 */

  /* BallEnv.__init__ constants, ballenv_env.py:49-65 */
  int32_t radius_obstacle;   /* radius_rand_person = 20 */
  int32_t radius_agent;      /* radius_ctrl_person = 5 */
  int32_t speed_x, speed_y;  /* speedx/y_ctrl_person = 1 (also the window cell step) */
  double threshold_goal;     /* 10 (strict <) */
  double time_penalty;       /* timepenalty = 0 */
  double min_spawn_dist;     /* reset re-sample distance, ballenv_env.py:122 (50) */

  /* customize_environment(args), ballenv_env.py:87-109 */
  int32_t num_static;        /* args.static_obstacles (13) */
  int32_t num_dynamic;       /* args.dynamic_obstacles (5) */
  double static_penalty;     /* args.static_penalty[1]  (threshold_2_penalty, 1) */
  double dynamic_penalty;    /* args.dynamic_penalty[1] (8000) */
  int32_t goal_change_step;  /* args.time_step_for_change (50) */
  int32_t obs_certainty;     /* args.rd_th_obs (60): P(directed move) in percent */
  int32_t num_goals;         /* len(args.obs_goal_position) */
  int32_t goals[BE_MAX_GOALS][2];
  int32_t obstacle_speed[BE_MAX_DYNAMIC];

  /* action table: index -> (dx, dy); default = move_list of ball_cnn_ac3.py:530 */
  int32_t num_actions;
  int32_t actions[BE_MAX_ACTIONS][2];

  int32_t time_limit;        /* gym TimeLimit max_episode_steps (1000); 0 = none */
  int32_t autoreset;         /* 1: a done env is reset inside be_step (vector-env semantics) */
} be_config;

/* Per-env state, all device pointers owned by the caller. */
typedef struct be_state {
  int32_t* agent;       /* (N)  int16x2 packed (x, y)            state[0]          */
  int32_t* goal;        /* (N)  int16x2 packed                    state[1]          */
  double* prev_dist;    /* (N)  f64                               state[2] / old_dist */
  double* total_dist;   /* (N)  f64                               total_distance    */
  double* ep_return;    /* (N)  f64                               total_reward_accumulated */
  int32_t* ep_len;      /* (N)  steps since reset (TimeLimit elapsed; also the obstacles' curr_counter phase) */
  uint32_t* episode;    /* (N)  resets so far; with ep_len it keys this env's Philox draws */
  int32_t* static_obs;  /* (Ns, N) int16x2 packed                 static_obstacle_list */
  int32_t* dyn_obs;     /* (Nd, N) int16x2 packed                 dynamic_obstacle_list */
  uint8_t* dyn_goal;    /* (Nd, N) index into goals               obstacle.curr_goal */
} be_state;

/* Step / observe outputs (device pointers; NULL = not requested). */
typedef struct be_out {
  uint8_t* obs;           /* (N, 4+W*W) u8 0/1: quadrant one-hot ++ W*W window */
  float* obs_f32;         /* (N, 4+W*W) f32 copy of the same (what prep_state4 returns) */
  double* reward;         /* (N) f64 (be_step only) */
  uint8_t* done;          /* (N) 0/1 (be_step only) */
  uint8_t* truncated;     /* (N) 0/1: done came from the time limit alone */
  uint8_t* terminal_obs;  /* (N, 4+W*W): obs of the terminal state, rows of done envs only (autoreset) */
  double* final_return;   /* (N): episode return, written for done envs only */
  int32_t* final_len;     /* (N): episode length, written for done envs only */
  double* stats;          /* (be_stats_slots(cfg), 8) f64 accumulators, one slot per 32 envs of the step
                             kernel (no atomics): [0]=episodes, [1]=sum return, [2]=sum return^2,
                             [3]=sum length, [4]=min return, [5]=max return, [6..7] unused; the caller
                             initialises [4]=+inf, [5]=-inf, the rest 0, and reduces over slots */
} be_out;

typedef struct be_ctx be_ctx;

/* ---- pure host functions (no GPU needed) ---- */
int be_abi_version(void);
/* Fill cfg with the ball_cnn_ac3.py / BallEnv defaults for N envs and window W. */
int be_config_default(be_config* cfg, int32_t num_envs, int32_t window);
/* Validate cfg; on failure returns BE_E_INVALID and writes a message into msg.
 * Besides the ranges, with autoreset and time_limit > 0 it requires
 *   max spawn extent + max|obstacle_speed| * time_limit <= 32767
 * (spawn extent: max(|strip_obs|, |screen - strip_obs|) per axis), so no dynamic obstacle can
 * leave the int16 coordinates within an episode (BE_STATUS_COORD_RANGE).                    */
int be_config_check(const be_config* cfg, char* msg, int32_t msg_len);
/* Bytes of HBM traffic per env-step the step kernel is designed to move (u8 obs). */
int64_t be_step_bytes(const be_config* cfg);
/* Number of 8-double slots the be_out.stats buffer must hold for this config. */
int64_t be_stats_slots(const be_config* cfg);
const char* be_last_error(const be_ctx* ctx);

/* Which kernel an entry point launches for this context (for profiles and bench lines: the
 * name matches rocprofv3's kernel name without the namespace/argument list), or NULL for a
 * bad ctx / entry.  No GPU work.  Diagnostics only; the reference has no counterpart. */
enum { BE_ENTRY_STEP_ACTIONS = 0,   /* be_step with caller action indices           */
       BE_ENTRY_STEP_SAMPLED = 1,   /* be_step with in-kernel sampled actions       */
       BE_ENTRY_ROLLOUT = 2,        /* be_rollout (NULL when it falls back to looping be_step) */
       BE_ENTRY_RESET = 3, BE_ENTRY_OBSERVE = 4 };
const char* be_kernel_name(const be_ctx* ctx, int32_t entry);
/* Which instance of its kernel the context's last be_step / be_step_n call launched: 0 none yet,
 * 1 the plain one, 2 step2_kernel's wide-row-load instance.  A state whose static_obs, dyn_obs and
 * dyn_goal are 16-byte aligned, in a batch that is a multiple of 32 envs, takes the faster
 * instance; anything else is still correct (bit for bit the same results) on the plain one.
 * BALLENV_STEP2_WIDE=0 / 1, read at be_create, forces either side where it is valid (A/B).
 * No GPU work.  Diagnostics only. */
int32_t be_step_instance(const be_ctx* ctx);

/* ---- device functions ---- */
int be_create(const be_config* cfg, int32_t device, be_ctx** out);
int be_destroy(be_ctx* ctx);

/* Reset envs (all, or those with mask[i] != 0) and write the obs of every env.
 * A reset env's episode counter is incremented first.
 * reset_tape == NULL: draws come from Philox(seed; global env id, new episode).
 * reset_tape != NULL: (tape_len, N) int16, the randint values the reference's
 * reset() would consume, in call order (parity mode).                           */
int be_reset(be_ctx* ctx, const be_state* st, const uint8_t* mask,
             const int16_t* reset_tape, int32_t tape_len, const be_out* out, void* stream);

/* One step of every env.
 * actions:       (N) u8 index into cfg.actions, or NULL to use action_deltas.
 * action_deltas: (N, 2) int16 raw (dx, dy) as BallEnv.step accepts, or NULL
 *                (both NULL: actions are sampled uniformly from Philox).
 * draw_tape:     (Nd, 2, N) int16: the move_obstacles randint values of this
 *                step per obstacle in call order (parity mode), or NULL (Philox). */
int be_step(be_ctx* ctx, const be_state* st, const uint8_t* actions, const int16_t* action_deltas,
            const int16_t* draw_tape, const be_out* out, void* stream);

/* `steps` consecutive be_step calls in one launch (a fused rollout), for an action tape.
 * actions: (steps, N) u8 indices into cfg.actions.  Outputs are per step: out->obs
 * (steps, N, 4+W*W) u8, out->reward (steps, N) f64, out->done / truncated (steps, N) u8,
 * out->final_return / final_len (steps, N) and out->terminal_obs (steps, N, 4+W*W) (rows of
 * reset envs only), or NULL; out->stats accumulates as for be_step.  out->obs_f32 must be
 * NULL; N*(4+W*W) must be a multiple of 16.
 * Results are bit-identical to `steps` be_step calls with actions + s*N (same state, same
 * Philox draws).  The reference has no batched counterpart: it is the caller's loop
 *   for t: state, reward, done, _ = env.step(move_list[a_t]); prep_state4(state)
 * (examples/ball_cnn_ac3.py:573-600 over ballenv_env.py:232-289), run for every env.
 * The default shape (13 static + 5 dynamic obstacles, W 5 or 10, unit moves) runs one kernel
 * that keeps each env's state in registers; other configs loop be_step.             */
int be_rollout(be_ctx* ctx, const be_state* st, const uint8_t* actions, int32_t steps, const be_out* out,
               void* stream);

/* `steps` be_step launches (one kernel per step, caller actions + s*N) queued from a host loop
 * in the library, with the same `out` every step: out holds the last step's outputs (and
 * stats accumulate) exactly as after `steps` be_step calls.  The reference's counterpart is
 * the caller's per-step loop (examples/ball_cnn_ac3.py:573-600): this is that loop for every
 * env, minus the per-call Python overhead.                                             */
int be_step_n(be_ctx* ctx, const be_state* st, const uint8_t* actions, int32_t steps, const be_out* out,
              void* stream);

/* prep_state4 of the current state of every env (no state change). */
int be_observe(be_ctx* ctx, const be_state* st, const be_out* out, void* stream);

/* Fill actions_out (steps, N) u8 with uniform action indices from Philox keyed
 * by (seed, global env id): identical per global env at any GPU count.         */
int be_sample_actions(be_ctx* ctx, uint8_t* actions_out, int32_t steps, uint64_t seed, void* stream);

/* Synchronise the stream and read (then clear) the device status word. */
int be_status(be_ctx* ctx, int32_t* status_out, void* stream);

/* ---- env-state checkpoint (SURVEY 8(b) be_save_state / be_load_state; the reference keeps no
 * env checkpoint, only torch.save of the policy, examples/ball_cnn_ac3.py:637-639) ----
 * The be_state arrays of every env packed into ONE contiguous blob of be_state_blob_bytes(cfg)
 * bytes, in device or host memory: a 64-byte header (magic "BALLENV1", ABI version, N, Ns, Nd,
 * blob bytes) then agent, goal, prev_dist, total_dist, ep_return, ep_len, episode, static_obs,
 * dyn_obs, dyn_goal in be_state order, each array at a 16-byte aligned offset.
 * be_save_state: asynchronous copies on the stream (graph-capturable).  be_load_state:
 * SYNCHRONISES the stream to read and check the header (BE_E_INVALID when it does not match this
 * context's N / Ns / Nd), then copies asynchronously -- it cannot be captured in a HIP graph.  A saved blob restores the envs bit for bit, Philox positions included
 * (episode / ep_len key every draw).                                                        */
int64_t be_state_blob_bytes(const be_config* cfg);
int be_save_state(be_ctx* ctx, const be_state* st, void* blob, void* stream);
int be_load_state(be_ctx* ctx, const be_state* st, const void* blob, void* stream);

/* ---- the autoreset pool (a cache inside the context; no reference counterpart) ----
 * In Philox mode BallEnv.reset (ballenv_env.py:113-167) of env i into episode e is a pure
 * function of (seed, global id, e) and the config.  When be_step's kernel is a fixed-shape one
 * that consumes it (step2_kernel at W=10, stepw_kernel at W=5, and the one-lane kernel up to
 * 128 x 4 x CUs envs -- two waves per SIMD; past that its waves hide the draws and the pool
 * measured slower -- all at the reference's 13 + 5 obstacles), the context holds, per env, the precomputed resets into episodes e+1 and e+2 (ep = the env's
 * episode); a finishing env copies its entry instead of drawing the reset on the step's critical
 * path, and draws it inline as before when the entry is stale.  Results are bit-identical either
 * way -- the pool changes timing only.  be_reset and be_load_state fill it after their own work,
 * and be_step queues a fill every `period` step launches (default 128; BALLENV_POOL_PERIOD, and
 * BALLENV_POOL=0 disables the pool, for A/B runs).  The pool serves one state: the one last
 * reset, loaded or filled for (or the first stepped); steps of any other state draw every reset
 * inline.  The library does not order the pool's launches itself: the caller must order, on one
 * stream (or with events), every launch that uses a context's pool -- the owner's steps, resets,
 * loads and fills, and across a change of owner the previous owner's launches before the new
 * owner's reset / load / fill.  Two states of one context driven from unordered streams must not
 * trade ownership (keep one owner, or disable the pool).
 * be_pool_fill: fill now (every env's stale entries) and make st the pool's state.
 * be_pool_invalidate: mark every entry unwritten (async on the stream): the inline path until the
 * next fill.  be_pool_set_period / be_pool_period: step launches per fill (0: only the explicit ones).
 * be_pool_bytes: the pool's device bytes (0: this context has no pool). */
int be_pool_fill(be_ctx* ctx, const be_state* st, void* stream);
int be_pool_invalidate(be_ctx* ctx, void* stream);
int be_pool_set_period(be_ctx* ctx, int32_t period);
int32_t be_pool_period(const be_ctx* ctx);
int64_t be_pool_bytes(const be_ctx* ctx);
/* Test hook (synchronous; device-wide sync first): read (write = 0) or overwrite (write = 1) env's
 * entry in slot (0 / 1: the slot of episode x is x & 1).  words: TAG, AGENT, GOAL, ROWS0..2, then
 * the NS + ND obstacles' packed xy (6 + 13 + 5 words); f64: PREV, TOTAL.  ROWS0 bit 30 marks a
 * written entry, bit 31 a rejection-limit hit (layout: csrc/pool_layout.h). */
int be_pool_entry(be_ctx* ctx, int32_t env, int32_t slot, uint32_t* words, double* f64, int32_t write);

/* ---- on-GPU select_action for batched rollouts (BASELINE config 5) ----
 * Replaces, for every env at once, the caller's per-step
 *   probs, value = Policy(W)(prep_state4(state))      examples/ball_cnn_ac3.py:109-146
 *   action ~ Categorical(probs); saved log_prob, value  ball_cnn_ac3.py:210-220
 * (the reference runs it per single env with a host round trip per step,
 * ball_cnn_ac3.py:573-600).  fc1 runs on the int8 matrix cores against a
 * 24-bit fixed-point image of the fp32 weights (see csrc/policy.hip); the heads,
 * softmax and log_prob are fp32.  The draw is an inverse-CDF of a Philox uniform
 * keyed by (seed; global env id, episode, ep_len), so it is reproducible and
 * independent of GPU count and graph replay.                                     */
typedef struct be_policy be_policy;

typedef struct be_act_out {
  uint8_t* action;   /* (N) u8 sampled action index (feeds be_step's actions) */
  float* log_prob;   /* (N) f32 log probs[action], or NULL */
  float* value;      /* (N) f32 value_head output, or NULL */
  float* probs;      /* (N, A) f32 softmax probabilities, or NULL */
} be_act_out;

/* A policy for ctx's window (inputs 4+W*W <= 128), hidden <= 256, actions <= 15. */
int be_policy_create(be_ctx* ctx, int32_t hidden, int32_t num_actions, be_policy** out);
int be_policy_destroy(be_policy* pol);
/* (Re)load weights from DEVICE f32 arrays in torch state_dict layout:
 * fc1_w (H, 4+W*W), fc1_b (H), act_w (A, H), act_b (A), val_w (1, H), val_b (1).
 * Asynchronous on stream (one packing kernel); graph-capturable.                  */
int be_policy_load(be_policy* pol, const float* fc1_w, const float* fc1_b, const float* act_w, const float* act_b,
                   const float* val_w, const float* val_b, void* stream);
/* Policy forward + draw for every env from obs (N, 4+W*W) u8; st supplies episode/ep_len (Philox key). */
int be_policy_act(be_policy* pol, const be_state* st, const uint8_t* obs, const be_act_out* out, uint64_t seed,
                  void* stream);

/* `steps` config-5 steps in one launch: for s in 0..steps-1
 *   act[s] = select_action(obs_s) (as be_policy_act, same Philox draw);  be_step(act[s]) -> obs_{s+1}
 * obs_in: (N, F) obs of the current state (obs_0, e.g. the env's obs buffer).  out: per-step
 * (steps, N, ...) outputs as for be_rollout; out->obs (steps, N, F) records obs_1..obs_steps or is
 * NULL; obs_last (N, F) receives obs_steps (may equal obs_in) or is NULL; one of the two is
 * required.  act: (steps, N) action / log_prob / value (probs must be NULL).  N*F % 16 == 0.
 * Bit-identical to the be_policy_act + be_step loop (ball_cnn_ac3.py:573-600 for every env).
 * The default env shape with the Policy(10) / Policy(5) shapes runs one kernel with the packed
 * weights in LDS and each env's state in registers; other shapes run that loop.          */
int be_policy_rollout(be_policy* pol, const be_state* st, const uint8_t* obs_in, uint8_t* obs_last, int32_t steps,
                      const be_out* out, const be_act_out* act, uint64_t seed, void* stream);
/* Bytes of the packed weight image (staged once per workgroup in LDS). */
int64_t be_policy_bytes(const be_policy* pol);

/* ---- sibling observation formats (the reference's other callers) ----
 * prep_state2 of examples/ball_env_reinforce.py:130-172 for every env's current state:
 * (N, 29) block counts -- quadrant one-hot, [16] = 1 (the agent's cell), +1 per obstacle
 * in its 20-px block of the 5x5 grid -- as u8 (out) and/or f32 (out_f32; NULL = skip). */
int be_observe_blocks(be_ctx* ctx, const be_state* st, uint8_t* out, float* out_f32, void* stream);

/* extract_patch of examples/ball_cnn_reinforce.py:120-163 for every env's current state (no state
 * change): the frame BallEnv.render draws (gym_ballenv/envs/ballenv_env.py:357-386: agent disk and
 * goal fan black, static disks red, dynamic disks green, on white), padded with white, cut to the
 * 100 x 100 patch centred on the agent and resized to 40 x 40 with PIL's bicubic filter.
 *   patch    (N, 100, 100, 3) u8, HWC, top row first: cell (i, j) is world pixel
 *            x = ax - 50 + j, y = ay + 49 - i; white outside the screen
 *   out      (N, 3, 40, 40) u8, CHW: Image.fromarray(patch).resize((40, 40), Image.BICUBIC), byte
 *            for byte (a horizontal pass into a u8 intermediate, then a vertical one; 22-bit
 *            fixed-point coefficients, be_pixels_coeffs)
 *   out_f32  (N, 3, 40, 40) f32: ToTensor's out / 255 (f32 division)
 * Any subset: a NULL pointer skips that output, all three NULL is BE_E_INVALID.  Every pointer is
 * 16-byte aligned.  The reference then passes the HWC tensor through ToPILImage, which reads it
 * as CHW; that quirk is not reproduced.  One launch, no allocation: capturable. */
int be_observe_pixels(be_ctx* ctx, const be_state* st, uint8_t* patch, uint8_t* out, float* out_f32, void* stream);
/* The resize's coefficients, 100 -> 40 (PIL's precompute_coeffs + normalize_coeffs_8bpc): kk
 * (40, 10) i32, zero behind a row's taps; bounds (40, 2) i32, first input index and tap count.
 * Pure host code, no device. */
int be_pixels_coeffs(int32_t* kk, int32_t* bounds);

/* ---- on-GPU select_action of the REINFORCE / supervised agents (the block-count MLP) ----
 * Replaces, for every env at once, the caller's per-step
 *   probs = Policy()(prep_state2(state))                examples/ball_env_reinforce.py:57-73, 130-172
 *   action ~ Categorical(probs); saved log_prob          ball_env_reinforce.py:76-85
 * (also examples/test_model.py:57-85, and the Model of examples/train_supervise.py:11-26, whose
 * last layer has no relu).  The network: affine1 (29 -> hidden1), relu, [affine2 (hidden1 ->
 * hidden2), relu,] last layer (-> num_actions), [relu,] softmax.  It has no value head.
 * The arithmetic is pinned (csrc/mlp_policy.hip has the operand order of the fma chains):
 *   x      = the 29 u8 counts as f32 (exact: a count is at most 19 in the default config)
 *   h1     = relu(W1 x + b1);   3 layers: h2 = relu(W2 h1 + b2)
 *   z      = W_last h + b_last;  z = relu(z) iff final_relu
 *   p      = softmax(z), max-subtracted, as be_policy_act's
 *   a      = #{j : cdf_j <= u}, clamped to the last action with p > 0;  log_prob = log p[a]
 *   u      = the uniform be_policy_act draws: Philox(seed; global env id, episode, ep_len, POLICY)
 * Every product is an f32 fma chain on v_mfma_f32_16x16x4_f32 that starts at the bias.
 * layers 2 | 3; hidden1, hidden2 in [1, 128] (hidden2 = 0 with 2 layers); num_actions in [1, 15]. */
typedef struct be_mlp be_mlp;
int be_mlp_create(be_ctx* ctx, int32_t layers, int32_t hidden1, int32_t hidden2, int32_t num_actions,
                  int32_t final_relu, be_mlp** out);
int be_mlp_destroy(be_mlp* mlp);
/* (Re)load weights from DEVICE f32 arrays in torch state_dict layout: w1 (hidden1, 29), b1 (hidden1);
 * 3 layers: w2 (hidden2, hidden1), b2, w3 (A, hidden2), b3 (A); 2 layers: w2 (A, hidden1), b2 (A),
 * w3 = b3 = NULL.  One packing kernel into the padded image be_mlp_act stages (K 29 -> 32, hidden
 * -> 128, actions -> 16; pad rows and columns are zero).  Asynchronous on stream, graph-capturable,
 * allocates nothing.                                                                            */
int be_mlp_load(be_mlp* mlp, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                const float* b3, void* stream);
/* select_action for every env of st.  blocks_in NULL: the input is prep_state2 of each env's current
 * state, computed in the kernel (the rows be_observe_blocks writes); else the caller's (N, 29) u8 rows.
 * blocks_out, if given, receives the (N, 29) rows be_observe_blocks would write for st.
 * out->action is required, out->log_prob and out->probs (N, A) are optional, out->value must be
 * NULL (BE_E_INVALID).  One launch, asynchronous on stream, graph-capturable.                    */
int be_mlp_act(be_mlp* mlp, const be_state* st, const uint8_t* blocks_in, uint8_t* blocks_out, const be_act_out* out,
               uint64_t seed, void* stream);
/* `steps` steps of the REINFORCE agent's episode loop (examples/ball_env_reinforce.py:309-336: prep_state2,
 * select_action, env.step, the reward appended) for every env in one launch: for s in 0..steps-1
 *   act[s] = be_mlp_act(state) (the same pinned arithmetic, the same Philox draw);  be_step(act[s])
 * act: (steps, N) action (required) and log_prob (optional); act->value and act->probs must be NULL.
 * blocks_out (steps, N, 29) u8 or NULL: row s holds the counts action s was drawn from.  out: per-step
 * (steps, N) outputs as for be_rollout -- reward and done required, truncated / final_return / final_len
 * optional, stats accumulates as for be_step; out->obs, obs_f32 and terminal_obs must be NULL (this
 * agent reads no window rows; a caller who wants them per step runs the loop).  obs_last (N, 4+W*W),
 * required and 16-byte aligned, receives the window obs of the final state: what the loop's last
 * be_step writes.  steps == 0: BE_OK, no launch.  A handle never loaded and never stepped by be_mlp_opt
 * is rejected, as by be_mlp_act.  Bit-identical to the be_mlp_act + be_step loop in everything it
 * leaves (the outputs, the whole be_state, the stats slots, the status word, obs_last).
 * The fixed env shape (13 + 5 obstacles, unit moves, distinct goals, action indices, Philox mode) runs
 * one kernel with the packed weights in LDS and each env's state in registers, then the observe
 * kernel; other shapes run that loop.  Asynchronous on stream, graph-capturable, allocates nothing. */
int be_mlp_rollout(be_mlp* mlp, const be_state* st, uint8_t* obs_last, uint8_t* blocks_out, int32_t steps,
                   const be_out* out, const be_act_out* act, uint64_t seed, void* stream);
/* The fused kernel's instance name for this handle (the calling thread's buffer, valid until its next
 * call), or NULL when be_mlp_rollout runs the loop.  BALLENV_MLP_ROLLOUT_WAVES = 0 | 1 | 2 | 4 | 8, read at
 * be_mlp_create, forces the loop or one instance (A/B runs).                                       */
const char* be_mlp_rollout_kernel(const be_mlp* mlp);
/* Bytes of the packed weight image (staged once per workgroup in LDS). */
int64_t be_mlp_bytes(const be_mlp* mlp);

/* ---- on-GPU select_action of the pixel agent (the conv net of examples/ball_cnn_reinforce.py) ----
 * Replaces, for every env at once, the caller's per-step
 *   probs = Policy()(extract_patch(state), quadrant)     examples/ball_cnn_reinforce.py:60-83
 *   action ~ Categorical(probs); saved log_prob           ball_cnn_reinforce.py:85-95
 * The network: conv1 (3 -> 16), conv2 (16 -> 32), conv3 (32 -> 32), each 5 x 5 stride 2 with
 * BatchNorm and relu (maps 18 x 18, 7 x 7, 2 x 2), then head: Linear(132, num_actions) on the 128
 * features (channel-major) and the goal's quadrant one-hot, softmax.  It has no value head.
 * The reference never calls eval() and feeds one image at a time, so each BatchNorm normalises with the
 * statistics of that env's own feature map: BE_CNN_NORM_SAMPLE.  BE_CNN_NORM_RUNNING uses the stored
 * running statistics (Policy.eval()).
 * The arithmetic is pinned (csrc/cnn_policy.hip and csrc/cnn_host.h have the k order of the chains):
 *   x      = (float)v / 255.0f per image byte, one IEEE division: be_observe_pixels' out_f32 values
 *   conv   = bias + sum w x: f32 fma chains on v_mfma_f32_16x16x4_f32, the bias in the chain's start.
 *            conv1: one chain of 19 steps of 4 (ci, ky ascending with kx = 0..3 in a step, then the kx = 4
 *            column; K 75 -> 76 with a zero weight).  conv2: one chain of 100 steps, step 25 cg + tap
 *            taking the input channels 4 cg .. 4 cg + 3 at tap (ky, kx) = (tap / 5, tap % 5).  conv3: eight
 *            chains, chain c the 25 steps of the channels 4 c .. 4 c + 3 in that tap order, chain 0
 *            starting at the bias, conv = ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7))
 *   SAMPLE   mean = (sum conv) / n, var = (sum (conv - mean)^2) / n, n = 324, 49, 4: two passes, biased.
 *            A sum runs over P = 8, 4, 4 interleaved partial sums (partial j takes the positions j, j + P,
 *            ... in order, from 0.0f), combined pairwise: ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)),
 *            so four equal values have exactly their value as their mean.
 *            No atomics: an env's statistics are the same bits wherever it runs
 *   RUNNING  mean and var are the stored running_mean and running_var
 *   y      = relu(((conv - mean) * (1.0f / sqrtf(var + 1e-5f))) * gamma + beta): IEEE sqrt and
 *            division, no fused multiply-add
 *   z      = head [flatten(y3), one_hot(quadrant)] + b: four chains, chain s & 3 taking step s (the
 *            inputs 4 s .. 4 s + 3) for s < 32, the one-hot's step on chain 0, chain 0 starting at
 *            the bias, z = (c0 + c1) + (c2 + c3)
 *   p, a, log_prob, u: as be_mlp_act's (max-subtracted softmax, the inverse-CDF draw on the Philox
 *            uniform keyed by (seed; global env id, episode, ep_len, POLICY))
 * An env's outputs depend on its image, quadrant, episode counters and the seed only: not on N, the
 * workgroup or round that takes it, or whether the launch was captured.                          */
typedef struct be_cnn be_cnn;
#define BE_CNN_NORM_SAMPLE 0
#define BE_CNN_NORM_RUNNING 1
typedef struct be_cnn_weights {     /* DEVICE f32 arrays in torch state_dict layout                 */
  const float *conv1_weight, *conv1_bias;                                   /* (16, 3, 5, 5), (16)  */
  const float *bn1_weight, *bn1_bias, *bn1_running_mean, *bn1_running_var;  /* (16) each            */
  const float *conv2_weight, *conv2_bias;                                   /* (32, 16, 5, 5), (32) */
  const float *bn2_weight, *bn2_bias, *bn2_running_mean, *bn2_running_var;  /* (32) each            */
  const float *conv3_weight, *conv3_bias;                                   /* (32, 32, 5, 5), (32) */
  const float *bn3_weight, *bn3_bias, *bn3_running_mean, *bn3_running_var;  /* (32) each            */
  const float *head_weight, *head_bias;                                     /* (A, 132), (A)        */
} be_cnn_weights;
/* num_actions in [1, 15]. */
int be_cnn_create(be_ctx* ctx, int32_t num_actions, be_cnn** out);
int be_cnn_destroy(be_cnn* cnn);
/* (Re)load the weights: one packing kernel into the image be_cnn_act reads (MFMA A fragments, K padded
 * with zero weights, head rows padded to 16).  Every pointer is required and 4-byte aligned.
 * Asynchronous on stream, graph-capturable, allocates nothing.                                    */
int be_cnn_load(be_cnn* cnn, const be_cnn_weights* w, void* stream);
/* select_action for every env of st.  image: the (N, 3, 40, 40) u8 image be_observe_pixels writes
 * (required, 16-byte aligned).  quadrant_in NULL: the goal's quadrant is computed from st in the kernel
 * (prep_state2's rule, be_observe_blocks' first four bytes); else N bytes in 0..3.  norm: BE_CNN_NORM_*.
 * out->action is required, out->log_prob and out->probs (N, A) are optional, out->value must be NULL.
 * A failed check is BE_E_INVALID with the argument named in be_last_error, and launches nothing; a
 * handle never loaded is rejected.  st is not changed.  One launch, asynchronous on stream,
 * graph-capturable, allocates nothing.                                                            */
int be_cnn_act(be_cnn* cnn, const be_state* st, const uint8_t* image, const uint8_t* quadrant_in, int32_t norm,
               const be_act_out* out, uint64_t seed, void* stream);
/* Bytes of the packed weight image. */
int64_t be_cnn_bytes(const be_cnn* cnn);

/* ---- the pixel agent's loss and gradients: finish_episode of examples/ball_cnn_reinforce.py:98-117 ----
 * The REINFORCE loss of the network above over `rows` recorded rows (every row offset is 64-bit) and its
 * gradients, i.e. what loss.backward() leaves in each .grad; be_mlp_grad's contract (below) for this
 * network.  Contiguous device arrays: images (rows, 3, 40, 40) u8, 16-byte aligned; quadrants (rows) u8 in
 * 0..3; actions (rows) u8; coef (rows) f32 or NULL (= 1); valid (rows) u8 or NULL (= every row).  The
 * BatchNorm mode is BE_CNN_NORM_SAMPLE, the only one the reference trains in: weights' running statistics
 * are not read and may be NULL.  A row is active when it is valid and action < num_actions; any other row
 * adds exactly +0.  Per row, in f32 (a = its action, c = its coef, eps = FLT_EPSILON):
 *   forward  be_cnn_act's pinned arithmetic above: grads->probs of a row, if given, are bit for bit the
 *            probs be_cnn_act writes for that image and quadrant
 *   loss     += -c * log(min(max(p_a, eps), 1 - eps))          (Categorical(probs).log_prob's clamp)
 *   dz_j     = c * (p_j - [j == a]) if eps <= p_a <= 1 - eps, else 0; p_a - 1 is taken as -(sum of the
 *            other p_j, added in action order): the same number without the cancellation where p_a is near 1
 *   head     gW_head += dz (x) [flatten(y3), one_hot(quadrant)];  gb_head += dz;  dy3 = W_head[:, :128]^T dz
 *   each BatchNorm layer, per map of n = 4, 49, 324 positions, xhat = (conv - mean) * inv:
 *            dyr = (xhat * gamma + beta > 0) ? dy : 0   (the forward's own expression: the same mask)
 *            gbeta += sum dyr;  ggamma += sum dyr * xhat   (the sums as the forward's statistics:
 *            interleaved partials combined pairwise)
 *            dconv = (gamma * inv) * ((dyr - (sum dyr) / n) - xhat * ((sum dyr * xhat) / n))
 *   each convolution:  gW[co][ci][ky][kx] += sum_pos dconv[co][pos] * in[ci][2 oy + ky][2 ox + kx];
 *            din = the matching transposed convolution (none for the image)
 *   conv1..3_bias: the per-map mean subtracts the bias, so its gradient is zero: written as exact +0
 * Every product with more than a handful of terms is an f32 fma chain on v_mfma_f32_16x16x4_f32
 * (csrc/cnn_grad.hip has the operand and chain order).  No float atomics: each workgroup of a grid that
 * depends only on rows and the device adds its rows in a fixed order and writes its sums to `workspace`; a
 * last kernel adds the workgroups' sums in workgroup order in f64, multiplies by `scale` in f64 and rounds
 * once to f32.  losses[0] is scale * the f64 sum of the row losses, losses[1] the number of active rows.
 * Two calls on the same inputs and device give the same bits whatever the workspace held, and a row's
 * contribution does not depend on its place among the rows.  Every output element is written on every call
 * (zeros when no row is active; rows = 0 is valid).  Asynchronous on `stream`, no allocation and no
 * synchronisation (graph-capturable).  BE_E_INVALID, with the argument named in be_last_error and nothing
 * launched: a NULL ctx or required pointer, a misaligned images, num_actions outside [1, 15], rows < 0, a
 * workspace that is too small (or not 16-byte aligned).                                          */
typedef struct be_cnn_grads {       /* what loss.backward() leaves in each .grad; state_dict shapes */
  float *conv1_weight, *conv1_bias, *bn1_weight, *bn1_bias,
        *conv2_weight, *conv2_bias, *bn2_weight, *bn2_bias,
        *conv3_weight, *conv3_bias, *bn3_weight, *bn3_bias, *head_weight, *head_bias;
  double* losses;                   /* [2]: scale * f64 sum of the row losses, number of active rows */
  float*  probs;                    /* optional (rows, A): the forward's probabilities               */
} be_cnn_grads;
/* Bytes of workspace be_cnn_grad needs on ctx's device (16-byte aligned; independent of rows);
 * < 0: an error code.                                                                       */
int64_t be_cnn_grad_workspace_bytes(be_ctx* ctx, int32_t num_actions);
int be_cnn_grad(be_ctx* ctx, const uint8_t* images, const uint8_t* quadrants, const uint8_t* actions,
                const float* coef, const uint8_t* valid, int64_t rows, double scale,
                const be_cnn_weights* weights, int32_t num_actions,
                void* workspace, int64_t workspace_bytes, const be_cnn_grads* grads, void* stream);
/* The goal's quadrant of every env of st, out (N) u8 in 0..3: prep_state2's rule, the index of the one set
 * byte among be_observe_blocks' first four -- what be_cnn_act computes itself when quadrant_in is NULL.
 * One launch, asynchronous on stream, graph-capturable.                                            */
int be_observe_quadrant(be_ctx* ctx, const be_state* st, uint8_t* out, void* stream);

/* ---- the pixel agent's optimiser step and re-pack: optimizer.step() of examples/ball_cnn_reinforce.py ----
 *   finish_episode       examples/ball_cnn_reinforce.py:115, :244   optim.Adam(policy.parameters(), lr=1e-3)
 * One Adam step on the network's 14 parameters in place, and `cnn`'s packed image rebuilt from the new
 * weights: afterwards the image holds exactly the bytes be_cnn_load would build from them and the running
 * statistics that were last loaded, so be_cnn_act runs the updated network.  cnn's num_actions defines
 * every shape (be_cnn_load's).  be_mlp_opt's contract (below) for this network, with one difference: the six
 * running-statistics vectors are no parameters, so the step does not touch them -- their image rows and
 * the image's pad and -inf entries keep what the last be_cnn_load wrote -- and a cnn that was never loaded
 * is rejected.  (The reference's train-mode forward also updates running_mean / running_var, which it
 * never reads: policy.eval() is never called.  Maintaining them is not part of this entry.)
 * All tensors are contiguous f32 device arrays in state_dict layout: params (updated), grads (read: what
 * be_cnn_grad writes), exp_avg and exp_avg_sq (updated; zeros for a fresh optimiser).
 * state: 4 f64 on the device, [t, beta1^t, beta2^t, lr], as be_mlp_opt's; a fresh optimiser holds
 * [0, 1, 1, lr].  The arithmetic is BE_MLP_OPT_ADAM's, pinned below: every operation one f64 operation, no
 * FMA.  Every element is computed from the state as it was before the call; the state advances exactly
 * once per call, after all of them.  be_cnn_grad's conv*_bias gradients are exact +0: with eps > 0 the
 * pinned arithmetic then leaves those weights and their moments bit-unchanged (m' = v' = 0,
 * w' = w - ss * (0 / eps)); with eps = 0 it is 0 / 0.  They are not treated specially.
 * losses / loss_log: both NULL, or losses = the 2 f64 of be_cnn_grads.losses and loss_log a
 * (log_rows, 2) f64 device array, log_rows >= 1: row (t mod log_rows) receives a copy of losses, t
 * being the state's step count before the call -- a replayed graph logs every iteration's losses.
 * Asynchronous on `stream`, no allocation and no synchronisation (graph-capturable as a linear
 * chain); two launches: the update + pack kernel, the state kernel.
 * BE_E_INVALID, with nothing launched: a NULL cnn; a cnn never loaded ("be_cnn_adam before be_cnn_load");
 * a NULL set; a NULL or not 4-byte aligned tensor, named in the message ("grads->conv2_weight"); state
 * NULL or not 8-byte aligned; a beta outside [0, 1) or eps < 0; losses and loss_log not both or neither,
 * or not 8-byte aligned; log_rows < 1 with a log.                                                   */
typedef struct be_cnn_tensors {     /* f32 device arrays, state_dict shapes: the 14 parameters in be_cnn_grads' order */
  float *conv1_weight, *conv1_bias, *bn1_weight, *bn1_bias, *conv2_weight, *conv2_bias, *bn2_weight, *bn2_bias,
        *conv3_weight, *conv3_bias, *bn3_weight, *bn3_bias, *head_weight, *head_bias;
} be_cnn_tensors;
int be_cnn_adam(be_cnn* cnn, const be_cnn_tensors* params, const be_cnn_tensors* grads,
                const be_cnn_tensors* exp_avg, const be_cnn_tensors* exp_avg_sq, double* state,
                double beta1, double beta2, double eps,
                const double* losses, double* loss_log, int32_t log_rows, void* stream);

/* ---- the block-count MLP's losses and gradients: both of the reference's training loops ----
 *   finish_episode       examples/ball_env_reinforce.py:88-108  sum of -Categorical(probs).log_prob(a) * R^
 *   the supervised loop  examples/train_supervise.py:66-101     mean CrossEntropyLoss on the logits
 * The loss of the network above over `rows` recorded rows (every row offset is 64-bit) and its
 * gradients, i.e. what loss.backward() leaves in each .grad.  Contiguous device arrays: blocks
 * (rows, 29) u8, actions (rows) u8 (the labels with BE_MLP_LOSS_XENT), coef (rows) f32 or NULL (= 1),
 * valid (rows) u8 or NULL (= every row).  A row is active when it is valid and action < num_actions;
 * any other row adds exactly +0.  Per active row, in f32 (a = its action, c = its coef,
 * eps = FLT_EPSILON):
 *   x = the 29 counts as f32;  pre1 = W1 x + b1;  h1 = max(pre1, 0)
 *   3 layers: pre2 = W2 h1 + b2;  h2 = max(pre2, 0)
 *   zp = W_last h + b_last;  z = final_relu ? max(zp, 0) : zp
 *   m = max z;  e_j = exp(z_j - m);  S = sum e_j;  p_j = e_j / S
 *   BE_MLP_LOSS_REINFORCE (Categorical(probs).log_prob: the probabilities clamped to [eps, 1 - eps]):
 *     loss += -c * log(min(max(p_a, eps), 1 - eps))
 *     dz_j = c * (p_j - [j == a]) if eps <= p_a <= 1 - eps, else 0   (the clamp passes no gradient outside
 *     its bounds; Categorical's p / sum p has no gradient of its own and is left out)
 *   BE_MLP_LOSS_XENT (CrossEntropyLoss on z):
 *     loss += -c * (z_a - m - log S);   dz_j = c * (p_j - [j == a])
 *   dzp_j = (final_relu && zp_j <= 0) ? 0 : dz_j
 *   gW_last += dzp (x) h;  gb_last += dzp;  dh = W_last^T dzp;  dpre = pre > 0 ? dh : 0   (each hidden layer)
 *   3 layers: gW2 += dpre2 (x) h1;  gb2 += dpre2;  dh1 = W2^T dpre2
 *   gW1 += dpre1 (x) x;  gb1 += dpre1
 * Every product is an f32 fma chain on v_mfma_f32_16x16x4_f32 (csrc/mlp_grad.hip has the operand order).
 * No float atomics: each workgroup of a grid that depends only on rows and the device adds its
 * rows in a fixed order and writes its sums to `workspace`; a second kernel adds the workgroups'
 * sums in workgroup order in f64, multiplies by `scale` in f64 and rounds once to f32.  losses[0] is
 * scale * the f64 sum of the row losses, losses[1] the number of active rows.  scale: 1 / batch for the
 * supervised mean; 1 for REINFORCE with coef = returns_norm.  Two calls on the same inputs and
 * device give the same bits whatever the workspace held.  Every output element is written on every
 * call (zeros when no row is active; rows = 0 is valid).  Asynchronous on `stream`, no allocation
 * and no synchronisation (graph-capturable).  BE_E_INVALID, with nothing launched: a NULL ctx or
 * required pointer, a shape outside be_mlp_create's bounds, w3 / b3 not matching layers, an unknown
 * loss, a workspace that is too small.                                                        */
typedef struct be_mlp_weights {     /* state_dict layout, as be_mlp_load takes them, and the shape */
  const float *w1, *b1, *w2, *b2, *w3, *b3;          /* 2 layers: w3 = b3 = NULL                     */
  int32_t layers, hidden1, hidden2, num_actions, final_relu;   /* be_mlp_create's bounds            */
} be_mlp_weights;
typedef struct be_mlp_grads {       /* the same shapes: what loss.backward() leaves in each .grad  */
  float *w1, *b1, *w2, *b2, *w3, *b3;                /* 2 layers: w3 = b3 = NULL                     */
  double* losses;                   /* [2]: scale * sum of row losses, number of active rows       */
} be_mlp_grads;
#define BE_MLP_LOSS_REINFORCE 0
#define BE_MLP_LOSS_XENT      1
/* Bytes of workspace be_mlp_grad needs on ctx's device (8-byte aligned; independent of rows);
 * < 0: an error code.                                                                       */
int64_t be_mlp_grad_workspace_bytes(be_ctx* ctx, int32_t layers, int32_t hidden1, int32_t hidden2, int32_t num_actions);
int be_mlp_grad(be_ctx* ctx, const uint8_t* blocks, const uint8_t* actions, const float* coef, const uint8_t* valid,
                int64_t rows, int32_t loss, double scale, const be_mlp_weights* weights,
                void* workspace, int64_t workspace_bytes, const be_mlp_grads* grads, void* stream);

/* ---- the block-count MLP's optimiser step and re-pack: optimizer.step() of both training loops ----
 *   REINFORCE            examples/ball_env_reinforce.py:196, :105  optim.Adam(lr=1e-2)
 *   the supervised loop  examples/train_supervise.py:75, :101      torch.optim.SGD(lr=1e-2)
 * One optimiser step on the network's four (2 layers) or six tensors in place, and `mlp`'s packed
 * image rebuilt from the new weights: afterwards the image holds exactly the bytes be_mlp_load would
 * build from them, so be_mlp_act runs the updated network, and mlp counts as loaded.  mlp's layers,
 * hidden1, hidden2 and num_actions define every shape (be_mlp_load's); an mlp that was never loaded is
 * accepted (the step defines the whole image).
 * All tensors are contiguous f32 device arrays in state_dict layout: params (updated), grads (read:
 * what be_mlp_grad writes), and for BE_MLP_OPT_ADAM exp_avg and exp_avg_sq (updated; zeros for a
 * fresh optimiser); BE_MLP_OPT_SGD takes exp_avg = exp_avg_sq = NULL.
 * state: 4 f64 on the device, [t, beta1^t, beta2^t, lr], as be_a2c_adam's; a fresh optimiser holds
 * [0, 1, 1, lr].  The learning rate lives on the device so that a captured graph follows a change of it.
 * The arithmetic is pinned; every operation is one f64 operation, no FMA:
 *   BE_MLP_OPT_ADAM (torch.optim.Adam with weight_decay = 0, amsgrad = False, maximize = False), the
 *   arithmetic of be_a2c_adam:
 *     t' = t + 1;  p1' = p1 * beta1;  p2' = p2 * beta2       (state after the call: [t', p1', p2', lr])
 *     bc1 = 1 - p1';  bc2s = sqrt(1 - p2');  ss = lr / bc1
 *     per element:  g = (double)grad
 *       m' = (float)(beta1 * (double)m + (1 - beta1) * g)
 *       v' = (float)(beta2 * (double)v + ((1 - beta2) * g) * g)
 *       w' = (float)((double)w - ss * ((double)m' / (sqrt((double)v') / bc2s + eps)))
 *   BE_MLP_OPT_SGD (torch.optim.SGD with momentum = 0, weight_decay = 0, nesterov = False):
 *     per element:  w' = (float)((double)w - lr * (double)grad)
 *     the state after the call: [t + 1, p1, p2, lr]; beta1, beta2 and eps are ignored
 * Every element is computed from the state as it was before the call; the state advances exactly
 * once per call, after all of them (a one-thread kernel behind the update kernel on `stream`).
 * losses / loss_log: both NULL, or losses = the 2 f64 of be_mlp_grads.losses and loss_log a
 * (log_rows, 2) f64 device array, log_rows >= 1: row (t mod log_rows) receives a copy of losses, t
 * being the state's step count before the call -- a replayed graph logs every iteration's losses.
 * Asynchronous on `stream`, no allocation and no synchronisation (graph-capturable as a linear
 * chain); two launches: the update + pack kernel, the state kernel.
 * BE_E_INVALID, with nothing launched: a NULL mlp; an unknown kind; a NULL params or grads; a NULL
 * or not 4-byte aligned tensor of a given set, named in the message ("grads->w2"); w3 / b3 not
 * matching the layer count; moment sets missing for ADAM or given to SGD; state NULL or not 8-byte
 * aligned; for ADAM a beta outside [0, 1) or eps < 0; losses and loss_log not both or neither, or not
 * 8-byte aligned; log_rows < 1 with a log.                                                        */
typedef struct be_mlp_tensors {     /* f32 device arrays, state_dict layout, be_mlp_load's shapes  */
  float *w1, *b1, *w2, *b2, *w3, *b3;                /* 2 layers: w3 = b3 = NULL                     */
} be_mlp_tensors;
#define BE_MLP_OPT_ADAM 0
#define BE_MLP_OPT_SGD  1
int be_mlp_opt(be_mlp* mlp, int32_t kind, const be_mlp_tensors* params, const be_mlp_tensors* grads,
               const be_mlp_tensors* exp_avg, const be_mlp_tensors* exp_avg_sq, double* state,
               double beta1, double beta2, double eps,
               const double* losses, double* loss_log, int32_t log_rows, void* stream);

/* ---- A2C targets: the batched finish_episode (examples/ball_cnn_ac3.py:222-246) ----
 * From a recorded rollout of `steps` rows of ctx's N envs -- contiguous (steps, N) device
 * arrays: rewards f64, dones u8 0/1 (what be_out.done and the rollouts write), values f32 or
 * NULL; bootstrap (N) f64 or NULL: the return carried into the last, horizon-cut run -- the
 * per-episode normalised returns the policy and value losses are built from.  An episode of
 * env n is a maximal run of steps s..e with done[e] set or e = steps-1, and s = 0 or
 * done[s-1] set.  The arithmetic is pinned, so the outputs are reproducible bit for bit:
 *   1. walking t = steps-1 .. 0: acc = bootstrap[n] (or 0) at first, acc = 0 whenever done[t]
 *      is set, then acc = rewards[t] + gamma * acc (one f64 multiply, one f64 add, no FMA);
 *      R[t] = acc
 *   2. r32[t] = (float)R[t]
 *   3. mean = (sum of r32 in f64, accumulated in decreasing t) / L        (L = e - s + 1)
 *   4. ss = sum of (r32 - mean)^2 in f64, accumulated in increasing t
 *   5. L >= 2: std = sqrt(ss / (L-1)), returns_norm[t] = (float)(((double)r32[t] - mean) /
 *      (std + eps)), valid = 1, advantage[t] = returns_norm[t] - values[t] in f32
 *   6. L == 1 (never trained on, :614): returns_norm = 0, advantage = 0, valid = 0 (written).
 * Asynchronous on `stream`, no allocation and no synchronisation (graph-capturable).  While
 * the kernel runs returns_norm and valid hold intermediate values.                        */
typedef struct be_a2c_out {
  double*  returns;       /* (T, N) f64 R_t, or NULL                                   */
  float*   returns_norm;  /* (T, N) f32 normalised return, required                    */
  float*   advantage;     /* (T, N) f32 returns_norm - values, or NULL (needs values)  */
  uint8_t* valid;         /* (T, N) 1: the element's episode has >= 2 steps; required  */
} be_a2c_out;

int be_a2c_targets(be_ctx* ctx, const double* rewards, const uint8_t* dones, const float* values,
                   const double* bootstrap, int32_t steps, double gamma, double eps,
                   const be_a2c_out* out, void* stream);

/* ---- A2C losses and gradients: the rest of finish_episode (examples/ball_cnn_ac3.py:233-244) ----
 * The policy and value losses of Policy(W) over `rows` recorded rows (T*N of any rollout; every
 * row offset is 64-bit) and their gradients, i.e. what loss.backward() leaves in the six .grad.
 * Contiguous device arrays: obs (rows, F) u8 with F = 4 + W*W of ctx (bytes 0 and 1, what the step
 * kernels write), actions (rows) u8, returns_norm (rows) f32 and valid (rows) u8 as be_a2c_targets
 * writes them.  A row is active when valid != 0 and action < num_actions; any other row adds
 * nothing.  Per active row, in f32 (x = the row's observation, a = its action, Rn = returns_norm):
 *   pre = W1 x + b1;  h = max(pre, 0);  z = Wa h + ba;  v = Wv h + bv
 *   logp = z[a] - logsumexp(z)                       (log-softmax: finite where softmax underflows)
 *   adv = Rn - v                                     (v not differentiated here: value.item(), :234)
 *   policy_loss += -logp * adv;                      dz_j = adv * (p_j - [j == a]),  p = softmax(z)
 *   d = v - Rn;  value_loss += |d| < 1 ? 0.5 d^2 : |d| - 0.5;    dv = |d| < 1 ? d : sign(d)  (:238)
 *   dh = Wa^T dz + Wv^T dv;  dpre = pre > 0 ? dh : 0
 *   gW1 += dpre (x) x;  gb1 += dpre;  gWa += dz (x) h;  gba += dz;  gWv += dv h;  gbv += dv
 * No float atomics: each workgroup of a grid that depends only on rows and the device adds its
 * rows in a fixed order and writes its sums to `workspace`; a second kernel adds the workgroups'
 * sums in workgroup order in f64 and rounds once to f32 (the losses stay f64).  Two calls on the
 * same inputs and device give the same bits whatever the workspace held.  Every output element is
 * written on every call (zeros when no row is active; rows = 0 is valid).  Asynchronous on
 * `stream`, no allocation and no synchronisation (graph-capturable).                       */
typedef struct be_a2c_weights {           /* state_dict layout, as be_policy_load takes them */
  const float* fc1_weight;          /* (hidden, F)            Policy.fc1, :121 / :137          */
  const float* fc1_bias;            /* (hidden)                                                */
  const float* action_head_weight;  /* (num_actions, hidden)  Policy.action_head, :124 / :142  */
  const float* action_head_bias;    /* (num_actions)                                           */
  const float* value_head_weight;   /* (1, hidden)            Policy.value_head, :127 / :145   */
  const float* value_head_bias;     /* (1)                                                     */
  int32_t hidden;                   /* 1 .. 256 (be_policy_create's bounds; F <= 128)          */
  int32_t num_actions;              /* 1 .. 15                                                 */
} be_a2c_weights;

typedef struct be_a2c_grads {             /* what loss.backward() (:243) leaves in each .grad */
  float* fc1_weight;                /* (hidden, F)                                             */
  float* fc1_bias;                  /* (hidden)                                                */
  float* action_head_weight;        /* (num_actions, hidden)                                   */
  float* action_head_bias;          /* (num_actions)                                           */
  float* value_head_weight;         /* (1, hidden)                                             */
  float* value_head_bias;           /* (1)                                                     */
  double* losses;                   /* [3]: sum of policy losses (:236), sum of value losses
                                       (:238), number of active rows                           */
} be_a2c_grads;

/* Bytes of workspace be_a2c_grad needs on ctx's device (8-byte aligned; independent of rows);
 * < 0: an error code.                                                                       */
int64_t be_a2c_grad_workspace_bytes(be_ctx* ctx, int32_t hidden, int32_t num_actions);
int be_a2c_grad(be_ctx* ctx, const uint8_t* obs, const uint8_t* actions, const float* returns_norm,
                const uint8_t* valid, int64_t rows, const be_a2c_weights* weights, void* workspace,
                int64_t workspace_bytes, const be_a2c_grads* grads, void* stream);

/* ---- the Adam step and the policy re-pack: optimizer.step() (examples/ball_cnn_ac3.py:244, :505) ----
 * One Adam step (torch.optim.Adam with weight_decay = 0, amsgrad = False, maximize = False) on the
 * six Policy tensors in place, and `pol`'s packed image rebuilt from the new weights: afterwards
 * the image holds the bytes be_policy_load would build from them, so be_policy_act / be_policy_rollout
 * run the updated policy.  pol's ctx, F = 4 + W*W, hidden and num_actions define every shape; a
 * policy that was never loaded is accepted (the step defines the whole image).
 * All tensors are contiguous f32 device arrays in state_dict layout: params (updated), grads (read:
 * what be_a2c_grad writes), exp_avg and exp_avg_sq (updated; zeros for a fresh optimizer).
 * state: 4 f64 on the device, [t, beta1^t, beta2^t, lr]; a fresh optimizer holds [0, 1, 1, lr].
 * The learning rate lives on the device so that a captured graph follows a change of it.
 * The arithmetic is pinned; every operation is one f64 operation, no FMA:
 *   t' = t + 1;  p1' = p1 * beta1;  p2' = p2 * beta2         (state after the call: [t', p1', p2', lr])
 *   bc1 = 1 - p1';  bc2s = sqrt(1 - p2');  ss = lr / bc1
 *   per element:  g = (double)grad
 *     m' = (float)(beta1 * (double)m + (1 - beta1) * g)
 *     v' = (float)(beta2 * (double)v + ((1 - beta2) * g) * g)
 *     w' = (float)((double)w - ss * ((double)m' / (sqrt((double)v') / bc2s + eps)))
 * Every element is computed from the state as it was before the call; the state advances exactly
 * once per call, after all of them (a one-thread kernel behind the update kernel on `stream`).
 * losses / loss_log: both NULL, or losses = the 3 f64 of be_a2c_grads.losses and loss_log a
 * (log_rows, 3) f64 device array, log_rows >= 1: row (t mod log_rows) receives a copy of losses, t
 * being the state's step count before the call -- a replayed graph logs every iteration's losses.
 * Asynchronous on `stream`, no allocation and no synchronisation (graph-capturable); three
 * launches: the update + pack kernel, the state kernel, the empty-window table pass.        */
typedef struct be_a2c_tensors {           /* six f32 device arrays, state_dict layout             */
  float* fc1_weight;                /* (hidden, F)                                             */
  float* fc1_bias;                  /* (hidden)                                                */
  float* action_head_weight;        /* (num_actions, hidden)                                   */
  float* action_head_bias;          /* (num_actions)                                           */
  float* value_head_weight;         /* (1, hidden)                                             */
  float* value_head_bias;           /* (1)                                                     */
} be_a2c_tensors;

int be_a2c_adam(be_policy* pol, const be_a2c_tensors* params, const be_a2c_tensors* grads,
                const be_a2c_tensors* exp_avg, const be_a2c_tensors* exp_avg_sq, double* state, double beta1,
                double beta2, double eps, const double* losses, double* loss_log, int32_t log_rows, void* stream);

/* ---- the createBoard physics profile ----
 * N independent ballenv_pygame.createBoard worlds (reset :460-513, step :650-675,
 * calc_reward :680-706) with the 20 featureExtractor features (featureExtractor.py:247-265)
 * that step() computes.  f64 coordinates (ranf spawns), static obstacles only (the
 * reference's dynamic path is not runnable: createBoard never sets obstacle_goal_list). */
#define BE_BOARD_MAX_STATIC 32
#define BE_BOARD_MAX_ACTIONS 16
#define BE_BOARD_FEATURES 20

typedef struct be_board_config {
  int32_t num_envs;
  int32_t num_static;         /* createBoard(static_obstacles=) */
  int64_t env_offset;         /* global id of local env 0 (Philox key) */
  uint64_t seed;
  int32_t screen_width, screen_height;                /* _screen_width/_height = 100 (:8-9) */
  int32_t strip_obs_x, strip_obs_y;                   /* 0, 0 */
  int32_t strip_goal_x, strip_goal_y;                 /* 100, 100 */
  int32_t strip_agent_x, strip_agent_y;               /* 100, 100 */
  double agent_radius;        /* agent_radius = 10 (:316) */
  double static_radius;       /* static_obstacle_radius = 10: collisions at <= static + agent (:381-387) */
  double obstacle_feature_radius;  /* Obstacle.rad = 20 (:35-38): featureExtractor's calcDistance */
  double goal_threshold;      /* 15, strict < (:345, :690) */
  double min_spawn_dist;      /* 50: agent re-sampled while closer to the goal (:476-481) */
  double spawn_thresh_agent, spawn_thresh_goal;       /* 15, 5: static spawn rejection (:494) */
  int32_t num_actions;
  double actions[BE_BOARD_MAX_ACTIONS][2];            /* actionArray (:352-353): (0,-1),(1,0),(0,1),(-1,0) */
  int32_t time_limit;         /* 0 = none (createBoard has no TimeLimit) */
  int32_t autoreset;          /* 1: a done env is reset inside be_board_step */
} be_board_config;

typedef struct be_board_state {
  double* agent;        /* (N, 2) f64  state[0] */
  double* goal;         /* (N, 2) f64  state[1] */
  double* dist;         /* (N) f64     state[2] */
  double* total_dist;   /* (N) f64     total_distance */
  double* ep_return;    /* (N) f64     total_reward_accumulated */
  int32_t* ep_len;      /* (N) */
  uint32_t* episode;    /* (N) resets so far (Philox key) */
  int32_t* static_obs;  /* (Ns, N) int16x2 packed integer obstacle positions */
} be_board_state;

typedef struct be_board_out {
  float* features;      /* (N, 20) f32 featureExtractor output (sensor_readings), or NULL */
  double* reward;       /* (N) (step only) */
  uint8_t* done;        /* (N) (step only) */
  uint8_t* truncated;   /* (N) or NULL */
} be_board_out;

typedef struct be_board be_board;

int be_board_config_default(be_board_config* cfg, int32_t num_envs, int32_t num_static);
int be_board_create(const be_board_config* cfg, int32_t device, be_board** out);
int be_board_destroy(be_board* b);
const char* be_board_last_error(const be_board* b);
/* createBoard.reset for every env (or mask[i] != 0).  reset_tape: (tape_len, N) f64, the
 * reference's np.random.ranf / randint values in call order (parity); NULL: Philox. */
int be_board_reset(be_board* b, const be_board_state* st, const uint8_t* mask, const double* reset_tape,
                   int32_t tape_len, const be_board_out* out, void* stream);
/* createBoard.step + featureExtractor for every env: actions (N) u8 indices into cfg.actions,
 * or deltas (N, 2) f64 (take_action_from_user's float moves). */
int be_board_step(be_board* b, const be_board_state* st, const uint8_t* actions, const double* deltas,
                  const be_board_out* out, void* stream);
/* featureExtractor of the current state (no state change). */
/* `steps` consecutive be_board_step calls in one launch, each env's state in registers:
 * actions (steps, N) u8 or deltas (steps, N, 2) f64; out->reward / done / truncated
 * (steps, N) and out->features (steps, N, 20) or NULL.  Philox resets only (no tape).
 * Bit-identical to `steps` be_board_step calls (the caller's per-step loop over
 * createBoard.step, ballenv_pygame.py:650-675, for every env).                      */
int be_board_rollout(be_board* b, const be_board_state* st, const uint8_t* actions, const double* deltas,
                     int32_t steps, const be_board_out* out, void* stream);
int be_board_observe(be_board* b, const be_board_state* st, const be_board_out* out, void* stream);
int be_board_status(be_board* b, int32_t* status_out, void* stream);
/* The board's autoreset pool (as be_pool_* above): with Philox autoreset and one lane
 * per env, be_board_reset queues a fill of every env's next two episodes' resets and be_board_step
 * one every 128 steps (BALLENV_POOL_PERIOD), and the steps of the state last reset copy a current
 * entry where they would draw the reset inline -- the same bits either way.  The same ordering
 * contract holds: the caller orders every launch that uses a board's pool on one stream, a change
 * of owner (be_board_reset of another state) included.  BALLENV_POOL=0 at create disables it.
 * Bytes held (0: no pool). */
int64_t be_board_pool_bytes(const be_board* b);

#ifdef __cplusplus
}
#endif
#endif /* BALLENV_H */
