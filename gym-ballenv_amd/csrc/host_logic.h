// host_logic.h -- the host side's logic that needs no HIP: the autoreset pool's bookkeeping, the
// checkpoint blob's layout, be_pool_entry's word order, the per-step slice of a be_out, be_step's rule for
// step2_kernel's wide-row-load instance, be_mlp_rollout's instance rule and argument checks.  Only
// ballenv.h, pool_layout.h and standard headers, so the host C++ compiler alone builds and tests it
// (tests/host_logic_main.cpp, tests/step2_wide_host_main.cpp, tests/mlp_rollout_host_main.cpp); internal.h is
// the half that touches HIP.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "ballenv.h"
#include "pool_layout.h"

namespace behost {

// The autoreset pool's bookkeeping, for the step engine's context and the board's alike (the device
// memory is the context's own).  The pool serves one state, its owner, named by the state's episode
// array: the state last reset / loaded / filled for, else the first one stepped.  A step of any
// other state draws its resets inline.
struct PoolBook {
  bool has = false;            // the context allocated a pool (false: every method answers "no pool")
  int period = 128;            // owner step launches per fill (0: explicit fills only)
  int calls = 0;               // owner step launches since the last fill
  const void* owner = nullptr;

  // BALLENV_POOL: "0" disables the pool (A/B).  BALLENV_POOL_PERIOD: the period, clamped at 0.
  static bool env_enabled() { const char* v = getenv("BALLENV_POOL"); return !v || strcmp(v, "0") != 0; }
  void period_from_env() {
    const char* v = getenv("BALLENV_POOL_PERIOD");
    const int n = v ? atoi(v) : 128;
    period = n > 0 ? n : 0;
  }
  // A step launch of `state` that meets the pool's preconditions: does it use the pool?  Claims an
  // unowned pool.  (An ownership change is not ordered against the previous owner's launches here:
  // the caller orders them, include/ballenv.h.)
  bool step(const void* state) {
    if (!has) return false;
    if (!owner) owner = state;
    return state == owner;
  }
  // One step launch of the owner went out: is a fill due now?  A due fill restarts the count.
  bool fill_due() {
    if (period <= 0 || ++calls < period) return false;
    calls = 0;
    return true;
  }
  // A reset, a load or an explicit fill for `state`: it becomes the owner, and the fill that
  // follows restarts the count.
  void claim(const void* state) { owner = state; calls = 0; }
  void set_period(int p) { period = p; calls = 0; }
};

// ---- env-state checkpoint: a 64-byte header + the be_state arrays at 16-byte aligned offsets
struct BlobLayout { int64_t off[10], bytes[10], total; };
inline BlobLayout blob_layout(const be_config* c) {
  BlobLayout b;
  const int64_t N = c->num_envs, ns = c->num_static, nd = c->num_dynamic;
  const int64_t sz[10] = {4 * N, 4 * N, 8 * N, 8 * N, 8 * N, 4 * N, 4 * N, 4 * ns * N, 4 * nd * N, nd * N};
  int64_t o = 64;
  for (int k = 0; k < 10; ++k) { b.off[k] = o; b.bytes[k] = sz[k]; o += (sz[k] + 15) & ~15ll; }
  b.total = o;
  return b;
}
inline void blob_header(const be_config* c, int64_t total, int64_t (&hdr)[8]) {
  memset(hdr, 0, sizeof hdr);
  memcpy(&hdr[0], "BALLENV1", 8);
  hdr[1] = BE_ABI_VERSION; hdr[2] = c->num_envs; hdr[3] = c->num_static; hdr[4] = c->num_dynamic; hdr[5] = total;
}
inline void state_ptrs(const be_state* st, void* (&p)[10]) {
  p[0] = st->agent; p[1] = st->goal; p[2] = st->prev_dist; p[3] = st->total_dist; p[4] = st->ep_return;
  p[5] = st->ep_len; p[6] = st->episode; p[7] = st->static_obs; p[8] = st->dyn_obs; p[9] = st->dyn_goal;
}

// ---- be_pool_entry's word order (TAG, AGENT, GOAL, ROWS0 | flags << 30, ROWS1, ROWS2, the n_obs
// obstacles; f64: PREV, TOTAL) from / to an entry's (tag, body) pair of pool_layout.h
inline void pool_entry_unpack(const uint32_t (&tag)[2], const uint32_t* body, int n_obs, uint32_t* words, double* f64) {
  using namespace bestep;
  words[0] = tag[0]; words[1] = body[PB_AGENT]; words[2] = body[PB_GOAL];
  words[3] = (body[PB_ROWS] & 0x3FFFFFFFu) | ((tag[1] & 3u) << 30);
  words[4] = body[PB_ROWS + 1]; words[5] = body[PB_ROWS + 2];
  for (int k = 0; k < n_obs; ++k) words[6 + k] = body[PB_OBS + k];
  memcpy(&f64[0], &body[PB_PREV], 8);
  memcpy(&f64[1], &body[PB_TOTAL], 8);
}
// (writes the words it names; the body's other words keep what they held)
inline void pool_entry_pack(const uint32_t* words, const double* f64, int n_obs, uint32_t (&tag)[2], uint32_t* body) {
  using namespace bestep;
  tag[0] = words[0]; tag[1] = (words[3] >> 30) & 3u;
  body[PB_AGENT] = words[1]; body[PB_GOAL] = words[2];
  body[PB_ROWS] = words[3] & 0x3FFFFFFFu; body[PB_ROWS + 1] = words[4]; body[PB_ROWS + 2] = words[5];
  for (int k = 0; k < n_obs; ++k) body[PB_OBS + k] = words[6 + k];
  memcpy(&body[PB_PREV], &f64[0], 8);
  memcpy(&body[PB_TOTAL], &f64[1], 8);
}

// Step s's slice of a (steps, N, ...) be_out, F = 4 + W*W; NULL members stay NULL and stats, which
// accumulates over the steps, stays whole.
inline be_out be_out_at(const be_out& out, int64_t s, int64_t N, int64_t F) {
  be_out o = out;
  if (o.obs) o.obs += s * N * F;
  if (o.obs_f32) o.obs_f32 += s * N * F;
  if (o.reward) o.reward += s * N;
  if (o.done) o.done += s * N;
  if (o.truncated) o.truncated += s * N;
  if (o.terminal_obs) o.terminal_obs += s * N * F;
  if (o.final_return) o.final_return += s * N;
  if (o.final_len) o.final_len += s * N;
  return o;
}

// ---- be_step: does this call's state take step2_kernel's wide-row-load instance?  It loads a
// wave's 32 envs of an obstacle row 16 bytes per lane, so every wave must be whole (num_envs a positive
// multiple of 32) and every row chunk 16-byte aligned (the three obstacle arrays; with them aligned and
// 32 | num_envs every row of every wave is).  force: BALLENV_STEP2_WIDE as be_create read it (-1: the rule;
// 0: never; 1: wherever the instance is correct -- the conditions above are correctness, not preference,
// and no override lifts them).  STEP2_WIDE_DEFAULT: what the rule answers without an override where the
// instance may run.
constexpr bool STEP2_WIDE_DEFAULT = true;
inline bool step2_wide(int64_t num_envs, const void* static_obs, const void* dyn_obs, const void* dyn_goal, int force = -1) {
  if (force == 0) return false;
  if (num_envs < 32 || num_envs % 32) return false;
  if (!static_obs || !dyn_obs || !dyn_goal) return false;
  if (((uintptr_t)static_obs | (uintptr_t)dyn_obs | (uintptr_t)dyn_goal) & 15) return false;
  return force == 1 || STEP2_WIDE_DEFAULT;
}
// BALLENV_STEP2_WIDE: exactly "0" or "1", else (or unset) -1
inline int step2_wide_env(const char* v) {
  if (!v || !v[0] || v[1]) return -1;
  return v[0] == '0' ? 0 : (v[0] == '1' ? 1 : -1);
}
// which instance the context's last be_step / be_step_n launch took (be_step_instance, include/ballenv.h)
enum { STEP_INSTANCE_NONE = 0, STEP_INSTANCE_PLAIN = 1, STEP_INSTANCE_WIDE = 2 };

// ---- be_mlp_rollout: waves per workgroup of the fused kernel (mlp_rollout_kernel<LAYERS, NW>)
// A wave owns 32 envs and a workgroup stages the whole packed image, which leaves room for one workgroup
// per compute unit: the largest NW of 8, 4, 2 whose full workgroups still give every compute unit one
// (num_envs >= 32 NW cus), else 1 -- a batch too small for that runs one wave on as many units as it has
// 32-env groups.  The same for both layer counts (`layers` is an argument so that a measured difference has
// a place).  force: BALLENV_MLP_ROLLOUT_WAVES as be_mlp_create read it (-1: the rule; 0: no fused kernel,
// the caller loops be_mlp_act + be_step; 1, 2, 4, 8: that instance).  Returns 0, 1, 2, 4 or 8.
inline int mlp_rollout_waves(int64_t num_envs, int cus, int layers, int force = -1) {
  if (force >= 0) return force;
  if (num_envs < 1 || cus < 1 || (layers != 2 && layers != 3)) return 0;
  for (int nw = 8; nw > 1; nw >>= 1)
    if (num_envs >= (int64_t)32 * nw * cus) return nw;
  return 1;
}
// BALLENV_MLP_ROLLOUT_WAVES: exactly one of 0, 1, 2, 4, 8, else (or unset) -1
inline int mlp_rollout_waves_env(const char* v) {
  if (!v || !v[0] || v[1]) return -1;
  return (v[0] == '0' || v[0] == '1' || v[0] == '2' || v[0] == '4' || v[0] == '8') ? v[0] - '0' : -1;
}
// be_mlp_rollout's argument checks that need no device, in this order; NULL: fine, else the message.
inline const char* mlp_rollout_args_error(const void* obs_last, int32_t steps, const be_out* out, const be_act_out* act) {
  if (steps < 0) return "be_mlp_rollout: steps must be >= 0";
  if (!out || !out->reward || !out->done) return "be_mlp_rollout needs out->reward and out->done";
  if (!act || !act->action) return "be_mlp_rollout needs act->action";
  if (!obs_last) return "be_mlp_rollout needs obs_last";
  if ((uintptr_t)obs_last & 15) return "be_mlp_rollout: obs_last must be 16-byte aligned";
  if (out->obs || out->obs_f32 || out->terminal_obs)
    return "be_mlp_rollout: out->obs, obs_f32 and terminal_obs must be NULL (this agent reads no window rows)";
  if (act->value || act->probs) return "be_mlp_rollout: act->value and act->probs must be NULL";
  return nullptr;
}

// The optimiser arguments be_a2c_adam, be_mlp_opt and be_cnn_adam share, checked in this order: the state, the Adam
// constants (adam == false, plain SGD, has none), the loss log.  NULL: fine, else the message's tail,
// which the entry point puts behind its own name.
inline const char* optim_args_error(const double* state, bool adam, double beta1, double beta2, double eps,
                                    const double* losses, const double* loss_log, int32_t log_rows) {
  if (!state || ((uintptr_t)state & 7)) return "state is NULL or not 8-byte aligned";
  if (adam) {
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return "beta1 must be in [0, 1)";
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return "beta2 must be in [0, 1)";
    if (!(eps >= 0.0)) return "eps must be >= 0";
  }
  if ((losses != nullptr) != (loss_log != nullptr)) return "losses and loss_log go together (both or neither)";
  if (((uintptr_t)losses & 7) || ((uintptr_t)loss_log & 7)) return "losses / loss_log is not 8-byte aligned";
  if (loss_log && log_rows < 1) return "log_rows must be >= 1";
  return nullptr;
}

// be_mlp_grad's argument checks that need no device (mlp_grad.hip): the block MLP's shape against
// be_mlp_create's bounds and w3 / b3 against the layer count.  NULL: fine, else the message.
inline const char* mlp_grad_shape_error(int layers, int hidden1, int hidden2, int num_actions) {
  if (layers != 2 && layers != 3) return "be_mlp_grad: layers must be 2 or 3";
  if (hidden1 < 1 || hidden1 > 128) return "be_mlp_grad: hidden1 must be in [1, 128]";
  if (layers == 3 && (hidden2 < 1 || hidden2 > 128)) return "be_mlp_grad: hidden2 must be in [1, 128]";
  if (layers == 2 && hidden2 != 0) return "be_mlp_grad: hidden2 must be 0 with 2 layers";
  if (num_actions < 1 || num_actions > 15) return "be_mlp_grad: num_actions must be in [1, 15]";
  return nullptr;
}
inline const char* mlp_grad_last_layer_error(int layers, const void* w3, const void* b3) {
  if (layers == 3 && (!w3 || !b3)) return "be_mlp_grad: 3 layers need w3 and b3 (weights and grads)";
  if (layers == 2 && (w3 || b3)) return "be_mlp_grad: w3 and b3 must be NULL with 2 layers (weights and grads)";
  return nullptr;
}
// One workgroup's slot of be_mlp_grad's workspace (offsets in floats; the gradient elements in
// state_dict order, then two f64: the sum of the row losses and the number of active rows).
struct MlpGradSlot {
  int32_t o_b1, o_w2, o_b2, o_w3, o_b3, P;      // gW1 at 0; P gradient elements
  int32_t loss_off, slot_bytes;                 // bytes
};
inline MlpGradSlot mlp_grad_slot(int layers, int H1, int H2, int A) {
  MlpGradSlot s{};
  const int n2 = layers == 3 ? H2 : A;          // rows of affine2
  s.o_b1 = H1 * 29;
  s.o_w2 = s.o_b1 + H1;
  s.o_b2 = s.o_w2 + n2 * H1;
  s.o_w3 = s.o_b2 + n2;
  s.o_b3 = s.o_w3 + (layers == 3 ? A * H2 : 0);
  s.P = s.o_b3 + (layers == 3 ? A : 0);
  s.loss_off = (s.P * 4 + 7) / 8 * 8;
  s.slot_bytes = s.loss_off + 2 * 8;
  return s;
}

}  // namespace behost
