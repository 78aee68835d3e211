// a2c_adam.hip -- optimizer.step() of the batched A2C update (examples/ball_cnn_ac3.py:244, Adam :505)
// and the re-pack of the new weights for the policy kernels, in one entry:
//
//   be_a2c_adam   one Adam step on the six Policy tensors in place (the arithmetic include/ballenv.h
//                 pins: f64 operations, f32 storage), and the be_policy's packed image rebuilt from
//                 the new weights -- the bytes be_policy_load would build from them
//
// Three launches on the caller's stream:
//
//   a2c_adam_kernel    one wave per padded hidden row m < 16 HT, four rows per 256-thread workgroup,
//                      and one more wave for the head biases.  The wave of row m reads row m of
//                      fc1.weight, its gradient and its two moments as coalesced rows (F <= 128: up
//                      to two columns per lane), b1[m] in lane 16 and column m of the two heads in
//                      lanes o < NO; updates and stores them; takes max|w1'[m, :]| by a wave
//                      reduction (a maximum does not depend on the order, so the row's step s_m has
//                      the bits of the serial pack kernel's); and writes the row's three int8 digit
//                      planes into the fragment layout, bq_m and the row's NO scaled head entries
//                      through the helpers the pack kernel uses (policy_core.h).  Rows m >= H write
//                      the zeros the pack kernel writes.  No wave reads what another writes.
//   optim_advance      one wave: copies the losses into row (t mod rows) of the log, then advances
//                      the state [t, beta1^t, beta2^t, lr].  Every wave of the kernel before it read
//                      the state as it was before the call; stream order is the only ordering needed.
//                      Defined here for be_mlp_opt as well (be_internal_optim_advance, internal.h).
//   policy_kernel      the table pass over the four empty-window observations, as in be_policy_load
//                      (be_internal_policy_table).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "ballenv.h"
#include "host_logic.h"
#include "internal.h"
#include "optim_core.h"
#include "policy_core.h"

namespace {

constexpr int THREADS = 256, ROWS_PER_WG = THREADS / 64;
static_assert(POL_MAXF <= 2 * 64, "a lane holds at most two columns of an fc1 row");
static_assert(POL_MAXA + 1 <= 16, "the head column and b1 share one wave: lanes o < NO <= 16, lane 16");

struct Six { float *w1, *b1, *wa, *ba, *wv, *bv; };

struct AParams {
  Six w, g, m, v;            // params, grads (read only), exp_avg, exp_avg_sq
  const double* state;       // [t, beta1^t, beta2^t, lr] before the call
  double beta1, beta2, eps;
  uint8_t* img;
  PolLayout L;
  int32_t H, F, A;
};

__global__ __launch_bounds__(THREADS) void a2c_adam_kernel(AParams p) {
  const PolLayout& L = p.L;
  const int lane = (int)threadIdx.x & 63;
  const int m = __builtin_amdgcn_readfirstlane((int)blockIdx.x * ROWS_PER_WG + ((int)threadIdx.x >> 6));
  const int rows = 16 * L.HT, H = p.H, F = p.F, A = p.A, NO = L.NO;
  if (m > rows) return;
  const AdamStep c = adam_step(p.state, p.beta1, p.beta2, p.eps);
  const bool is_act = lane < A, is_val = lane == NO - 1;     // this lane's head output, if any

  if (m == rows) {           // the head biases: action o in lane o, the value bias in lane NO - 1
    float b = -INFINITY;     // pad actions
    if (is_act) b = adam_elem(c, p.g.ba, p.m.ba, p.v.ba, p.w.ba, lane);
    else if (is_val) b = adam_elem(c, p.g.bv, p.m.bv, p.v.bv, p.w.bv, 0);
    if (lane < NO) ((float*)(p.img + L.hbias))[lane] = b;
    return;
  }

  int32_t* bias = (int32_t*)(p.img + L.bias);
  if (m >= H) {              // a padded row: zeros
    if (lane == 0) bias[m] = 0;
    for (int k = lane; k < L.KS * 64; k += 64) pol_store_digits(p.img, L, m, k, false, 0.f, 1.0);
    if (lane < NO) pol_store_head(p.img, L, m, lane, 0.0, 1.0);
    return;
  }

  float wn[2] = {0.f, 0.f}, mx = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = lane + 64 * j;
    if (k < F) {
      wn[j] = adam_elem(c, p.g.w1, p.m.w1, p.v.w1, p.w.w1, (int64_t)m * F + k);
      mx = fmaxf(mx, fabsf(wn[j]));
    }
  }
  float hw = 0.f;            // lanes o < NO: W_o,m (0 for a pad output); lane 16: b1[m]
  if (is_act) hw = adam_elem(c, p.g.wa, p.m.wa, p.v.wa, p.w.wa, (int64_t)lane * H + m);
  else if (is_val) hw = adam_elem(c, p.g.wv, p.m.wv, p.v.wv, p.w.wv, m);
  else if (lane == 16) hw = adam_elem(c, p.g.b1, p.m.b1, p.v.b1, p.w.b1, m);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  const float b1n = __shfl(hw, 16);
  const double s = pol_row_step(mx, b1n);
  if (lane == 0) bias[m] = pol_quant_bias(b1n, s);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = lane + 64 * j;
    if (k < L.KS * 64) pol_store_digits(p.img, L, m, k, k < F, wn[j], s);
  }
  if (lane < NO) pol_store_head(p.img, L, m, lane, (double)hw, s);
}

// One wave, behind an update kernel on the stream: lane k < width copies loss k into row (t mod rows) of
// the log (one load and one store in flight for the whole row), then lane 0 advances the state
// (powers == 0, plain SGD: the step count alone).  Every lane has its t before lane 0 stores t + 1: the
// load is one instruction of the wave, and the stored value depends on it.
__global__ __launch_bounds__(64) void optim_advance(double* state, int32_t powers, double beta1, double beta2,
                                                    const double* losses, double* loss_log, int32_t width,
                                                    int32_t log_rows) {
  const int k = (int)threadIdx.x;
  const double t = state[0];
  if (loss_log && k < width) loss_log[width * ((int64_t)t % log_rows) + k] = losses[k];
  if (k != 0) return;
  state[0] = t + 1.0;
  if (powers) {
    state[1] = state[1] * beta1;
    state[2] = state[2] * beta2;
  }
}

// the first NULL or misaligned pointer of a tensor set, as "<set>-><field>", or nullptr
const char* bad_field(const be_a2c_tensors* t, const char* const (&names)[6]) {
  const float* const ptrs[6] = {t->fc1_weight, t->fc1_bias, t->action_head_weight, t->action_head_bias,
                                t->value_head_weight, t->value_head_bias};
  for (int i = 0; i < 6; ++i)
    if (!ptrs[i] || ((uintptr_t)ptrs[i] & 3)) return names[i];
  return nullptr;
}

#define BE_SIX_NAMES(set)                                                                              \
  {set "->fc1_weight", set "->fc1_bias", set "->action_head_weight", set "->action_head_bias",         \
   set "->value_head_weight", set "->value_head_bias"}
const char* const N_PARAMS[6] = BE_SIX_NAMES("params");
const char* const N_GRADS[6] = BE_SIX_NAMES("grads");
const char* const N_AVG[6] = BE_SIX_NAMES("exp_avg");
const char* const N_SQ[6] = BE_SIX_NAMES("exp_avg_sq");

Six six(const be_a2c_tensors* t) {
  return {t->fc1_weight, t->fc1_bias, t->action_head_weight, t->action_head_bias, t->value_head_weight,
          t->value_head_bias};
}

}  // namespace

int be_internal_optim_advance(char* err, double* state, bool powers, double beta1, double beta2, const double* losses,
                              double* loss_log, int32_t width, int32_t log_rows, void* stream) {
  hipLaunchKernelGGL(optim_advance, dim3(1), dim3(64), 0, (hipStream_t)stream, state, (int32_t)powers, beta1, beta2,
                     losses, loss_log, width, log_rows);
  return be_launched(err);
}

extern "C" {

int be_a2c_adam(be_policy* pol, const be_a2c_tensors* params, const be_a2c_tensors* grads,
                const be_a2c_tensors* exp_avg, const be_a2c_tensors* exp_avg_sq, double* state, double beta1,
                double beta2, double eps, const double* losses, double* loss_log, int32_t log_rows, void* stream) {
  if (!pol) return be_ctx_fail(nullptr, BE_E_INVALID, "be_a2c_adam: policy is NULL");
  const be_policy_view pv = be_policy_get(pol);
  be_ctx* ctx = pv.ctx;
  char* err = be_ctx_err(ctx);
  if (!params) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_adam: params is NULL");
  if (!grads) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_adam: grads is NULL");
  if (!exp_avg) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_adam: exp_avg is NULL");
  if (!exp_avg_sq) return be_ctx_fail(ctx, BE_E_INVALID, "be_a2c_adam: exp_avg_sq is NULL");
  const struct { const be_a2c_tensors* t; const char* const (&names)[6]; } sets[4] = {
      {params, N_PARAMS}, {grads, N_GRADS}, {exp_avg, N_AVG}, {exp_avg_sq, N_SQ}};
  for (const auto& s : sets)
    if (const char* name = bad_field(s.t, s.names))
      return be_fail(err, BE_E_INVALID, "be_a2c_adam: %s is NULL or not 4-byte aligned", name);
  if (const char* msg = behost::optim_args_error(state, true, beta1, beta2, eps, losses, loss_log, log_rows))
    return be_fail(err, BE_E_INVALID, "be_a2c_adam: %s", msg);
  BE_ENTER_DEVICE(err, pv.device);
  const AParams p{six(params), six(grads), six(exp_avg), six(exp_avg_sq), state, beta1, beta2, eps, pv.img,
                  pol_layout(pv.HT, pv.KS, pv.NO), pv.H, pv.F, pv.A};
  hipStream_t hs = (hipStream_t)stream;
  const int waves = 16 * pv.HT + 1;          // the padded rows and the head-bias wave
  hipLaunchKernelGGL(a2c_adam_kernel, dim3((unsigned)((waves + ROWS_PER_WG - 1) / ROWS_PER_WG)), dim3(THREADS), 0, hs,
                     p);
  if (int rc = be_launched(err)) return rc;
  if (int rc = be_internal_optim_advance(err, state, true, beta1, beta2, losses, loss_log, 3, log_rows, stream)) return rc;
  return be_internal_policy_table(pol, stream);
}

}  // extern "C"
