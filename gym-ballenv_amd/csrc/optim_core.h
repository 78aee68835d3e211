// optim_core.h -- the optimiser arithmetic include/ballenv.h pins, shared by the three update kernels
// (a2c_adam_kernel in a2c_adam.hip, mlp_opt_kernel in mlp_policy.hip, cnn_adam_kernel in cnn_policy.hip): one step's constants and one
// element's update.  f64 operations on f32 storage, no FMA (every unit is built with
// -ffp-contract=off); the operand order below is the pinned one.
// Reference: torch.optim.Adam (weight_decay=0, amsgrad=False, maximize=False), examples/ball_cnn_ac3.py:505,
// examples/ball_env_reinforce.py:196, examples/ball_cnn_reinforce.py:244; torch.optim.SGD (momentum=0), examples/train_supervise.py:75.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

// One Adam step's constants: bc2s = sqrt(1 - beta2^t), ss = lr / (1 - beta1^t), t the step being taken.
struct AdamStep { double beta1, beta2, omb1, omb2, eps, bc2s, ss; };

// state: [t, beta1^t, beta2^t, lr] as it was before the call
__device__ __forceinline__ AdamStep adam_step(const double* state, double beta1, double beta2, double eps) {
  const double p1 = state[1] * beta1, p2 = state[2] * beta2, lr = state[3];
  return AdamStep{beta1, beta2, 1.0 - beta1, 1.0 - beta2, eps, sqrt(1.0 - p2), lr / (1.0 - p1)};
}

// One element of an Adam step, in place.  Returns w'.
__device__ __forceinline__ float adam_elem(const AdamStep& c, const float* g, float* m, float* v, float* w, int64_t i) {
  const double gd = (double)g[i];
  const float m1 = (float)(c.beta1 * (double)m[i] + c.omb1 * gd);
  const float v1 = (float)(c.beta2 * (double)v[i] + (c.omb2 * gd) * gd);
  const float w1 = (float)((double)w[i] - c.ss * ((double)m1 / (sqrt((double)v1) / c.bc2s + c.eps)));
  m[i] = m1; v[i] = v1; w[i] = w1;
  return w1;
}

// One element of a plain SGD step (lr = state[3]), in place.  Returns w'.
__device__ __forceinline__ float sgd_elem(double lr, const float* g, float* w, int64_t i) {
  const float w1 = (float)((double)w[i] - lr * (double)g[i]);
  w[i] = w1;
  return w1;
}

}  // namespace
