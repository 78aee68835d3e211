// internal.h -- library-internal interface between the translation units of
// libballenv.so (not part of the C ABI in include/ballenv.h), and the HIP-touching half of the
// host toolkit every unit's entry points share: error reporting, entering a context's device, the
// status word.  (The half without HIP: host_logic.h.)
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <hip/hip_runtime.h>

#include "ballenv.h"

// Makes `device` the calling thread's current HIP device for the scope of one entry point and
// restores the caller's device on exit, so no be_* call changes which GPU later torch / HIP calls
// of the same thread use (a one-process multi-device caller).  err != hipSuccess: the switch failed
// (nothing to restore).
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int device) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != device) err = hipSetDevice(device);
    else prev = -1;                        // already current (or the query failed): nothing to restore
    if (err != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Error reporting.  `err` is the 512-byte buffer the caller's last-error function reads: the
// context's, the board's, or the matching thread-local one for a NULL context.  Returns code.
inline int be_fail(char* err, int code, const char* fmt, const char* detail) {
  snprintf(err, 512, fmt, detail ? detail : "");
  return code;
}
inline int be_hip_fail(char* err, hipError_t e) { return be_fail(err, BE_E_HIP, "HIP error: %s", hipGetErrorString(e)); }
#define BE_HIP_TRY(err, expr)                                  \
  do {                                                         \
    const hipError_t e_ = (expr);                              \
    if (e_ != hipSuccess) return be_hip_fail(err, e_);         \
  } while (0)
// An entry point's frame: BE_ENTER_DEVICE once, ahead of its first HIP call (the caller's current
// device is restored when the scope ends), then its launches, then `return be_launched(err)`.
#define BE_ENTER_DEVICE(errbuf, device)    \
  const DeviceGuard device_guard_(device); \
  BE_HIP_TRY(errbuf, device_guard_.err)
inline int be_launched(char* err) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? BE_OK : be_hip_fail(err, e);
}

// The device status word of a context (be_status / be_board_status); the caller holds the device.
struct StatusWord {
  int* word = nullptr;
  hipError_t create() {
    const hipError_t e = hipMalloc(&word, sizeof(int));
    return e == hipSuccess ? hipMemset(word, 0, sizeof(int)) : e;
  }
  void release() { if (word) (void)hipFree(word); word = nullptr; }
  // synchronise the stream, then read and clear the word (*out is written on success only)
  hipError_t take(void* stream, int32_t* out) {
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    int v = 0;
    if (e == hipSuccess) e = hipMemcpy(&v, word, sizeof v, hipMemcpyDeviceToHost);
    const int zero = 0;
    if (e == hipSuccess) e = hipMemcpy(word, &zero, sizeof zero, hipMemcpyHostToDevice);
    if (e == hipSuccess) *out = v;
    return e;
  }
};
// A context's autoreset pool: `bytes` of device memory, every entry unwritten.
inline hipError_t be_pool_alloc(uint32_t** pool, int64_t bytes) {
  hipError_t e = hipMalloc(pool, (size_t)bytes);
  if (e == hipSuccess) e = hipMemset(*pool, 0, (size_t)bytes);
  return e == hipSuccess ? hipDeviceSynchronize() : e;
}

struct be_ctx_view {
  int32_t num_envs, window, device, num_static, num_dynamic;
  int64_t env_offset;
  int32_t screen_width, screen_height, radius_obstacle, radius_agent;   // what a frame of the env shows (pixels.hip)
};
__attribute__((visibility("hidden"))) be_ctx_view be_ctx_get(const be_ctx* ctx);
// ctx's last-error buffer (the calling thread's own for a NULL ctx), and msg recorded in it; returns code
__attribute__((visibility("hidden"))) char* be_ctx_err(be_ctx* ctx);
inline int be_ctx_fail(be_ctx* ctx, int code, const char* msg) { return be_fail(be_ctx_err(ctx), code, "%s", msg); }
// an entry point's ctx and be_state pointer checks ("ctx is NULL" first; BE_OK or a be_ctx_fail code)
__attribute__((visibility("hidden"))) int be_ctx_check_state(be_ctx* ctx, const be_state* st);

// What another unit may know of a be_policy (policy.hip): its packed image on the device and the
// shape it was created for (pol_layout(HT, KS, NO) in policy_core.h is the image's layout).
struct be_policy_view {
  be_ctx* ctx;
  uint8_t* img;
  int32_t HT, KS, NO;          // the layout pick_policy chose
  int32_t H, F, A;             // hidden, 4 + W*W, num_actions
  int32_t device;
};
__attribute__((visibility("hidden"))) be_policy_view be_policy_get(const be_policy* pol);
// The table pass behind a rewritten image (be_policy_load, be_a2c_adam): the dense forward of the four
// empty-window observations into the image's table, on `stream`; marks the policy loaded.  The
// caller has entered the policy's device.  BE_OK or an error code recorded in the ctx.
__attribute__((visibility("hidden"))) int be_internal_policy_table(be_policy* pol, void* stream);

// The state kernel behind an optimiser's update kernel (be_a2c_adam, be_mlp_opt, be_cnn_adam; defined in a2c_adam.hip):
// one wave copies the `width` <= 64 losses into row (t mod log_rows) of loss_log (if there is one), then
// advances state [t, beta1^t, beta2^t, lr] -- the step count alone unless `powers`.  One dim3(1), dim3(64)
// launch on `stream`; the caller has checked the arguments and entered the device.  BE_OK or a HIP error
// recorded in err.
__attribute__((visibility("hidden"))) int be_internal_optim_advance(char* err, double* state, bool powers, double beta1,
                                                                    double beta2, const double* losses, double* loss_log,
                                                                    int32_t width, int32_t log_rows, void* stream);

// fused config-5 rollout (be_policy_rollout -> rollout_kernel with the policy in the loop)
struct be_pol_rollout_args {
  const uint8_t* img;          // packed Policy(W) image (device)
  int32_t img_bytes, HT, KS, NO, num_actions;
  unsigned long long seed;
  const uint8_t* obs_in;       // (N, F) obs of the current state
  uint8_t* obs_last;           // (N, F) or NULL
  int32_t steps;
  const be_out* out;           // per-step (steps, N, ...) outputs
  const be_act_out* act;       // (steps, N) action / log_prob / value
};
// 1: launched; 0: no fused kernel for this env / policy shape (the caller loops); < 0: error.
// The caller has entered the context's device.
__attribute__((visibility("hidden"))) int be_internal_policy_rollout(be_ctx* ctx, const be_state* st,
                                                                     const be_pol_rollout_args* a, void* stream);

// fused block-policy rollout (be_mlp_rollout -> mlp_rollout_kernel, then the observe kernel into obs_last)
struct be_mlp_rollout_args {
  const float* img;            // packed block-MLP image (device; mlp_core.h MlpLayout)
  int32_t layers, waves;       // the instance: 2 | 3 layers, waves per workgroup (host_logic.h mlp_rollout_waves)
  int32_t num_actions, final_relu;
  unsigned long long seed;
  uint8_t* obs_last;           // (N, F)
  uint8_t* blocks_out;         // (steps, N, 29) or NULL
  int32_t steps;
  const be_out* out;           // per-step (steps, N) outputs
  const be_act_out* act;       // (steps, N) action / log_prob
};
// 1: launched; 0: no fused kernel for this env shape / instance (the caller loops); < 0: error.
// The caller has entered the context's device.
__attribute__((visibility("hidden"))) int be_internal_mlp_rollout(be_ctx* ctx, const be_state* st,
                                                                  const be_mlp_rollout_args* a, void* stream);
// The instance name be_internal_mlp_rollout would launch (the calling thread's buffer), or NULL where it returns 0.
__attribute__((visibility("hidden"))) const char* be_internal_mlp_rollout_name(be_ctx* ctx, int32_t layers, int32_t waves);
