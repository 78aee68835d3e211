// blocks_core.h -- prep_state2 of one env (examples/ball_env_reinforce.py:130-172, block_to_arrpos
// :169-172), shared by the observation kernel (features.hip) and the block-count policy
// (mlp_policy.hip): the 29 counters of a row live in 8 packed 32-bit registers, byte b of the row in
// byte b & 3 of word b >> 2 (bytes 29..31 stay 0), and each obstacle adds 1 << 8*(cell & 3) to the
// word of its cell with selects (no scratch memory).  All integer: the reference's
// sign(x)*(x-10)//20 on integer coordinates is exact.  A counter holds at most 1 + the obstacle
// count, so sums of partial rows (one per lane group in mlp_policy.hip) carry nothing across bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int BLK_ROW = 29;      // bytes of a row; BLK_WORDS packed words hold it
constexpr int BLK_WORDS = 8;

__device__ __forceinline__ int floordiv20(int a) { return a >= 0 ? a / 20 : -((-a + 19) / 20); }
__device__ __forceinline__ int px(int32_t p) { return (int)(int16_t)(p & 0xFFFF); }
__device__ __forceinline__ int py(int32_t p) { return p >> 16; }

// A row with no obstacle: the goal's quadrant one-hot (bytes 0..3) and byte 16 (the agent's cell) = 1.
__device__ __forceinline__ void blocks_init(uint32_t (&w8)[BLK_WORDS], int32_t agent, int32_t goal) {
  const int dx = px(goal) - px(agent), dy = py(goal) - py(agent);
  const int quad = dx >= 0 ? (dy >= 0 ? 1 : 2) : (dy >= 0 ? 0 : 3);
#pragma unroll
  for (int q = 0; q < BLK_WORDS; ++q) w8[q] = 0;
  w8[0] = 1u << (8 * quad);
  w8[4] = 1u;
}

// +1 in the cell of obstacle o (packed x | y << 16) around the agent at (ax, ay), if `live` and the
// cell lies in the 5x5 grid.
__device__ __forceinline__ void blocks_add(uint32_t (&w8)[BLK_WORDS], int ax, int ay, int32_t o, bool live) {
  const int xd = ax - px(o), yd = ay - py(o);
  const bool off = xd == 0 || yd == 0;   // the reference's sign(0) = 0: block 0 on both axes
  const int xb = off ? 0 : floordiv20(xd > 0 ? xd - 10 : 10 - xd);
  const int yb = off ? 0 : floordiv20(yd > 0 ? yd - 10 : 10 - yd);
  const bool in = live && xb > -3 && xb < 3 && yb > -3 && yb < 3;
  const int cell = 16 + 5 * yb + xb;         // byte index 4 + (12 + 5 yb + xb)
  const uint32_t inc = in ? 1u << (8 * (cell & 3)) : 0u;
#pragma unroll
  for (int q = 1; q < BLK_WORDS; ++q) w8[q] += (cell >> 2) == q ? inc : 0u;
}

}  // namespace
