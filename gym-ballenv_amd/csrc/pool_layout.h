// pool_layout.h -- the autoreset pool's layout.  No HIP in it: step_types.h includes it for the
// kernels and the dispatcher, host_logic.h for be_pool_entry's word order.
#pragma once
#include <stdint.h>

namespace bestep {

// A reset in Philox mode is a pure function of (seed, global env id, new episode) and the context's
// config (reset_env_philox's counter layout), so it can be drawn before the env finishes.
// pool_fill_kernel draws, for every env at episode e, the resets into episodes e+1 and e+2; the step
// kernels (step2_kernel, stepw_kernel) copy the entry of episode e+1 when the env finishes, instead
// of running the reset's Philox chains on the wave's critical path, and fall back to the inline
// wave_resets pass when the entry is stale (its tag is not e+1: the env reset twice since the last
// fill, or no fill ran).  Two entries per env, slot = episode & 1 (entry index x = slot * N + env),
// everything addressed from the one base p.pool (a uniform pointer + a 32-bit byte offset + an
// immediate: no per-array base pointers to keep in SGPRs):
//   tags    uint2 [2N] at byte 0:      (the episode the entry resets into, flags: POOL_VALID written,
//                                      POOL_REJ a rejection loop hit its bound) -- the fill's scan
//                                      reads these 8 bytes per entry, coalesced
//   bodies  112 B [2N] at byte 16 N:   the entry itself, contiguous (a consuming lane reads it with
//                                      seven 16-byte loads):
//     w0..2  ROWS: the reset obs's distinct window rows, packed as the consuming kernel ORs them
//            (W = 10: three rows per word at bits 10 r; W = 5: four rows at bits 5 r, in w0)
//     w3 AGENT, w4 GOAL (packed xy), w5 unused, w6..7 PREV f64 (state[2], the pre-resample distance,
//     Q9), w8..9 TOTAL f64, w10.. the NS statics' then the ND dynamics' packed xy (a reset's dyn_goal
//     is k)
constexpr uint32_t POOL_VALID = 1u, POOL_REJ = 2u;
constexpr int PB_ROWS = 0, PB_AGENT = 3, PB_GOAL = 4, PB_PREV = 6, PB_TOTAL = 8, PB_OBS = 10;
constexpr int pool_body_words(int ns, int nd) { return (PB_OBS + ns + nd + 3) & ~3; }   // (host and device)
constexpr int64_t pool_bytes_per_env(int ns, int nd) { return 2 * (8 + 4ll * pool_body_words(ns, nd)); }
static_assert(pool_body_words(13, 5) == 28, "the fixed-shape kernels' 112-byte entry body");
constexpr int64_t POOL_MAX_ENVS = 1ll << 22;

}  // namespace bestep
