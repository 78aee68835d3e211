// abi.hip -- the step engine's host side: be_ctx, the config check, every C entry point of
// include/ballenv.h that steps, resets, observes or checkpoints envs, and the autoreset pool's
// entry points.  No kernels: which kernel a context runs is the dispatcher's answer (a Launch,
// step_types.h; csrc/ballenv.hip), and this unit decides from its description only.
#include <hip/hip_runtime.h>

#include <math.h>
#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <new>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ballenv.h"
#include "host_logic.h"
#include "internal.h"
#include "step_types.h"

using namespace bestep;
using namespace behost;

struct be_ctx {
  be_config cfg;
  TablesX tables;
  KParams base;      // config-derived part of every launch's KParams
  int device;
  StatusWord status;
  TablesX* d_tables;
  bool generic_only;   // BALLENV_GENERIC_KERNELS=1: never use the fixed-shape step kernels (A/B diagnostics)
  bool unit_moves;     // every action move in {-1,0,1}^2 (fixed-shape kernels' packed table)
  bool distinct_goals; // >= 2 pairwise-distinct goals (fixed-shape kernels' arithmetic newGoalList)
  int step_lanes;      // W = 10: lanes per env of the fixed step kernel (1: be_kernel; 2: step2_kernel)
  int step2_wide;      // BALLENV_STEP2_WIDE as read at create (-1: step2_wide()'s rule per call; 0 / 1: forced, A/B)
  int step_instance;   // which instance the last be_step / be_step_n launch took (STEP_INSTANCE_*; be_step_instance)
  int step5_lpe;       // W = 5: lanes per env of the fixed step kernel (1: be_kernel; 4 / 8: stepw_kernel)
  int roll5_lpe;       // W = 5: lanes per env of the fused rollout (1: rollout_kernel; 4 / 8: rolloutw_kernel)
  int max_lds;         // the device's LDS bytes per workgroup
  Launch step_launch[2];   // be_step's kernel without / with the fixed-shape preconditions (fixed per context)
  Launch step_launch_pool; // the fixed-shape kernel's pool variant (when the context has a pool)
  int64_t blob_hdr[8]; // be_save_state's header (host memory that outlives the async copy)
  // the autoreset pool (layout in pool_layout.h): allocated when be_step's fixed-shape kernel consumes it
  uint32_t* pool;      // nullptr: no pool (every reset inline)
  int64_t pool_bytes;
  Launch pool_fill;    // the pool's fill kernel for this window
  PoolBook book;       // the pool's owner state, and when be_step queues a fill
  mutable struct { const void* fn; int lds; bool ok; } lds_cache[16];  // fits_lds() answers per (kernel, dynamic LDS): the two rollouts and the block-policy
                                                                        // rollout's instances (up to 4 under forced-waves A/B runs); full: asked again per call
  mutable std::mutex lds_mu;                                    // guards lds_cache (const entries may race)
  char err[512];
};

// Does a fused kernel's LDS (static + this launch's dynamic bytes) fit one workgroup?  The fused
// rollouts' dynamic LDS grows with R = radius_obstacle + radius_agent (near lists, row-span
// table) and the config-5 kernel is within 72 B of the CU's 160 KB at the default R = 25, so a
// larger R must take the per-step fallback instead of failing the launch.
static bool fits_lds(const be_ctx* ctx, const Launch& L) {
  if (!L.fn && !L.fnm) return false;
  const void* fn = L.entry();
  std::lock_guard<std::mutex> lock(ctx->lds_mu);
  for (auto& c : ctx->lds_cache)
    if (c.fn == fn && c.lds == L.lds) return c.ok;
  hipFuncAttributes fa;
  bool ok = hipFuncGetAttributes(&fa, fn) == hipSuccess && (int64_t)fa.sharedSizeBytes + L.lds <= (int64_t)ctx->max_lds;
  for (auto& c : ctx->lds_cache)
    if (!c.fn) { c.fn = fn; c.lds = L.lds; c.ok = ok; break; }
  return ok;
}

// The context's part of the fixed-shape preconditions (the config's part: the dispatcher's).
static bool fixed_ok(const be_ctx* ctx) { return !ctx->generic_only && ctx->unit_moves && ctx->distinct_goals; }

// An A/B override of a lane count: the variable must be exactly one of `allowed`, else it is ignored.
static void env_lanes(const char* name, std::initializer_list<int> allowed, int& lanes) {
  const char* v = getenv(name);
  if (!v) return;
  for (const int a : allowed) {
    char text[8];
    snprintf(text, sizeof text, "%d", a);
    if (!strcmp(v, text)) lanes = a;
  }
}

static thread_local char g_err[512];

// library-internal accessors for the other translation units (csrc/internal.h)
char* be_ctx_err(be_ctx* ctx) { return ctx ? ctx->err : g_err; }
be_ctx_view be_ctx_get(const be_ctx* ctx) {
  be_ctx_view v;
  v.num_envs = ctx->cfg.num_envs; v.window = ctx->cfg.window; v.device = ctx->device;
  v.num_static = ctx->cfg.num_static; v.num_dynamic = ctx->cfg.num_dynamic;
  v.env_offset = ctx->cfg.env_offset;
  v.screen_width = ctx->cfg.screen_width; v.screen_height = ctx->cfg.screen_height;
  v.radius_obstacle = ctx->cfg.radius_obstacle; v.radius_agent = ctx->cfg.radius_agent;
  return v;
}
int be_ctx_check_state(be_ctx* ctx, const be_state* st) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  if (!st || !st->agent || !st->goal || !st->prev_dist || !st->total_dist || !st->ep_return || !st->ep_len ||
      !st->episode)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_state has a NULL pointer");
  if (ctx->cfg.num_static > 0 && !st->static_obs) return be_ctx_fail(ctx, BE_E_INVALID, "static_obs is NULL");
  if (ctx->cfg.num_dynamic > 0 && (!st->dyn_obs || !st->dyn_goal))
    return be_ctx_fail(ctx, BE_E_INVALID, "dyn_obs/dyn_goal is NULL");
  return BE_OK;
}

extern "C" {

int be_abi_version(void) { return BE_ABI_VERSION; }

int be_config_default(be_config* c, int32_t num_envs, int32_t window) {
  if (!c) return be_ctx_fail(nullptr, BE_E_INVALID, "cfg is NULL");
  memset(c, 0, sizeof(*c));
  c->num_envs = num_envs; c->window = window; c->env_offset = 0; c->seed = 0xBA11ull;
  c->screen_width = 500; c->screen_height = 500;                                     // ballenv_env.py:11-18
  c->strip_obs_x = 0; c->strip_obs_y = 20; c->strip_goal_x = 500; c->strip_goal_y = 20;
  c->strip_agent_x = 500; c->strip_agent_y = 10;
  c->radius_obstacle = 20; c->radius_agent = 5; c->speed_x = 1; c->speed_y = 1;     // :49-54
  c->threshold_goal = 10.0; c->time_penalty = 0.0; c->min_spawn_dist = 50.0;        // :64-65, :122
  c->num_static = 13; c->num_dynamic = 5; c->static_penalty = 1.0; c->dynamic_penalty = 8000.0;  // ball_cnn_ac3.py:40-51
  c->goal_change_step = 50; c->obs_certainty = 60;
  static const int goals[5][2] = {{12, 122}, {123, 93}, {87, 150}, {430, 440}, {230, 11}};
  c->num_goals = 5;
  for (int g = 0; g < 5; ++g) { c->goals[g][0] = goals[g][0]; c->goals[g][1] = goals[g][1]; }
  for (int k = 0; k < 5; ++k) c->obstacle_speed[k] = 1;
  static const int moves[9][2] = {{1, 1}, {1, -1}, {1, 0}, {0, 1}, {0, -1}, {0, 0}, {-1, 1}, {-1, 0}, {-1, -1}};
  c->num_actions = 9;                                                                // ball_cnn_ac3.py:530
  for (int a = 0; a < 9; ++a) { c->actions[a][0] = moves[a][0]; c->actions[a][1] = moves[a][1]; }
  c->time_limit = 1000; c->autoreset = 1;                                            // gym_ballenv/__init__.py:7
  return BE_OK;
}

int be_config_check(const be_config* c, char* msg, int32_t msg_len) {
  char buf[256] = {0};
#define BE_REQ(cond, text) do { if (!(cond)) { snprintf(buf, sizeof buf, "%s", text); goto bad; } } while (0)
  BE_REQ(c != nullptr, "cfg is NULL");
  BE_REQ(c->num_envs >= 1, "num_envs must be >= 1");
  BE_REQ(c->window >= 1 && c->window <= BE_MAX_WINDOW, "window must be in [1, 64]");
  BE_REQ(c->num_static >= 0 && c->num_static <= BE_MAX_STATIC, "num_static must be in [0, 64]");
  BE_REQ(c->num_dynamic >= 0 && c->num_dynamic <= BE_MAX_DYNAMIC, "num_dynamic must be in [0, 32]");
  BE_REQ(c->env_offset >= 0 && c->env_offset + (int64_t)c->num_envs <= (1ll << 32), "global env ids must fit in 32 bits");
  BE_REQ(c->screen_width >= 1 && c->screen_width <= 16384 && c->screen_height >= 1 && c->screen_height <= 16384,
         "screen size must be in [1, 16384]");
  BE_REQ(c->strip_goal_x >= 1 && c->strip_goal_x <= c->screen_width + 16384 && c->strip_goal_y >= 1 &&
         c->strip_goal_y <= c->screen_height + 16384, "goal strips must give non-empty randint ranges");
  BE_REQ(c->strip_agent_x >= 1 && c->strip_agent_x <= 16384 && c->strip_agent_y >= 1 && c->strip_agent_y <= 16384,
         "agent strips must give non-empty randint ranges");
  BE_REQ(c->screen_width - 2 * c->strip_obs_x >= 1 && c->screen_height - 2 * c->strip_obs_y >= 1,
         "obstacle strips must give non-empty randint ranges");
  BE_REQ(c->radius_obstacle >= 0 && c->radius_agent >= 0 && c->radius_obstacle + c->radius_agent <= 2047,
         "radii must be >= 0 with r_obstacle + r_agent <= 2047");
  BE_REQ(c->speed_x >= 1 && c->speed_y >= 1 && c->speed_x <= 1024 && c->speed_y <= 1024,
         "agent speeds (window cell steps) must be in [1, 1024]");
  BE_REQ(c->speed_x * (c->window / 2) <= 16384 && c->speed_y * (c->window / 2) <= 16384, "window too wide");
  BE_REQ(c->goal_change_step >= 0 && c->goal_change_step < (1 << 30), "goal_change_step out of range");
  BE_REQ(c->num_goals >= 0 && c->num_goals <= BE_MAX_GOALS, "num_goals must be in [0, 16]");
  BE_REQ(c->num_goals >= c->num_dynamic, "need a goal per dynamic obstacle (obs_goal_position)");
  BE_REQ(c->num_actions >= 1 && c->num_actions <= BE_MAX_ACTIONS, "num_actions must be in [1, 16]");
  for (int k = 0; k < c->num_dynamic; ++k)
    BE_REQ(c->obstacle_speed[k] >= -1024 && c->obstacle_speed[k] <= 1024, "obstacle speed out of range");
  for (int g = 0; g < c->num_goals; ++g)
    BE_REQ(c->goals[g][0] >= -16384 && c->goals[g][0] <= 16384 && c->goals[g][1] >= -16384 && c->goals[g][1] <= 16384,
           "goal coordinates out of range");
  for (int a = 0; a < c->num_actions; ++a)
    BE_REQ(c->actions[a][0] >= -1024 && c->actions[a][0] <= 1024 && c->actions[a][1] >= -1024 && c->actions[a][1] <= 1024,
           "action deltas out of range");
  BE_REQ(c->time_limit >= 0, "time_limit must be >= 0");
  BE_REQ(!(c->threshold_goal != c->threshold_goal), "threshold_goal is NaN");
  {  // int16 coordinates.  The reference's dynamic obstacles are unbounded Python ints (no clamp,
     // ballenv_env.py:334-347); here they are int16.  An obstacle spawns inside the obstacle strips
     // and moves at most |speed| per axis per step, and with autoreset and a time limit an episode
     // has at most time_limit moves, so the bound below holds for every episode and such a config
     // can never leave int16.  Without that bound (time_limit 0, or autoreset 0: a caller may step
     // past done) the kernels flag BE_STATUS_COORD_RANGE, the stored coordinate wraps (two's
     // complement int16) and the caller must poll be_status.
    int64_t ms = 0;
    for (int k = 0; k < c->num_dynamic; ++k) ms = std::max<int64_t>(ms, std::abs((int64_t)c->obstacle_speed[k]));
    const int64_t ex = std::max<int64_t>(std::abs((int64_t)c->strip_obs_x),
                                         std::abs((int64_t)c->screen_width - c->strip_obs_x));
    const int64_t ey = std::max<int64_t>(std::abs((int64_t)c->strip_obs_y),
                                         std::abs((int64_t)c->screen_height - c->strip_obs_y));
    BE_REQ(!(c->autoreset && c->time_limit > 0 && c->num_dynamic > 0) ||
               std::max(ex, ey) + ms * (int64_t)c->time_limit <= 32767,
           "dynamic obstacles can leave the int16 coordinate range within one episode: need "
           "max spawn extent + max|obstacle_speed| * time_limit <= 32767 (or time_limit 0 / autoreset 0 "
           "and poll status())");
  }
#undef BE_REQ
  if (msg && msg_len > 0) msg[0] = 0;
  return BE_OK;
bad:
  if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", buf);
  return be_fail(g_err, BE_E_INVALID, "invalid config: %s", buf);
}

// Can a reset re-sample the agent (ballenv_env.py:121-126, quirk Q9)?  Only if some agent spawn
// point lies closer than min_spawn_dist to some goal spawn point: with the reference's strips
// (agent y < 10, goal y >= 480) never.  When it cannot, prev_dist (state[2]) always equals
// calc_dist(goal, agent) -- after a step it is that distance, after a reset total_distance -- so
// the fixed-shape step kernels may recompute it instead of reading it (an A/B option, KParams).
static bool q9_possible(const be_config* c) {
  const int64_t dx = std::max<int64_t>(0, (int64_t)(c->screen_width - c->strip_goal_x) - (c->strip_agent_x - 1));
  const int64_t dy = std::max<int64_t>(0, (int64_t)(c->screen_height - c->strip_goal_y) - (c->strip_agent_y - 1));
  const double D = c->min_spawn_dist;
  return D > 0.0 && sqrt((double)(dx * dx + dy * dy)) < D;
}

int64_t be_step_bytes(const be_config* c) {
  if (!c) return 0;
  // agent R+W 8 | goal R 4 | prev_dist R+W 16 | total_dist R 8 | ep_return R+W 16 | ep_len R+W 8
  // | episode R 4 | action R 1 | reward W 8 | done W 1                                     = 74
  // | statics R 4*Ns | dyn xy R+W 8*Nd | dyn goal R 1*Nd | obs W 4+W^2
  return 74 + 4ll * c->num_static + 9ll * c->num_dynamic + 4 + (int64_t)c->window * c->window;
}

const char* be_last_error(const be_ctx* ctx) { return ctx ? ctx->err : g_err; }

const char* be_kernel_name(const be_ctx* ctx, int32_t entry) {
  static thread_local char name[48];
  if (!ctx) return nullptr;
  Launch L;
  switch (entry) {
    case BE_ENTRY_STEP_ACTIONS:   // (the pool variant when the context has a pool: its state's steps run it)
      L = pick_kernel(ctx->cfg, MODE_STEP, fixed_ok(ctx), ctx->step_lanes, ctx->step5_lpe, ctx->pool != nullptr);
      break;
    case BE_ENTRY_STEP_SAMPLED: L = pick_kernel(ctx->cfg, MODE_STEP, false); break;
    case BE_ENTRY_ROLLOUT: {
      L = pick_rollout(ctx->cfg, fixed_ok(ctx), ctx->roll5_lpe);
      const DeviceGuard dg(ctx->device);   // fits_lds queries the context's device
      if (dg.err != hipSuccess || !fits_lds(ctx, L)) return nullptr;
      break;
    }
    case BE_ENTRY_RESET: L = pick_kernel(ctx->cfg, MODE_RESET, false); break;
    case BE_ENTRY_OBSERVE: L = pick_kernel(ctx->cfg, MODE_OBSERVE, false); break;
    default: return nullptr;
  }
  if (!L.ok()) return nullptr;
  memcpy(name, L.name, sizeof name);
  return name;
}

int32_t be_step_instance(const be_ctx* ctx) { return ctx ? ctx->step_instance : STEP_INSTANCE_NONE; }

int64_t be_stats_slots(const be_config* c) {
  if (!c || c->num_envs < 1 || c->window < 1) return 0;
  // one slot per 32 envs: the fixed-shape kernels settle stats per half-wave (LPE 1) or per
  // wave (LPE 2), the generic ones per block (fewer slots, a prefix of these)
  return ((int64_t)c->num_envs + 31) / 32;
}

// Frees what a context holds on its device, and the context (the caller has entered the device).
static void ctx_release(be_ctx* ctx) {
  ctx->status.release();
  if (ctx->d_tables) (void)hipFree(ctx->d_tables);
  if (ctx->pool) (void)hipFree(ctx->pool);
  delete ctx;
}

int be_create(const be_config* cfg, int32_t device, be_ctx** out) {
  if (!out) return be_ctx_fail(nullptr, BE_E_INVALID, "out is NULL");
  *out = nullptr;
  char msg[256];
  if (be_config_check(cfg, msg, sizeof msg) != BE_OK) return be_fail(g_err, BE_E_INVALID, "invalid config: %s", msg);
  be_ctx* ctx = new (std::nothrow) be_ctx();
  if (!ctx) return be_ctx_fail(nullptr, BE_E_NOMEM, "out of host memory");
  ctx->cfg = *cfg;
  ctx->device = device;
  KParams& b = ctx->base;
  memset(&b, 0, sizeof b);
  b.n = cfg->num_envs; b.window = cfg->window; b.ns = cfg->num_static; b.nd = cfg->num_dynamic;
  b.R = cfg->radius_obstacle + cfg->radius_agent; b.speed_x = cfg->speed_x; b.speed_y = cfg->speed_y;
  b.screen_w = cfg->screen_width; b.screen_h = cfg->screen_height; b.goal_change = cfg->goal_change_step;
  b.certainty = cfg->obs_certainty; b.time_limit = cfg->time_limit; b.num_actions = cfg->num_actions;
  b.autoreset = cfg->autoreset; b.gid0 = (int32_t)(uint32_t)cfg->env_offset;
  b.threshold_goal = cfg->threshold_goal; b.time_penalty = cfg->time_penalty;
  b.static_penalty = cfg->static_penalty; b.dynamic_penalty = cfg->dynamic_penalty;
  b.min_spawn_dist = cfg->min_spawn_dist; b.seed = cfg->seed;
  b.num_goals = cfg->num_goals;
  // prev_dist is read: recomputing it (possible when q9_possible() is false) measured slower, the
  // f64 sqrt lands on the reward's chain (step2 6.52 vs 6.38 us, stepw 4.36 vs 4.20 us, A/B in one
  // process, profiles/r03_prev_dist_ab.txt); BALLENV_PREV_READ=0 selects it where it is exact (A/B)
  b.prev_read = 1;
  if (const char* r = getenv("BALLENV_PREV_READ")) { if (!strcmp(r, "0") && !q9_possible(cfg)) b.prev_read = 0; }
  ctx->unit_moves = cfg->num_actions <= 16;
  for (int a = 0; a < cfg->num_actions && a < 16; ++a) {
    const int mx = cfg->actions[a][0], my = cfg->actions[a][1];
    if (mx < -1 || mx > 1 || my < -1 || my > 1) ctx->unit_moves = false;
    else { b.amx |= (uint32_t)(mx + 1) << (2 * a); b.amy |= (uint32_t)(my + 1) << (2 * a); }
  }
  ctx->distinct_goals = cfg->num_goals >= 2;
  for (int g = 0; g < cfg->num_goals; ++g)
    for (int h = 0; h < g; ++h)
      if (cfg->goals[g][0] == cfg->goals[h][0] && cfg->goals[g][1] == cfg->goals[h][1]) ctx->distinct_goals = false;
  {  // smallest integer n with sqrt(n) >= min_spawn_dist (f64, correctly rounded: monotone in n)
    const double D = cfg->min_spawn_dist;
    long long n = D <= 0.0 ? 0 : (long long)ceil(D * D);
    if (n > (1ll << 30)) n = 1ll << 30;
    while (n > 0 && sqrt((double)(n - 1)) >= D) --n;
    while (n < (1ll << 30) && sqrt((double)n) < D) ++n;
    b.min_spawn_d2 = (int32_t)n;
  }
  b.inv_g1 = 1.0 / ((double)cfg->goal_change_step + 1.0);
  if (const char* d = getenv("BALLENV_DEBUG_SKIP")) b.dbg = (int32_t)strtoul(d, nullptr, 0);
  if (const char* g = getenv("BALLENV_GENERIC_KERNELS")) ctx->generic_only = atoi(g) != 0;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
  {  // Two lanes per env (step2_kernel) shorten each wave's dependent chain where one lane per env
     // leaves at most ~1.5 waves per SIMD; past that the one-lane kernel has the waves to hide its
     // latency and the pair's duplicated per-env work costs more than it saves (measured on MI355X,
     // 256 CUs: step2 6.42 / 7.51 us at 65 536 / 98 304 envs against 6.97 / 7.92; one lane 8.13 /
     // 14.5 / 48.9 us at 131 072 / 262 144 / 2^20 against 8.54 / 16.2 / 52.6).
     // BALLENV_STEP_LPE=1 / 2 forces one or two lanes (A/B).
    ctx->step_lanes = (int64_t)cfg->num_envs > (int64_t)96 * 4 * cus ? 1 : 2;
  }
  // W = 5 (BASELINE config 2): stepw_kernel's 8 lanes per env while one lane per env would leave
  // most of the chip idle (<= 64 envs per CU), the one-lane kernel above that.
  ctx->step5_lpe = (int64_t)cfg->num_envs <= (int64_t)64 * cus ? 8 : 1;
  ctx->roll5_lpe = ctx->step5_lpe;
  env_lanes("BALLENV_ROLLOUT5_LPE", {1, 4, 8}, ctx->roll5_lpe);   // (the rollout does not follow BALLENV_STEP5_LPE)
  env_lanes("BALLENV_STEP5_LPE", {1, 4, 8}, ctx->step5_lpe);
  // (four lanes per env, step2_kernel<10, 13, 5, 4, 128> of commit b0bc389, was bit-exact but slower
  // at every size: 6.08 vs 5.28 us at 32 768 envs, profiles/r04_w10_lanes_2_4.jsonl)
  env_lanes("BALLENV_STEP_LPE", {1, 2}, ctx->step_lanes);
  ctx->step2_wide = step2_wide_env(getenv("BALLENV_STEP2_WIDE"));   // (A/B and the tests: forces either instance)
  if (hipDeviceGetAttribute(&ctx->max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess ||
      ctx->max_lds <= 0)
    ctx->max_lds = 65536;
  memset(&ctx->tables, 0, sizeof ctx->tables);
  Tables& t = ctx->tables.t;
  for (int k = 0; k < cfg->num_dynamic; ++k) t.speed[k] = cfg->obstacle_speed[k];
  t.strip_obs_x = cfg->strip_obs_x; t.strip_obs_y = cfg->strip_obs_y;
  t.strip_goal_x = cfg->strip_goal_x; t.strip_goal_y = cfg->strip_goal_y;
  t.strip_agent_x = cfg->strip_agent_x; t.strip_agent_y = cfg->strip_agent_y;
  t.radius_obstacle = cfg->radius_obstacle; t.radius_agent = cfg->radius_agent;
  for (int g = 0; g < cfg->num_goals; ++g)
    t.goal[g] = (int32_t)(((uint32_t)cfg->goals[g][0] & 0xFFFFu) | ((uint32_t)cfg->goals[g][1] << 16));
  for (int a = 0; a < cfg->num_actions; ++a)
    t.action[a] = (int32_t)(((uint32_t)cfg->actions[a][0] & 0xFFFFu) | ((uint32_t)cfg->actions[a][1] << 16));
  for (int g = 0; g < cfg->num_goals; ++g) {  // newGoalList, ballenv_env.py:351
    int n = 0;
    for (int q = 0; q < cfg->num_goals; ++q)
      if (cfg->goals[q][0] != cfg->goals[g][0] || cfg->goals[q][1] != cfg->goals[g][1]) t.other[g][n++] = (uint8_t)q;
    t.n_other[g] = (uint8_t)n;
  }
  const int R = cfg->radius_obstacle + cfg->radius_agent;
  for (int d = 0; d <= R && d <= HW_MAX; ++d) {   // exact integer sqrt
    int h = 0;
    while ((h + 1) * (h + 1) <= R * R - d * d) ++h;
    t.hw[d] = (uint8_t)h;
  }
  if (span_fits(cfg->window, R)) {   // step2_kernel's row-span table (TablesX)
    const int W = cfg->window, C = W - 1 + R, J0 = R + W - 2;   // K = W-1 rows
    for (int j = 0; j < SPAN_N; ++j) {
      const int a = abs(j - J0), hw = a <= R ? t.hw[a] : 0;
      ctx->tables.span[j] = a <= R && j <= 2 * J0 ? ((2ull << (2 * hw)) - 1ull) << (C - hw) : 0ull;
    }
  }
  const DeviceGuard dg(device);   // the caller's current device is restored on return
  hipError_t e = dg.err;
  if (e == hipSuccess) e = ctx->status.create();
  if (e == hipSuccess) e = hipMalloc(&ctx->d_tables, sizeof(TablesX));
  if (e == hipSuccess) e = hipMemcpy(ctx->d_tables, &ctx->tables, sizeof(TablesX), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  // be_step's two possible kernels, picked once (pick_kernel formats a name: not per launch)
  ctx->step_launch[0] = pick_kernel(ctx->cfg, MODE_STEP, false, ctx->step_lanes, ctx->step5_lpe);
  ctx->step_launch[1] = pick_kernel(ctx->cfg, MODE_STEP, true, ctx->step_lanes, ctx->step5_lpe);
  {  // the autoreset pool, for the fixed-shape kernels that consume it (two lanes, L lanes, the one-lane kernel)
    const Launch& fixed = ctx->step_launch[1];
    int64_t onelane_max = (int64_t)2 * 64 * 4 * cus;   // BALLENV_POOL_ONELANE_MAX: the bound below, for A/B runs
    if (const char* v = getenv("BALLENV_POOL_ONELANE_MAX")) onelane_max = atoll(v);
    // the one-lane kernel up to two waves per SIMD: 7.51-7.59 against 7.76-7.85 us at 131 072 envs; at
    // 262 144 (four waves per SIMD hide the reset draws, and the fill costs more) 14.11-14.24 against
    // 13.71-13.72 (profiles/r06_onelane_pool_ab.txt)
    const bool consumes = fixed_ok(ctx) && cfg->autoreset && fixed.consumes_pool &&
                          (fixed.kind != KIND_FIXED1 || (int64_t)cfg->num_envs <= onelane_max);
    const bool want = consumes && (int64_t)cfg->num_envs <= POOL_MAX_ENVS && PoolBook::env_enabled();
    ctx->book.period_from_env();
    if (want && e == hipSuccess) {
      ctx->pool_bytes = pool_bytes_per_env(FIX_NS, FIX_ND) * cfg->num_envs;
      ctx->pool_fill = pick_pool_fill(cfg->window);
      e = be_pool_alloc(&ctx->pool, ctx->pool_bytes);
      ctx->book.has = e == hipSuccess;
      ctx->step_launch_pool = pick_kernel(ctx->cfg, MODE_STEP, true, ctx->step_lanes, ctx->step5_lpe, true);
    }
  }
  if (e != hipSuccess) {
    ctx_release(ctx);
    return be_fail(g_err, BE_E_HIP, "HIP error in be_create: %s", hipGetErrorString(e));
  }
  *out = ctx;
  return BE_OK;
}

int be_destroy(be_ctx* ctx) {
  if (!ctx) return BE_OK;
  const DeviceGuard dg(ctx->device);   // the caller's current device is restored on return
  ctx_release(ctx);
  return BE_OK;
}

// Per-call KParams: the context's config part + this call's pointers.
static KParams make_params(be_ctx* ctx, const be_state* st, const be_out* out) {
  KParams a = ctx->base;
  a.agent = st->agent; a.goal = st->goal; a.prev_dist = st->prev_dist; a.total_dist = st->total_dist;
  a.ep_return = st->ep_return; a.ep_len = st->ep_len; a.episode = st->episode; a.static_obs = st->static_obs;
  a.dyn_obs = st->dyn_obs; a.dyn_goal = st->dyn_goal;
  if (out) {
    a.obs = out->obs; a.obs_f32 = out->obs_f32; a.reward = out->reward; a.done = out->done;
    a.truncated = out->truncated; a.terminal_obs = out->terminal_obs; a.final_return = out->final_return;
    a.final_len = out->final_len; a.stats = out->stats;
  }
  a.tables = &ctx->d_tables->t;
  a.status = ctx->status.word;
  return a;
}

// An obs-only launch (be_reset, be_observe) writes none of a step's outputs.
static void obs_only(KParams& a) {
  a.reward = nullptr; a.done = nullptr; a.truncated = nullptr; a.terminal_obs = nullptr;
  a.final_return = nullptr; a.final_len = nullptr; a.stats = nullptr;
}

// The pool's fill over every env of the state (its caller has claimed the pool or found the fill due)
static void launch_pool_fill(be_ctx* ctx, const KParams& a, void* stream) {
  KParams f = a;
  f.pool = ctx->pool;
  launch_kernel(ctx->pool_fill, f, (hipStream_t)stream);
}

// The launches of one entry point, which has entered the context's device.  steps > 1 (be_step_n):
// `steps` launches of the same kernel, actions advancing by N per step.
static int launch(be_ctx* ctx, int mode, KParams& a, void* stream, int32_t steps = 1) {
  const bool fixed = mode == MODE_STEP && a.tape == nullptr && a.actions != nullptr && fixed_ok(ctx);
  if (((uintptr_t)a.obs & 15) || ((uintptr_t)a.obs_f32 & 15))
    return be_ctx_fail(ctx, BE_E_INVALID, "obs / obs_f32 must be 16-byte aligned");
  // the pool serves one state (PoolBook, host_logic.h): a step of any other state draws its resets inline
  const bool use_pool = fixed && ctx->book.step(a.episode);
  a.pool = use_pool ? ctx->pool : nullptr;
  const Launch L = mode == MODE_STEP ? (use_pool ? ctx->step_launch_pool : ctx->step_launch[fixed ? 1 : 0])
                                     : pick_kernel(ctx->cfg, mode);
  const int N = ctx->cfg.num_envs;
  // step2_kernel's wide-row-load instance, by this call's state: whole waves, 16-byte aligned obstacle arrays
  const bool wide = L.fn2_wide && a.prev_read && step2_wide(N, a.static_obs, a.dyn_obs, a.dyn_goal, ctx->step2_wide);
  if (mode == MODE_STEP) ctx->step_instance = wide ? STEP_INSTANCE_WIDE : STEP_INSTANCE_PLAIN;
  for (int32_t s = 0; s < steps; ++s) {
    launch_kernel(L, a, (hipStream_t)stream, wide);
    a.actions += N;
    if (use_pool && ctx->book.fill_due()) launch_pool_fill(ctx, a, stream);
  }
  return be_launched(ctx->err);
}

// be_reset, be_load_state, be_pool_fill: st becomes the pool's state, with its next two episodes per env drawn
static int claim_and_fill(be_ctx* ctx, const be_state* st, void* stream) {
  if (!ctx->pool) return BE_OK;
  ctx->book.claim(st->episode);
  launch_pool_fill(ctx, make_params(ctx, st, nullptr), stream);
  return be_launched(ctx->err);
}

int be_reset(be_ctx* ctx, const be_state* st, const uint8_t* mask, const int16_t* reset_tape, int32_t tape_len,
             const be_out* out, void* stream) {
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (reset_tape && tape_len < 0) return be_ctx_fail(ctx, BE_E_INVALID, "tape_len < 0");
  if (!out || (!out->obs && !out->obs_f32)) return be_ctx_fail(ctx, BE_E_INVALID, "be_reset needs out->obs or out->obs_f32");
  KParams a = make_params(ctx, st, out);
  obs_only(a);
  a.mask = mask; a.reset_tape = reset_tape; a.reset_tape_len = reset_tape ? tape_len : 0;
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  if (int rc = launch(ctx, MODE_RESET, a, stream)) return rc;
  return claim_and_fill(ctx, st, stream);   // ahead of this state's first step
}

int be_step(be_ctx* ctx, const be_state* st, const uint8_t* actions, const int16_t* action_deltas,
            const int16_t* draw_tape, const be_out* out, void* stream) {
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (!out || !out->reward || !out->done) return be_ctx_fail(ctx, BE_E_INVALID, "be_step needs out->reward and out->done");
  if (draw_tape && ctx->cfg.autoreset) return be_ctx_fail(ctx, BE_E_INVALID, "draw tapes (parity mode) need autoreset = 0");
  KParams a = make_params(ctx, st, out);
  a.actions = actions; a.deltas = action_deltas; a.tape = draw_tape;
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  return launch(ctx, MODE_STEP, a, stream);
}

int be_step_n(be_ctx* ctx, const be_state* st, const uint8_t* actions, int32_t steps, const be_out* out,
              void* stream) {
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (!actions || steps < 0) return be_ctx_fail(ctx, BE_E_INVALID, "be_step_n needs actions and steps >= 0");
  if (!out || !out->reward || !out->done) return be_ctx_fail(ctx, BE_E_INVALID, "be_step_n needs out->reward and out->done");
  if (steps == 0) return BE_OK;
  KParams a = make_params(ctx, st, out);
  a.actions = actions;
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  return launch(ctx, MODE_STEP, a, stream, steps);
}

int be_rollout(be_ctx* ctx, const be_state* st, const uint8_t* actions, int32_t steps, const be_out* out,
               void* stream) {
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (!actions || steps < 0) return be_ctx_fail(ctx, BE_E_INVALID, "be_rollout needs actions and steps >= 0");
  if (!out || !out->obs || !out->reward || !out->done)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_rollout needs out->obs, out->reward and out->done");
  if (out->obs_f32) return be_ctx_fail(ctx, BE_E_INVALID, "be_rollout writes u8 obs only (obs_f32 must be NULL)");
  const int64_t N = ctx->cfg.num_envs, F = 4 + (int64_t)ctx->cfg.window * ctx->cfg.window;
  if (((uintptr_t)out->obs & 15) || (N * F) % 16)
    return be_ctx_fail(ctx, BE_E_INVALID, "be_rollout needs a 16-byte aligned obs and num_envs * (4+W*W) % 16 == 0");
  if (steps == 0) return BE_OK;
  const Launch L = pick_rollout(ctx->cfg, fixed_ok(ctx), ctx->roll5_lpe);
  BE_ENTER_DEVICE(ctx->err, ctx->device);   // (fits_lds queries the function's attributes on the context's device)
  if (fits_lds(ctx, L)) {
    KParams a = make_params(ctx, st, out);
    a.actions = actions; a.steps = steps;
    launch_kernel(L, a, (hipStream_t)stream);
    return be_launched(ctx->err);
  }
  // any other config: one step launch per step into the (steps, N, ...) slices (same results)
  for (int32_t s = 0; s < steps; ++s) {
    const be_out o = be_out_at(*out, s, N, F);
    KParams a = make_params(ctx, st, &o);
    a.actions = actions + s * N;
    if (int rc = launch(ctx, MODE_STEP, a, stream)) return rc;
  }
  return BE_OK;
}

}  // extern "C"

int be_internal_policy_rollout(be_ctx* ctx, const be_state* st, const be_pol_rollout_args* r, void* stream) {
  const Launch L = pick_policy_rollout(ctx->cfg, fixed_ok(ctx), r->HT, r->KS, r->NO);
  if (!fits_lds(ctx, L)) return 0;   // the caller loops select_action + be_step instead
  KParams a = make_params(ctx, st, r->out);
  a.steps = r->steps;
  a.pol_bytes = r->img_bytes; a.pol_actions = r->num_actions; a.pol_img = r->img; a.pol_seed = r->seed;
  a.obs_in = r->obs_in; a.obs_last = r->obs_last;
  a.act_out = r->act->action; a.logp_out = r->act->log_prob; a.value_out = r->act->value;
  launch_kernel(L, a, (hipStream_t)stream);
  const int rc = be_launched(ctx->err);
  return rc ? rc : 1;
}

int be_internal_mlp_rollout(be_ctx* ctx, const be_state* st, const be_mlp_rollout_args* r, void* stream) {
  const Launch L = pick_mlp_rollout(ctx->cfg, fixed_ok(ctx), r->layers, r->waves);
  if (!fits_lds(ctx, L)) return 0;   // the caller loops be_mlp_act + be_step instead
  KParams a = make_params(ctx, st, r->out);
  a.steps = r->steps;
  const MlpRollParams q{r->img, r->blocks_out, r->act->action, r->act->log_prob, r->seed, r->num_actions, r->final_relu};
  launch_mlp_rollout(L, a, q, (hipStream_t)stream);
  if (int rc = be_launched(ctx->err)) return rc;
  // the window obs of the final state, as the loop's last be_step leaves it: what be_observe writes
  const be_out last{r->obs_last, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  KParams o = make_params(ctx, st, &last);
  obs_only(o);
  const int rc = launch(ctx, MODE_OBSERVE, o, stream);
  return rc ? rc : 1;
}

const char* be_internal_mlp_rollout_name(be_ctx* ctx, int32_t layers, int32_t waves) {
  static thread_local char name[48];
  const Launch L = pick_mlp_rollout(ctx->cfg, fixed_ok(ctx), layers, waves);
  const DeviceGuard dg(ctx->device);   // fits_lds queries the context's device
  if (dg.err != hipSuccess || !fits_lds(ctx, L)) return nullptr;
  memcpy(name, L.name, sizeof name);
  return name;
}

extern "C" {

int be_observe(be_ctx* ctx, const be_state* st, const be_out* out, void* stream) {
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (!out || (!out->obs && !out->obs_f32)) return be_ctx_fail(ctx, BE_E_INVALID, "be_observe needs out->obs or out->obs_f32");
  KParams a = make_params(ctx, st, out);
  obs_only(a);
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  return launch(ctx, MODE_OBSERVE, a, stream);
}

int be_sample_actions(be_ctx* ctx, uint8_t* actions_out, int32_t steps, uint64_t seed, void* stream) {
  if (!ctx || !actions_out || steps < 0) return be_ctx_fail(ctx, BE_E_INVALID, "bad arguments to be_sample_actions");
  if (steps == 0) return BE_OK;
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  launch_sample_actions(actions_out, ctx->cfg.num_envs, steps, ctx->cfg.env_offset, ctx->cfg.num_actions,
                        (unsigned long long)seed, (hipStream_t)stream);
  return be_launched(ctx->err);
}

// ---- env-state checkpoint (the blob's layout and header: host_logic.h)
int64_t be_state_blob_bytes(const be_config* cfg) {
  if (!cfg || cfg->num_envs < 1) return 0;
  return blob_layout(cfg).total;
}

int be_save_state(be_ctx* ctx, const be_state* st, void* blob, void* stream) {
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (!blob) return be_ctx_fail(ctx, BE_E_INVALID, "blob is NULL");
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  const BlobLayout L = blob_layout(&ctx->cfg);
  blob_header(&ctx->cfg, L.total, ctx->blob_hdr);   // lives in the context: safe for an async copy
  hipStream_t s = (hipStream_t)stream;
  BE_HIP_TRY(ctx->err, hipMemcpyAsync(blob, ctx->blob_hdr, sizeof ctx->blob_hdr, hipMemcpyDefault, s));
  void* src[10];
  state_ptrs(st, src);
  for (int k = 0; k < 10; ++k)
    if (L.bytes[k] > 0)
      BE_HIP_TRY(ctx->err, hipMemcpyAsync(static_cast<char*>(blob) + L.off[k], src[k], (size_t)L.bytes[k], hipMemcpyDefault, s));
  return BE_OK;
}

int be_load_state(be_ctx* ctx, const be_state* st, const void* blob, void* stream) {
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (!blob) return be_ctx_fail(ctx, BE_E_INVALID, "blob is NULL");
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  const BlobLayout L = blob_layout(&ctx->cfg);
  hipStream_t s = (hipStream_t)stream;
  int64_t got[8], want[8];
  BE_HIP_TRY(ctx->err, hipMemcpyAsync(got, blob, sizeof got, hipMemcpyDefault, s));
  BE_HIP_TRY(ctx->err, hipStreamSynchronize(s));
  blob_header(&ctx->cfg, L.total, want);
  if (memcmp(got, want, sizeof got) != 0)
    return be_ctx_fail(ctx, BE_E_INVALID, "state blob header does not match this context (magic, ABI, N, Ns, Nd)");
  void* dst[10];
  state_ptrs(st, dst);
  for (int k = 0; k < 10; ++k)
    if (L.bytes[k] > 0)
      BE_HIP_TRY(ctx->err, hipMemcpyAsync(dst[k], static_cast<const char*>(blob) + L.off[k], (size_t)L.bytes[k], hipMemcpyDefault, s));
  // the loaded episodes' next entries (the pool's entries need no invalidation: each is a pure
  // function of (seed, global id, episode) and is checked by its tag)
  return claim_and_fill(ctx, st, stream);
}

int be_pool_fill(be_ctx* ctx, const be_state* st, void* stream) {
  if (int rc = be_ctx_check_state(ctx, st)) return rc;
  if (!ctx->pool) return BE_OK;
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  return claim_and_fill(ctx, st, stream);
}

int be_pool_invalidate(be_ctx* ctx, void* stream) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  if (!ctx->pool) return BE_OK;
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  BE_HIP_TRY(ctx->err, hipMemsetAsync(ctx->pool, 0, (size_t)ctx->pool_bytes, (hipStream_t)stream));
  return BE_OK;
}

int be_pool_set_period(be_ctx* ctx, int32_t period) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  if (period < 0) return be_ctx_fail(ctx, BE_E_INVALID, "pool period must be >= 0");
  ctx->book.set_period(period);
  return BE_OK;
}

int64_t be_pool_bytes(const be_ctx* ctx) { return ctx && ctx->pool ? ctx->pool_bytes : 0; }

int32_t be_pool_period(const be_ctx* ctx) { return ctx ? ctx->book.period : 0; }

int be_pool_entry(be_ctx* ctx, int32_t env, int32_t slot, uint32_t* words, double* f64, int32_t write) {
  if (!ctx) return be_ctx_fail(nullptr, BE_E_INVALID, "ctx is NULL");
  if (!ctx->pool) return be_ctx_fail(ctx, BE_E_INVALID, "this context has no autoreset pool");
  if (env < 0 || env >= ctx->cfg.num_envs || slot < 0 || slot > 1 || !words || !f64)
    return be_ctx_fail(ctx, BE_E_INVALID, "bad arguments to be_pool_entry");
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  BE_HIP_TRY(ctx->err, hipDeviceSynchronize());
  // the entry's tag and body (pool_layout.h) from / to the header's word order (host_logic.h)
  const int64_t n = ctx->cfg.num_envs, x = (int64_t)slot * n + env;
  constexpr int NBW = pool_body_words(FIX_NS, FIX_ND), NO = FIX_NS + FIX_ND;
  char* tv = reinterpret_cast<char*>(ctx->pool) + x * 8;
  char* body = reinterpret_cast<char*>(ctx->pool) + 16 * n + x * 4 * NBW;
  uint32_t t[2], b[NBW];
  BE_HIP_TRY(ctx->err, hipMemcpy(t, tv, sizeof t, hipMemcpyDeviceToHost));
  BE_HIP_TRY(ctx->err, hipMemcpy(b, body, sizeof b, hipMemcpyDeviceToHost));
  if (!write) {
    pool_entry_unpack(t, b, NO, words, f64);
    return BE_OK;
  }
  pool_entry_pack(words, f64, NO, t, b);
  BE_HIP_TRY(ctx->err, hipMemcpy(tv, t, sizeof t, hipMemcpyHostToDevice));
  BE_HIP_TRY(ctx->err, hipMemcpy(body, b, sizeof b, hipMemcpyHostToDevice));
  return BE_OK;
}

int be_status(be_ctx* ctx, int32_t* status_out, void* stream) {
  if (!ctx || !status_out) return be_ctx_fail(ctx, BE_E_INVALID, "bad arguments to be_status");
  BE_ENTER_DEVICE(ctx->err, ctx->device);
  BE_HIP_TRY(ctx->err, ctx->status.take(stream, status_out));
  return BE_OK;
}

}  // extern "C"
