// Stand-alone check of csrc/host_logic.h: the host logic of libballenv.so that needs no HIP, built by
// the host C++ compiler alone under ASan + UBSan (tests/test_host_logic.py).  Prints one OK line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>

#include "host_logic.h"

using namespace behost;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

// One step launch of `state` that meets the pool's preconditions, as both engines book it:
// *used = the launch ran the pool instance; returns whether a fill was queued after it.
static bool step(PoolBook& b, const void* state, bool* used = nullptr) {
  const bool use = b.step(state);
  if (used) *used = use;
  return use && b.fill_due();
}

static void test_pool_book() {
  uint32_t ep_a[1], ep_b[1];   // two states' episode arrays: only their addresses matter
  bool used = false;
  {  // no pool: nothing is claimed, used or due
    PoolBook b;
    b.set_period(1);
    CHECK(!step(b, ep_a, &used) && !used && b.owner == nullptr);
  }
  PoolBook b;
  b.has = true;
  b.set_period(3);
  CHECK(b.owner == nullptr);
  // the first state stepped becomes the owner; fills fall due after its 3rd and 6th steps only
  for (int s = 1; s <= 8; ++s) {
    const bool fill = step(b, ep_a, &used);
    CHECK(used && b.owner == ep_a);
    CHECK(fill == (s == 3 || s == 6));
    // a second state's steps neither use the pool nor count towards the period
    const int calls = b.calls;
    CHECK(!step(b, ep_b, &used) && !used);
    CHECK(b.owner == ep_a && b.calls == calls);
  }
  CHECK(b.calls == 2);
  // a reset / load / fill for the second state moves ownership and restarts the count
  b.claim(ep_b);
  CHECK(b.owner == ep_b && b.calls == 0);
  CHECK(!step(b, ep_a, &used) && !used);      // the first state's later steps go without the pool
  CHECK(b.calls == 0);
  CHECK(!step(b, ep_b, &used) && used);
  CHECK(!step(b, ep_b, &used) && used && b.calls == 2);
  // setting the period zeroes the count
  b.set_period(2);
  CHECK(b.period == 2 && b.calls == 0);
  CHECK(!step(b, ep_b));
  CHECK(step(b, ep_b) && b.calls == 0);       // a due fill zeroes it too
  CHECK(!step(b, ep_b) && b.calls == 1);
  b.claim(ep_b);                              // and so does a claim that fills (same owner)
  CHECK(b.owner == ep_b && b.calls == 0);
  // period 0: explicit fills only
  b.set_period(0);
  for (int s = 0; s < 1000; ++s) CHECK(!step(b, ep_b, &used) && used);

  // the environment, as be_create and be_board_create read it
  unsetenv("BALLENV_POOL");
  unsetenv("BALLENV_POOL_PERIOD");
  PoolBook e;
  CHECK(PoolBook::env_enabled());
  e.period_from_env();
  CHECK(e.period == 128);
  const struct { const char* text; bool enabled; } pools[] = {{"0", false}, {"1", true}, {"", true}, {"00", true}, {"no", true}};
  for (const auto& c : pools) {
    setenv("BALLENV_POOL", c.text, 1);
    CHECK(PoolBook::env_enabled() == c.enabled);
  }
  const struct { const char* text; int period; } periods[] = {{"1", 1}, {"64", 64}, {"0", 0}, {"-5", 0}, {"abc", 0}, {"7x", 7}};
  for (const auto& c : periods) {
    setenv("BALLENV_POOL_PERIOD", c.text, 1);
    e.calls = 5;
    e.period_from_env();
    CHECK(e.period == c.period);
  }
  unsetenv("BALLENV_POOL");
  unsetenv("BALLENV_POOL_PERIOD");
}

static void test_blob() {
  const int shapes[3][3] = {{1, 0, 0}, {3, 1, 1}, {65, 13, 5}};
  for (const auto& sh : shapes) {
    be_config c;
    memset(&c, 0, sizeof c);
    c.num_envs = sh[0]; c.num_static = sh[1]; c.num_dynamic = sh[2];
    const int64_t N = sh[0], ns = sh[1], nd = sh[2];
    // be_state's order: agent, goal (i32) | prev_dist, total_dist, ep_return (f64) | ep_len, episode (i32)
    // | static_obs (Ns, N) i32 | dyn_obs (Nd, N) i32 | dyn_goal (Nd, N) u8
    const int64_t want[10] = {4 * N, 4 * N, 8 * N, 8 * N, 8 * N, 4 * N, 4 * N, 4 * ns * N, 4 * nd * N, nd * N};
    const BlobLayout L = blob_layout(&c);
    int64_t end = 64;                          // the header is 64 bytes
    for (int k = 0; k < 10; ++k) {
      CHECK(L.bytes[k] == want[k]);
      CHECK(L.off[k] % 16 == 0);
      CHECK(L.off[k] >= end && L.off[k] - end < 16);   // in order, no overlap, padding below one line
      end = L.off[k] + L.bytes[k];
    }
    CHECK(L.off[0] == 64);
    CHECK(L.total % 16 == 0 && L.total >= end && L.total - end < 16);
    int64_t hdr[8];
    blob_header(&c, L.total, hdr);
    CHECK(sizeof hdr == 64 && memcmp(&hdr[0], "BALLENV1", 8) == 0);
    CHECK(hdr[1] == BE_ABI_VERSION && hdr[2] == N && hdr[3] == ns && hdr[4] == nd && hdr[5] == L.total);
    CHECK(hdr[6] == 0 && hdr[7] == 0);
  }
  int32_t a[10];
  be_state st{a + 0, a + 1, (double*)(a + 2), (double*)(a + 3), (double*)(a + 4), a + 5, (uint32_t*)(a + 6), a + 7, a + 8,
              (uint8_t*)(a + 9)};
  void* p[10];
  state_ptrs(&st, p);
  for (int k = 0; k < 10; ++k) CHECK(p[k] == (void*)(a + k));
}

static void test_pool_entry() {
  using namespace bestep;
  constexpr int NO = 13 + 5, NBW = pool_body_words(13, 5);
  for (const uint32_t flags : {3u, 0u, 1u, 2u}) {
    uint32_t words[6 + NO], back[6 + NO];
    for (int k = 0; k < 6 + NO; ++k) words[k] = 0x01010101u * (uint32_t)(k + 1) + 0x00A00000u;   // all distinct
    words[3] = 0x3FFFFFFFu;                    // rows up to bit 29 ...
    words[3] = (words[3] & ~0x1000u) | (flags << 30);   // ... (one hole, so a stuck-at-1 shows) | flags
    const double f64[2] = {123.456, -7.25e9};
    double f64_back[2] = {0, 0};
    uint32_t tag[2] = {0xDEADBEEFu, 0xDEADBEEFu}, body[NBW];
    for (int k = 0; k < NBW; ++k) body[k] = 0xC0FFEE00u + (uint32_t)k;
    pool_entry_pack(words, f64, NO, tag, body);
    CHECK(tag[0] == words[0] && tag[1] == flags);
    CHECK(body[PB_ROWS] == (words[3] & 0x3FFFFFFFu));   // the flags are nowhere in the body
    CHECK(body[PB_ROWS + 1] == words[4] && body[PB_ROWS + 2] == words[5]);
    CHECK(body[PB_AGENT] == words[1] && body[PB_GOAL] == words[2]);
    CHECK(body[5] == 0xC0FFEE05u);             // the unused word and the padding keep what they held
    for (int k = PB_OBS + NO; k < NBW; ++k) CHECK(body[k] == 0xC0FFEE00u + (uint32_t)k);
    for (int k = 0; k < NO; ++k) CHECK(body[PB_OBS + k] == words[6 + k]);
    CHECK(memcmp(&body[PB_PREV], &f64[0], 8) == 0 && memcmp(&body[PB_TOTAL], &f64[1], 8) == 0);
    pool_entry_unpack(tag, body, NO, back, f64_back);
    CHECK(memcmp(back, words, sizeof words) == 0);
    CHECK(memcmp(f64_back, f64, sizeof f64) == 0);
    for (int k = 0; k < 6 + NO; ++k)           // the flags land in bits 30..31 of word 3 and nowhere else
      if (k != 3) CHECK(back[k] == words[k]);
    CHECK((back[3] >> 30) == flags && (back[3] & 0x3FFFFFFFu) == (0x3FFFFFFFu & ~0x1000u));
    tag[1] = flags | 0xFFFFFFFCu;              // only the tag's two flag bits reach the words
    pool_entry_unpack(tag, body, NO, back, f64_back);
    CHECK(memcmp(back, words, sizeof words) == 0);
  }
}

static void test_out_at() {
  constexpr int64_t S = 6, N = 7, F = 29;
  static uint8_t obs[S * N * F], done[S * N], trunc[S * N], term[S * N * F];
  static float obs_f32[S * N * F];
  static double reward[S * N], final_return[S * N], stats[8];
  static int32_t final_len[S * N];
  const be_out full{obs, obs_f32, reward, done, trunc, term, final_return, final_len, stats};
  const be_out s0 = be_out_at(full, 0, N, F);
  CHECK(memcmp(&s0, &full, sizeof full) == 0);   // step 0: the identity
  for (const int64_t s : {1, 5}) {
    const be_out o = be_out_at(full, s, N, F);   // each array by its own element size
    CHECK(o.obs == obs + s * N * F && o.obs_f32 == obs_f32 + s * N * F && o.terminal_obs == term + s * N * F);
    CHECK(o.reward == reward + s * N && o.done == done + s * N && o.truncated == trunc + s * N);
    CHECK(o.final_return == final_return + s * N && o.final_len == final_len + s * N);
    CHECK((char*)o.obs_f32 - (char*)obs_f32 == 4 * s * N * F && (char*)o.reward - (char*)reward == 8 * s * N);
    CHECK(o.stats == stats);                     // accumulates over the steps: never sliced
    be_out none;
    memset(&none, 0, sizeof none);
    none.reward = reward;
    const be_out n = be_out_at(none, s, N, F);   // NULL members stay NULL
    CHECK(!n.obs && !n.obs_f32 && !n.done && !n.truncated && !n.terminal_obs && !n.final_return && !n.final_len && !n.stats);
    CHECK(n.reward == reward + s * N);
  }
}

// be_a2c_adam's and be_mlp_opt's shared argument check: each rejection, in the order of the checks
// (every case is valid up to the argument it names, so the message shows which check fired).
static void test_optim_args() {
  alignas(8) static double buf[8];             // only addresses: nothing is read through them
  const double* state = buf;
  const double* losses = buf + 4;
  const double* log = buf + 6;
  const double* const off4[3] = {(const double*)((const char*)state + 4), (const double*)((const char*)losses + 4),
                                 (const double*)((const char*)log + 4)};
  const double nan = strtod("nan", nullptr);
  const auto has = [](const char* msg, const char* part) { return msg && strstr(msg, part); };
  // a fully valid call, with and without a log (log_rows is not looked at without one)
  CHECK(optim_args_error(state, true, 0.9, 0.999, 1e-8, losses, log, 2) == nullptr);
  CHECK(optim_args_error(state, true, 0.0, 0.0, 0.0, nullptr, nullptr, 0) == nullptr);
  CHECK(optim_args_error(state, true, 0.9, 0.999, 1e-8, nullptr, nullptr, -3) == nullptr);
  // the state: NULL, and 4 bytes past an 8-byte boundary (ahead of every other complaint)
  CHECK(has(optim_args_error(nullptr, true, 0.9, 0.999, 1e-8, losses, log, 2), "state"));
  CHECK(has(optim_args_error(off4[0], true, 0.9, 0.999, 1e-8, losses, log, 2), "state"));
  CHECK(has(optim_args_error(nullptr, true, 1.0, -0.1, -1.0, losses, nullptr, 0), "state"));
  // the Adam constants, beta1 before beta2 before eps; a NaN is out of every range
  CHECK(has(optim_args_error(state, true, 1.0, 0.999, 1e-8, losses, log, 2), "beta1"));
  CHECK(has(optim_args_error(state, true, 1.0, -0.1, -1.0, losses, log, 2), "beta1"));
  CHECK(has(optim_args_error(state, true, 0.9, -0.1, 1e-8, losses, log, 2), "beta2"));
  CHECK(has(optim_args_error(state, true, 0.9, -0.1, -1.0, losses, log, 2), "beta2"));
  CHECK(has(optim_args_error(state, true, nan, 0.999, 1e-8, losses, log, 2), "beta1"));
  CHECK(has(optim_args_error(state, true, 0.9, nan, 1e-8, losses, log, 2), "beta2"));
  CHECK(has(optim_args_error(state, true, 0.9, 0.999, -1.0, losses, log, 2), "eps"));
  CHECK(has(optim_args_error(state, true, 0.9, 0.999, nan, losses, log, 2), "eps"));
  CHECK(has(optim_args_error(state, true, 0.9, 0.999, -1.0, losses, nullptr, 0), "eps"));   // ahead of the log's checks
  // the loss log: losses without a log and the reverse, each of the two misaligned by 4, no rows
  CHECK(has(optim_args_error(state, true, 0.9, 0.999, 1e-8, losses, nullptr, 0), "losses and loss_log"));
  CHECK(has(optim_args_error(state, true, 0.9, 0.999, 1e-8, nullptr, log, 2), "losses and loss_log"));
  CHECK(has(optim_args_error(state, true, 0.9, 0.999, 1e-8, off4[1], log, 2), "not 8-byte aligned"));
  CHECK(has(optim_args_error(state, true, 0.9, 0.999, 1e-8, losses, off4[2], 2), "not 8-byte aligned"));
  CHECK(has(optim_args_error(state, true, 0.9, 0.999, 1e-8, off4[1], off4[2], 0), "not 8-byte aligned"));   // ahead of log_rows
  CHECK(has(optim_args_error(state, true, 0.9, 0.999, 1e-8, losses, log, 0), "log_rows"));
  CHECK(has(optim_args_error(state, true, 0.9, 0.999, 1e-8, losses, log, -1), "log_rows"));
  // plain SGD: the betas and eps are not looked at, the state and the log are
  CHECK(optim_args_error(state, false, 1.0, -0.1, -1.0, losses, log, 2) == nullptr);
  CHECK(optim_args_error(state, false, nan, nan, nan, nullptr, nullptr, 0) == nullptr);
  CHECK(has(optim_args_error(off4[0], false, 0.9, 0.999, 1e-8, losses, log, 2), "state"));
  CHECK(has(optim_args_error(state, false, 1.0, -0.1, -1.0, losses, nullptr, 0), "losses and loss_log"));
  CHECK(has(optim_args_error(state, false, 1.0, -0.1, -1.0, losses, off4[2], 2), "not 8-byte aligned"));
  CHECK(has(optim_args_error(state, false, 1.0, -0.1, -1.0, losses, log, 0), "log_rows"));
}

int main() {
  test_optim_args();
  test_pool_book();
  test_blob();
  test_pool_entry();
  test_out_at();
  printf("host_logic: OK\n");
  return 0;
}
