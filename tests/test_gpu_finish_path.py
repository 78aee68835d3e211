"""GPU: step2_kernel's two paths ("the wave-uniform split").

After `done` is known a wave of step2_kernel takes one of two instruction streams: the lean path
when none of its 32 envs finished, the finishing path (pool entry loads issued ahead of the stores,
the statistics fold, ONE raster shared by the obs and the terminal obs, then the resets) when one
did.  Each test here aims at one way that split can go wrong: a wave on the wrong path, a lane of a
finishing wave that does not itself finish, hit / stale / unwritten entries side by side, the
terminal obs taken from the shared raster, the moved statistics fold, finishing without a reset,
and the pool's rejection flag.  W = 10 and the default obstacle counts throughout (the two-lane
kernel), against the C oracle and against the env without a pool.
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from test_gpu_parity import KEYS, assert_state_equal, make_env
from test_gpu_pool import _no_pool_env

pytestmark = pytest.mark.gpu

W = 10
POOL, NOPOOL = "step2_kernel<10, 13, 5, true>", "step2_kernel<10, 13, 5, false>"


def _oracle(cfg_py, N, seed, terminal=True):
    cfg = cfg_py.to_abi(N, W, seed=seed)
    st, out = oracle.new_state(cfg), oracle.new_out(cfg, terminal=terminal)
    oracle.reset(cfg, st, out)
    return cfg, st, out


def _check_outputs(t, out, obs, reward, done, info):
    d = out["done"].astype(bool)
    np.testing.assert_array_equal(done.cpu().numpy(), d, err_msg=f"t={t} done")
    np.testing.assert_array_equal(reward.cpu().numpy(), out["reward"], err_msg=f"t={t} reward")
    np.testing.assert_array_equal(obs.cpu().numpy(), out["obs"], err_msg=f"t={t} obs")
    np.testing.assert_array_equal(info["truncated"].cpu().numpy(), out["truncated"].astype(bool), err_msg=f"t={t} truncated")
    np.testing.assert_array_equal(info["final_return"].cpu().numpy()[d], out["final_return"][d], err_msg=f"t={t} final_return")
    np.testing.assert_array_equal(info["final_len"].cpu().numpy()[d], out["final_len"][d], err_msg=f"t={t} final_len")
    if "terminal_obs" in info:
        np.testing.assert_array_equal(info["terminal_obs"].cpu().numpy()[d], out["terminal_obs"][d],
                                      err_msg=f"t={t} terminal_obs")
    return d


def _check_stats(env, out, abs_returns):
    """count, sum of lengths, min and max exactly; the two f64 sums to the reassociation bound: the
    env adds per 32-env slot and then over the slots, the oracle in env order, so each is within
    (n - 1) 2^-53 sum|x| of the exact sum and they differ by at most (n - 1) 2^-52 sum|x|.  (The
    two sums cannot be compared bit for bit: the summation orders differ by design.  The bound is
    tighter than the rtol = 1e-12 of the existing oracle comparisons.  episode_stats()'s sum is the
    record's, so it is held to the oracle's through the same bound.)"""
    s_gpu, s_orc = env.stats_record().cpu().numpy(), out["stats"]
    n = int(s_orc[0])
    assert n > 0
    assert s_gpu[0] == s_orc[0] and s_gpu[3] == s_orc[3] and s_gpu[4] == s_orc[4] and s_gpu[5] == s_orc[5]
    r = np.abs(np.asarray(abs_returns, np.float64))
    assert abs(s_gpu[1] - s_orc[1]) <= n * 2.0 ** -52 * r.sum()
    # (the squares: the same bound, plus one rounding of each square should a compiler contract r * r + s)
    assert abs(s_gpu[2] - s_orc[2]) <= (n + 1) * 2.0 ** -52 * (r * r).sum()
    es = env.episode_stats()
    assert es["episodes"] == n and es["min_return"] == s_orc[4] and es["max_return"] == s_orc[5]
    assert es["sum_return"] == s_gpu[1]


@pytest.mark.parametrize("pool", [True, False])
def test_mixed_waves(gpu, pool):
    """N = 100: three full waves, a four-env partial wave, a partial block.  Env 5 finishes alone in
    wave 0, no env of wave 1 does (the lean path), the neighbouring pairs 70 and 71 in wave 2, and
    the last env, 99, in the partial wave.  One step, with the pool and without: every output, the
    terminal obs and the whole state equal the oracle."""
    from gym_ballenv_amd.config import EnvConfig
    N, seed = 100, 22   # (at this seed no other env finishes on the first step: the oracle's done below)
    cfg_py = EnvConfig(time_limit=1000)
    env = (make_env if pool else _no_pool_env)(cfg_py, N, W, gpu, seed=seed, terminal_obs=True)
    assert env.kernel_name("step") == (POOL if pool else NOPOOL) and (env.pool_bytes() > 0) == pool
    cfg, st, out = _oracle(cfg_py, N, seed)
    env.reset()
    for j in (5, 70, 71, 99):
        env.ep_len[j] = 999
        st["ep_len"][j] = 999
    acts = env.sample_actions(1, seed=seed)
    obs, reward, done, info = env.step(acts[0])
    oracle.step(cfg, st, out, actions=acts[0].cpu().numpy())
    d = _check_outputs(0, out, obs, reward, done, info)
    assert np.nonzero(d)[0].tolist() == [5, 70, 71, 99], "env 5 alone in wave 0, wave 1 on the lean path"
    assert_state_equal(env, st, "mixed waves")
    env.status()
    env.close()


def test_hit_stale_unwritten_in_one_wave(gpu):
    """Three finishing envs of one wave (N = 64): env 3's entry is current (a hit), env 10's is
    re-tagged to another episode (stale), env 21's has its written flag cleared.  All three reset to
    the oracle's state and obs.  Then env 3's next entry is poisoned (a moved agent) and shows up
    in the state: the hit is still a copy."""
    from gym_ballenv_amd.config import EnvConfig
    N, seed = 64, 23
    cfg_py = EnvConfig(time_limit=1000)
    env = make_env(cfg_py, N, W, gpu, seed=seed, terminal_obs=True)
    assert env.kernel_name("step") == POOL
    env.pool_set_period(0)
    cfg, st, out = _oracle(cfg_py, N, seed)
    env.reset()
    ep = env.episode.cpu().numpy().view(np.uint32)
    e10, e21 = int(ep[10]), int(ep[21])
    words, f64 = env.pool_entry(10, (e10 + 1) & 1)
    assert words[0] == e10 + 1
    words[0] = e10 + 5
    env.pool_entry(10, (e10 + 1) & 1, write=(words, f64))
    words, f64 = env.pool_entry(21, (e21 + 1) & 1)
    assert words[3] & (1 << 30)
    words[3] &= ~(1 << 30)
    env.pool_entry(21, (e21 + 1) & 1, write=(words, f64))
    for j in (3, 10, 21):
        env.ep_len[j] = 999
        st["ep_len"][j] = 999
    acts = env.sample_actions(2, seed=seed)
    obs, reward, done, info = env.step(acts[0])
    oracle.step(cfg, st, out, actions=acts[0].cpu().numpy())
    d = _check_outputs(0, out, obs, reward, done, info)
    assert d[[3, 10, 21]].all()
    assert_state_equal(env, st, "hit / stale / unwritten")
    e3 = int(env.episode[3].item())
    words, f64 = env.pool_entry(3, (e3 + 1) & 1)
    assert words[0] == e3 + 1 and words[3] & (1 << 30)
    words[1] = (7 & 0xFFFF) | (3 << 16)                      # agent (7, 3)
    env.pool_entry(3, (e3 + 1) & 1, write=(words, f64))
    env.ep_len[3] = 999
    env.step(acts[1])
    assert env.episode[3].item() == e3 + 1 and env.ep_len[3].item() == 0
    assert env.agent[3].tolist() == [7, 3], "the finishing path did not copy the pool entry"
    env.status()
    env.close()


def _run(envs, cfg_py, N, seed, steps, limit, gpu, check=True, terminal=True):
    """`steps` steps of `envs` (the same ids and seed) and the oracle from random ep_len phases; with
    check, every output and the state of envs[0] against the oracle after every step.  Returns the
    oracle's out and the finished episodes' returns."""
    cfg, st, out = _oracle(cfg_py, N, seed, terminal=terminal)
    lens = np.random.default_rng(seed).integers(0, limit, N).astype(np.int32)
    for e in envs:
        e.reset()
        e.ep_len.copy_(torch.from_numpy(lens).to(gpu))
    st["ep_len"][:] = lens
    acts = envs[0].sample_actions(steps, seed=seed + 1)
    acts_np = acts.cpu().numpy()
    rets = []
    for t in range(steps):
        res = [e.step(acts[t]) for e in envs]
        oracle.step(cfg, st, out, actions=acts_np[t])
        rets.append(out["final_return"][out["done"].astype(bool)].copy())
        if check:
            _check_outputs(t, out, *res[0])
            assert_state_equal(envs[0], st, f"t={t}")
    return out, np.concatenate(rets)


def test_terminal_obs_from_the_shared_raster(gpu):
    """terminal_obs=True, N = 256, TimeLimit 20, 60 steps from random phases with a refill every 4
    steps, so hits and stale entries mix: the terminal obs on done rows, obs, reward, done,
    truncated, final_* and the state equal the oracle after every step."""
    from gym_ballenv_amd.config import EnvConfig
    cfg_py = EnvConfig(time_limit=20)
    env = make_env(cfg_py, 256, W, gpu, seed=41, terminal_obs=True)
    assert env.kernel_name("step") == POOL
    env.pool_set_period(4)
    out, rets = _run([env], cfg_py, 256, 41, 60, 20, gpu)
    assert len(rets) >= 3 * 256
    env.status()
    env.close()


@pytest.mark.parametrize("limit,steps", [(20, 60), (1, 3)])
def test_statistics_fold(gpu, limit, steps):
    """The fold now runs ahead of the resets, only in finishing waves.  N = 1 000, the run of the
    terminal-obs test (and TimeLimit 1 for three steps: every lane of every wave folds): the stats
    slots equal the no-pool env's bit for bit, and episode_stats() the oracle's count, sums, min
    and max."""
    from gym_ballenv_amd.config import EnvConfig
    N, seed = 1000, 43
    cfg_py = EnvConfig(time_limit=limit)
    a = make_env(cfg_py, N, W, gpu, seed=seed, terminal_obs=True)
    b = _no_pool_env(cfg_py, N, W, gpu, seed=seed, terminal_obs=True)
    assert a.kernel_name("step") == POOL and b.kernel_name("step") == NOPOOL
    a.pool_set_period(4)
    out, rets = _run([a, b], cfg_py, N, seed, steps, limit, gpu, check=False)
    assert torch.equal(a.stats_buf, b.stats_buf)
    for k in KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert len(rets) == steps * N if limit == 1 else len(rets) >= 2 * N
    _check_stats(a, out, rets)
    a.status()
    b.status()
    a.close()
    b.close()


def test_autoreset_off(gpu):
    """autoreset off: a done env takes the finishing path and is not reset.  N = 100 (a partial
    wave), TimeLimit 20 from random phases, 25 steps (by then every env is past the limit and done
    on every step): final_return / final_len, the statistics and the un-reset state equal the
    oracle."""
    from gym_ballenv_amd.config import EnvConfig
    N, seed = 100, 47
    cfg_py = EnvConfig(time_limit=20, autoreset=False)
    env = make_env(cfg_py, N, W, gpu, seed=seed)
    assert env.kernel_name("step") == NOPOOL and env.pool_bytes() == 0
    out, rets = _run([env], cfg_py, N, seed, 25, 20, gpu, terminal=False)
    assert out["done"].all() and (env.ep_len.cpu().numpy() >= 25).all()
    _check_stats(env, out, rets)
    env.status()
    env.close()


def test_rejection_flag_through_the_pool(gpu):
    """An entry's rejection flag reaches the status word when, and only when, a step consumes the
    entry.  Env 12 shares wave 0 with env 9, which finishes: the wave runs the finishing path and
    loads env 12's flagged entry, but env 12 does not finish, so the status must stay clean.  Flagged
    on env 9 itself, which finishes again, status() reports the rejection limit."""
    from gym_ballenv_amd import _abi
    from gym_ballenv_amd.config import EnvConfig
    N, seed = 64, 53
    cfg_py = EnvConfig(time_limit=1000)
    env = make_env(cfg_py, N, W, gpu, seed=seed)
    assert env.kernel_name("step") == POOL
    env.pool_set_period(0)
    env.reset()

    def flag(j):
        e = int(env.episode[j].item())
        words, f64 = env.pool_entry(j, (e + 1) & 1)
        assert words[0] == e + 1 and words[3] & (1 << 30) and not words[3] & (1 << 31)
        words[3] |= 1 << 31
        env.pool_entry(j, (e + 1) & 1, write=(words, f64))

    acts = env.sample_actions(2, seed=seed)
    flag(12)                                                   # wave 0; does not finish
    env.ep_len[9] = 999                                        # env 9 of the same wave finishes, its entry unflagged
    _, _, done, _ = env.step(acts[0])
    assert done[9].item() and not done[12].item()
    assert env.status() == 0
    flag(9)
    env.ep_len[9] = 999
    _, _, done, _ = env.step(acts[1])
    assert done[9].item() and not done[12].item()
    with pytest.raises(_abi.BallEnvError, match="rejection"):
        env.status()
    env.close()
