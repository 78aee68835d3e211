"""step2_kernel's wide-row-load instance: a wave's obstacle rows arrive 16 bytes per
lane and reach the pairs through LDS.  It has to be the plain instance bit for bit, against the
oracle too, put every (row, env) into the right lane's slot, and be taken only for whole waves
(num_envs a multiple of 32) and 16-byte aligned obstacle arrays -- anything else runs the plain
instance.  Default config (13 + 5 obstacles, W = 10), Philox mode, autoreset on.

BALLENV_STEP2_WIDE is read at be_create: the bit-identity runs are two fresh child processes (one
per value, each running every case, tests/step2_wide_worker.py); the other tests set it in this
process ahead of the context they create."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle
from step2_wide_worker import CASES, OUTPUTS
from test_gpu_episode import _check_state, _check_step, _setup
from test_gpu_parity import KEYS, load_np_state, make_env, np_state

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POOL, NOPOOL = "step2_kernel<10, 13, 5, true>", "step2_kernel<10, 13, 5, false>"


@pytest.fixture(scope="module")
def both_sides(gpu, tmp_path_factory):
    """The worker's record with BALLENV_STEP2_WIDE=1 and =0: computed once, shared, left unchanged."""
    d = tmp_path_factory.mktemp("step2_wide")
    res = {}
    for v in ("1", "0"):
        out = str(d / f"wide{v}.npz")
        env_vars = dict(os.environ, BALLENV_STEP2_WIDE=v, PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, os.path.join(HERE, "step2_wide_worker.py"), out], cwd=ROOT, env=env_vars,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        res[v] = dict(np.load(out))
    return res


@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("N,steps,offset", CASES)
def test_wide_equals_plain_instance(both_sides, N, steps, offset, pool):
    """Every per-step output, the save_state() blob and the stats slots of the two instances, from
    one seed: equal with ==.  N = 32 is one wave, 288 nine (the last block partial in waves), 96 at
    env_offset 12345; the 1 100 steps at N = 64 cross the TimeLimit and the pool's refills."""
    a, b = both_sides["1"], both_sides["0"]
    p = f"{N}_{int(pool)}_"
    assert str(a[p + "instance"]) == "wide" and str(b[p + "instance"]) == "plain"
    assert a[p + "reward"].shape == (steps, N)
    for k in OUTPUTS + ("state", "stats"):
        np.testing.assert_array_equal(a[p + k], b[p + k], err_msg=f"N={N} pool={pool}: {k}")
    done, trunc = a[p + "done"], a[p + "truncated"]
    print(f"N={N} pool={pool}: {int(done.sum())} episodes ended, {int(trunc.sum())} by the TimeLimit")
    assert done.sum() > 0
    if steps > 1000:
        assert trunc.sum() > 0, "no env reached the TimeLimit"


def test_wide_against_oracle(gpu, monkeypatch):
    """The wide instance forced, N = 64, 120 default-config steps from random episode phases
    (goal changes, TimeLimit truncations, resets): bit-exact against the oracle."""
    from gym_ballenv_amd.config import EnvConfig
    monkeypatch.setenv("BALLENV_STEP2_WIDE", "1")
    N, W = 64, 10
    env, cfg, st, out = _setup(EnvConfig(), N, W, gpu, 0, N, seed=0xBA11, rng=np.random.default_rng(64))
    assert env.kernel_name("step") == POOL
    acts = env.sample_actions(120, seed=0xBA11)
    n_trunc = 0
    for t in range(120):
        out["terminal_obs"][:] = 0
        env.terminal_obs.zero_()
        oracle.step(cfg, st, out, actions=acts[t].cpu().numpy())
        obs, reward, done, info = env.step(acts[t])
        assert env.step_instance() == "wide"
        n_trunc += _check_step(t, 0, N, out, obs, reward, done, info["truncated"], info["final_return"],
                               info["final_len"], info["terminal_obs"])
        _check_state(env, st, 0, N, f"t={t}")
    assert n_trunc > 0
    env.status()
    env.close()


AGENT, GOAL = (250, 450), (250, 50)


def _crafted_state(N):
    """Every static and dynamic obstacle of every env at a place of its own that names (row, env),
    all far from the agent (R = 25), which stands still under action 5."""
    e = np.arange(N)
    st = dict(agent=np.tile(np.int16(AGENT), (N, 1)), goal=np.tile(np.int16(GOAL), (N, 1)),
              prev_dist=np.full(N, 400.0), total_dist=np.full(N, 400.0), ep_return=np.zeros(N),
              ep_len=np.zeros(N, np.int32), episode=np.ones(N, np.uint32),
              static_obs=np.zeros((13, N, 2), np.int16), dyn_obs=np.zeros((5, N, 2), np.int16),
              dyn_goal=np.zeros((5, N), np.uint8))
    for k in range(13):
        st["static_obs"][k, :, 0] = 20 + 36 * k
        st["static_obs"][k, :, 1] = 20 + 8 * e
    for k in range(5):
        st["dyn_obs"][k, :, 0] = 30 + 90 * k
        st["dyn_obs"][k, :, 1] = 300 + 3 * e
        st["dyn_goal"][k] = k
    return st


@pytest.mark.parametrize("kind,row", [("static", 0), ("static", 7), ("static", 8), ("static", 12), ("dynamic", 4)])
def test_rows_land_in_the_right_slots(gpu, monkeypatch, kind, row):
    """A hand-written state at N = 32 in which only obstacle (row, env) touches the agent, for the
    first and last row of each of the two static loads and the last dynamic row, in envs 0, 3, 4
    and 31 (the ends of a lane's four envs and of the wave): only that env reports done, with the
    static or the dynamic penalty, and the outputs and the state -- every row of dyn_obs among
    them -- are the oracle's.  A transposed or shifted exchange cannot pass this."""
    from gym_ballenv_amd.config import EnvConfig
    monkeypatch.setenv("BALLENV_STEP2_WIDE", "1")
    N, W = 32, 10
    cfg_py = EnvConfig()
    env = make_env(cfg_py, N, W, gpu, seed=3, terminal_obs=True)
    cfg = cfg_py.to_abi(N, W, seed=3)
    out = oracle.new_out(cfg, terminal=True)
    acts = torch.full((N,), 5, dtype=torch.uint8, device=gpu)
    assert cfg_py.actions[5] == (0, 0)
    for e in (0, 3, 4, 31):
        st = _crafted_state(N)
        st["static_obs" if kind == "static" else "dyn_obs"][row, e] = AGENT
        load_np_state(env, st)
        out["terminal_obs"][:] = 0
        env.terminal_obs.zero_()
        oracle.step(cfg, st, out, actions=acts.cpu().numpy())
        obs, reward, done, info = env.step(acts)
        assert env.step_instance() == "wide"
        want = np.zeros(N, bool)
        want[e] = True
        np.testing.assert_array_equal(done.cpu().numpy(), want, err_msg=f"{kind} row {row} env {e}")
        r = reward.cpu().numpy()
        assert r[e] == -(cfg_py.static_penalty if kind == "static" else cfg_py.dynamic_penalty)
        assert (np.delete(r, e) == 0.0).all()
        _check_step(0, 0, N, out, obs, reward, done, info["truncated"], info["final_return"], info["final_len"],
                    info["terminal_obs"])
        got = np_state(env)
        np.testing.assert_array_equal(got["dyn_obs"], st["dyn_obs"], err_msg=f"{kind} row {row} env {e}: dyn_obs")
        for k in KEYS:
            np.testing.assert_array_equal(got[k], st[k], err_msg=f"{kind} row {row} env {e}: state[{k}]")
    env.status()
    env.close()


def _misalign_static(env):
    """static_obs as a view that starts 4 bytes into a larger buffer, and the be_state rebuilt on it."""
    from gym_ballenv_amd import _abi
    buf = torch.zeros(env.static_obs.numel() + 8, dtype=torch.int16, device=env.device)
    view = buf[2:2 + env.static_obs.numel()].view(env.static_obs.shape)
    view.copy_(env.static_obs)
    env.static_obs = view
    assert view.data_ptr() % 16 == 4
    env._st = _abi.BeState(*[getattr(env, k).data_ptr() for k in env.STATE_KEYS])
    env._st_ref = C.byref(env._st)


@pytest.mark.parametrize("N,misalign", [(33, False), (48, False), (64, True)])
def test_fallback_runs_the_plain_instance(gpu, monkeypatch, N, misalign):
    """With the variable unset, a batch that is no multiple of 32 (33, 48) and a state whose
    static_obs is not 16-byte aligned (N = 64) take the plain instance -- be_step_instance says so --
    and equal the one-lane kernel bit for bit (test_step2_equals_one_lane_kernel's method)."""
    from gym_ballenv_amd.config import EnvConfig
    monkeypatch.delenv("BALLENV_STEP2_WIDE", raising=False)
    cfg_py = EnvConfig(time_limit=20)
    envs = []
    for lpe in ("2", "1"):
        monkeypatch.setenv("BALLENV_STEP_LPE", lpe)
        envs.append(make_env(cfg_py, N, 10, gpu, seed=31, terminal_obs=True))
    monkeypatch.delenv("BALLENV_STEP_LPE")
    assert envs[0].kernel_name("step") == POOL and envs[1].kernel_name("step") == "be_kernel<10, 0, 13, 5, true>"
    for e in envs:
        e.reset()
    if misalign:
        _misalign_static(envs[0])
    assert envs[0].step_instance() == "none"
    acts = envs[0].sample_actions(45, seed=9)
    n_done = 0
    for t in range(45):
        for e in envs:
            e.terminal_obs.zero_()
        res = [e.step(acts[t]) for e in envs]
        assert envs[0].step_instance() == "plain" and envs[1].step_instance() == "plain"
        d = res[0][2].cpu().numpy()
        n_done += int(d.sum())
        for a, b in zip(res[0][:3], res[1][:3]):
            np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy(), err_msg=f"t={t}")
        for key in ("truncated", "terminal_obs"):
            np.testing.assert_array_equal(res[0][3][key].cpu().numpy(), res[1][3][key].cpu().numpy(), err_msg=key)
        for key in ("final_return", "final_len"):
            np.testing.assert_array_equal(res[0][3][key].cpu().numpy()[d], res[1][3][key].cpu().numpy()[d])
        s0, s1 = np_state(envs[0]), np_state(envs[1])
        for k in KEYS:
            np.testing.assert_array_equal(s0[k], s1[k], err_msg=f"t={t} {k}")
    np.testing.assert_array_equal(envs[0].stats_buf.cpu().numpy(), envs[1].stats_buf.cpu().numpy())
    assert n_done > 0
    for e in envs:
        e.status()
        e.close()


def test_forced_wide_still_falls_back(gpu, monkeypatch):
    """BALLENV_STEP2_WIDE=1 lifts no precondition: N = 33 runs the plain instance; =0 keeps an
    aligned N = 64 off the wide one."""
    from gym_ballenv_amd.config import EnvConfig
    for v, N in (("1", 33), ("0", 64)):
        monkeypatch.setenv("BALLENV_STEP2_WIDE", v)
        env = make_env(EnvConfig(), N, 10, gpu, seed=1)
        env.reset()
        env.step(env.sample_actions(1, seed=1)[0])
        assert env.step_instance() == "plain", (v, N)
        env.status()
        env.close()
