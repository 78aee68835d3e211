"""GPU: the step kernels' argument passing ("the prologue's kernel arguments").

step2_kernel takes the arguments its first loads go through (tables, episode, ep_len, the obstacle
arrays, n, gid0) as leading scalar kernel arguments, preloaded into SGPRs, then KHot (the pointers of
its other prologue loads, the stats slots, prev_read, goal_change) in front of the KParams block;
launch() fills all three from one KParams.  A leading argument
in the wrong position, or one kept from an earlier launch (another context, another buffer, a
captured graph), sends a load or a store through the wrong pointer.  Every case here runs 40 steps
with autoreset on (TimeLimit 20 from random ep_len phases, so every env finishes about twice and
both of step2_kernel's paths run) at N = 1, 33, 127, 129, 257 -- one lane pair, a partial wave, one
env short of a block, one env past it, two blocks and one env -- asserts the kernel it expects, and
compares outputs, state and status bit for bit with the C oracle.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from test_gpu_finish_path import _check_outputs
from test_gpu_parity import KEYS, assert_state_equal, make_env

pytestmark = pytest.mark.gpu

T, LIMIT = 40, 20
SIZES = (1, 33, 127, 129, 257)
STEP2, STEP2_NOPOOL = "step2_kernel<10, 13, 5, true>", "step2_kernel<10, 13, 5, false>"
STEPW, ONE_LANE = "stepw_kernel<5, 13, 5, 8, true>", "be_kernel<10, 0, 13, 5, true>"
OUT_KEYS = ("obs", "reward", "done", "truncated", "final_return", "final_len", "terminal_obs")


def _cfg():
    from gym_ballenv_amd.config import EnvConfig
    return EnvConfig(time_limit=LIMIT)


def _lens(N, seed):
    return np.random.default_rng(seed).integers(0, LIMIT, N).astype(np.int32)


def _seed(W, N):
    return 1000 * W + N


@functools.lru_cache(maxsize=None)
def _reference(W, N, seed):
    """The oracle's trajectory, computed once per (W, N, seed) and read-only afterwards: the actions,
    and per step the outputs, the state after the step and the status."""
    cfg = _cfg().to_abi(N, W, seed=seed)
    st, out = oracle.new_state(cfg), oracle.new_out(cfg, terminal=True)
    oracle.reset(cfg, st, out)
    st["ep_len"][:] = _lens(N, seed)
    acts = oracle.sample_actions(cfg, T, seed + 1)
    steps = []
    for t in range(T):
        out["terminal_obs"][:] = 0
        status = oracle.step(cfg, st, out, actions=acts[t])
        rec = ({k: out[k].copy() for k in OUT_KEYS}, {k: st[k].copy() for k in KEYS}, status)
        for d in rec[:2]:
            for v in d.values():
                v.flags.writeable = False
        steps.append(rec)
    assert sum(int(o["done"].sum()) for o, _, _ in steps) >= N, "every env finishes inside the run"
    acts.flags.writeable = False
    return acts, steps


def _acts(acts_np, dev):
    return torch.from_numpy(acts_np.copy()).to(dev)


def _env(W, N, dev, seed, pool=True):
    old = os.environ.get("BALLENV_POOL")
    if not pool:
        os.environ["BALLENV_POOL"] = "0"
    try:
        env = make_env(_cfg(), N, W, dev, seed=seed, terminal_obs=True)
    finally:
        if not pool:
            if old is None:
                del os.environ["BALLENV_POOL"]
            else:
                os.environ["BALLENV_POOL"] = old
    env.reset()
    env.ep_len.copy_(torch.from_numpy(_lens(N, seed)).to(dev))
    if env.pool_bytes():
        env.pool_set_period(4)      # refills inside the run: pool hits and stale entries both happen
    return env


def _check_step(env, t, ref, res):
    out, st, status = ref
    _check_outputs(t, out, *res)
    assert_state_equal(env, st, f"t={t}")
    assert env.status() == status == 0, f"t={t} status"


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kernel", ["step2_pool", "step2_nopool", "stepw", "one_lane"])
def test_fixed_shape_kernels_equal_the_oracle(gpu, monkeypatch, kernel, N):
    """Each fixed-shape step kernel: step2_kernel with the pool and with BALLENV_POOL=0, stepw_kernel
    at W = 5, and the one-lane kernel (BALLENV_STEP_LPE=1)."""
    W = 5 if kernel == "stepw" else 10
    if kernel == "one_lane":
        monkeypatch.setenv("BALLENV_STEP_LPE", "1")
    seed = _seed(W, N)
    env = _env(W, N, gpu, seed, pool=kernel != "step2_nopool")
    assert env.kernel_name("step") == {"step2_pool": STEP2, "step2_nopool": STEP2_NOPOOL, "stepw": STEPW,
                                       "one_lane": ONE_LANE}[kernel]
    acts_np, steps = _reference(W, N, seed)
    acts = _acts(acts_np, gpu)
    for t in range(T):
        env.terminal_obs.zero_()
        _check_step(env, t, steps[t], env.step(acts[t]))
    env.close()


@pytest.mark.parametrize("N", SIZES)
def test_step_n_equals_steps(gpu, N):
    """be_step_n (the action pointer advances per launch inside one library call) leaves the state and
    the last step's outputs of the same count of be_step calls: the oracle's after step T."""
    W, seed = 10, _seed(10, N)
    env = _env(W, N, gpu, seed)
    assert env.kernel_name("step") == STEP2
    acts_np, steps = _reference(W, N, seed)
    acts, half = _acts(acts_np, gpu), T // 2
    _check_step(env, half - 1, steps[half - 1], env.step_n(acts[:half]))
    env.step_n(acts[half:T - 1])
    res = env.step_n(acts[T - 1:])
    _check_step(env, T - 1, steps[T - 1], res)
    env.close()


@pytest.mark.parametrize("N", SIZES)
def test_captured_graph_equals_the_oracle(gpu, N):
    """The T steps captured into one graph (as bench.py launches them) and replayed: the per-step
    outputs copied inside the graph and the final state equal the oracle's, i.e. the eager run's."""
    from gym_ballenv_amd import _abi
    W, seed = 10, _seed(10, N)
    env = _env(W, N, gpu, seed)
    assert env.kernel_name("step") == STEP2
    acts_np, steps = _reference(W, N, seed)
    acts = _acts(acts_np, gpu)
    names = ("obs", "reward", "done", "truncated", "final_return", "final_len")
    rec = {k: torch.empty((T,) + tuple(getattr(env, k).shape), dtype=getattr(env, k).dtype, device=gpu) for k in names}
    lib, ctx, st, out = env._lib, env._ctx, C.byref(env._st), C.byref(env._out)
    side = torch.cuda.Stream(gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        cs = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
        for t in range(T):
            rc = lib.be_step(ctx, st, C.c_void_p(acts[t].data_ptr()), None, None, out, cs)
            if rc:
                _abi.check(rc, ctx)
            for k, buf in rec.items():
                buf[t].copy_(getattr(env, k))
    g.replay()
    torch.cuda.synchronize(gpu)
    for t in range(T):
        o = steps[t][0]
        _check_outputs(t, o, rec["obs"][t], rec["reward"][t], rec["done"][t],
                       {k: rec[k][t] for k in ("truncated", "final_return", "final_len")})
    assert_state_equal(env, steps[T - 1][1], "after the replay")
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("N", SIZES)
def test_two_contexts_stepped_alternately(gpu, N):
    """Two contexts (two seeds, so two trajectories, each with its own state, output buffers, tables
    and pool) stepped in turn: each equals its own oracle run after every step."""
    W = 10
    seeds = (_seed(W, N), _seed(W, N) + 7)
    envs = [_env(W, N, gpu, s) for s in seeds]
    refs = [_reference(W, N, s) for s in seeds]
    acts = [_acts(r[0], gpu) for r in refs]
    for t in range(T):
        for e, r, a in zip(envs, refs, acts):
            assert e.kernel_name("step") == STEP2
            e.terminal_obs.zero_()
            res = e.step(a[t])
            _check_step(e, t, r[1][t], res)
    for e in envs:
        e.close()


@pytest.mark.parametrize("N", SIZES)
def test_second_set_of_output_buffers(gpu, N):
    """One env, one state: the first half of the run into the env's own output buffers, the second half
    into a second set.  The second set receives the results (the oracle's, every step) and the first
    set stays exactly as the last step that wrote it left it."""
    from gym_ballenv_amd import _abi
    W, seed = 10, _seed(10, N)
    env = _env(W, N, gpu, seed)
    assert env.kernel_name("step") == STEP2
    acts_np, steps = _reference(W, N, seed)
    acts = _acts(acts_np, gpu)
    half = T // 2
    for t in range(half):
        env.terminal_obs.zero_()
        _check_step(env, t, steps[t], env.step(acts[t]))
    names = ("obs", "reward", "done", "truncated", "terminal_obs", "final_return", "final_len")
    first = {k: getattr(env, k).clone() for k in names}
    second = {k: torch.zeros_like(getattr(env, k)) for k in names}
    stats2 = torch.zeros_like(env.stats_buf)
    out2 = _abi.BeOut(second["obs"].data_ptr(), None, second["reward"].data_ptr(), second["done"].data_ptr(),
                      second["truncated"].data_ptr(), second["terminal_obs"].data_ptr(),
                      second["final_return"].data_ptr(), second["final_len"].data_ptr(), stats2.data_ptr())
    for t in range(half, T):
        second["terminal_obs"].zero_()
        _abi.check(env._lib.be_step(env._ctx, C.byref(env._st), C.c_void_p(acts[t].data_ptr()), None, None,
                                    C.byref(out2), env._stream()), env._ctx)
        info = {k: second[k] for k in ("truncated", "final_return", "final_len", "terminal_obs")}
        _check_step(env, t, steps[t], (second["obs"], second["reward"], second["done"], info))
    for k in names:
        assert torch.equal(getattr(env, k), first[k]), f"the first set's {k} changed"
    assert stats2[:, 0].sum().item() == sum(int(steps[t][0]["done"].sum()) for t in range(half, T))
    env.close()
