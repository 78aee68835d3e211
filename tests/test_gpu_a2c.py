"""be_a2c_targets on the GPU: bit-equal to the scalar restatement (tests/a2c_ref.py) on random
and crafted episode structures, a drop-in for Rollout.discounted_returns, graph-capturable,
deterministic, and a2c_update(targets="hip") trains."""
import copy

import numpy as np
import pytest
import torch

from a2c_ref import EPS, a2c_targets_ref, make_case

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def _env(gpu, N, W=5, seed=3):
    import gym_ballenv_amd as gb
    return gb.BatchedBallEnv(N, W, gb.EnvConfig(), device=gpu, seed=seed)


def _crafted(T, N, seed):
    """Random inputs as in the CPU test (N(0, 0.7) rewards with 1 % of -8000; dones at 5 %, 1 % for
    the long horizon) with the first columns overwritten by the edge cases."""
    rng = np.random.default_rng(seed)
    rewards, dones = make_case(rng, T, N, 0.01 if T >= 1000 else 0.05, 0.7, True)
    values = rng.normal(0, 1, (T, N)).astype(np.float32)
    bootstrap = rng.normal(0, 5, N)
    dones[:, :8] = False
    dones[0, 0] = True                      # done at t = 0
    dones[T - 1, 1] = True                  # done at T-1
    if T >= 3:
        dones[T // 2 - 1:T // 2 + 1, 2] = True   # two consecutive dones: a one-step episode
    #  column 3: no done at all
    dones[:, 4] = True                      # every step done
    rewards[:, 5] = -1.25                   # constant rewards (std 0 at gamma = 0), one horizon-long episode
    if T > 20:
        dones[16, 6] = True                 # episodes of exactly 17 and 16 steps: either side of the
        dones[32, 6] = True                 # kernel's split between its short and long episode paths
        rewards[:, 7] = -1.25
        dones[T // 2, 7] = True             # constant rewards in two episodes
    return rewards, dones, values, bootstrap


def _run(env, gpu, rewards, dones, values, bootstrap, gamma, with_adv=True, with_returns=True, as_bool=True):
    from gym_ballenv_amd.rollout import A2CTargets, a2c_targets_into
    T, N = rewards.shape
    r = torch.from_numpy(rewards).to(gpu)
    d = torch.from_numpy(dones if as_bool else dones.astype(np.uint8)).to(gpu)
    v = torch.from_numpy(values).to(gpu) if with_adv else None
    b = torch.from_numpy(bootstrap).to(gpu) if bootstrap is not None else None
    out = A2CTargets(torch.full((T, N), SENTINEL, dtype=torch.float32, device=gpu),
                     torch.full((T, N), SENTINEL, dtype=torch.float32, device=gpu) if with_adv else None,
                     torch.full((T, N), 7, dtype=torch.uint8, device=gpu),
                     torch.full((T, N), SENTINEL, dtype=torch.float64, device=gpu) if with_returns else None)
    a2c_targets_into(env, r, d, v, gamma, EPS, b, out)
    torch.cuda.synchronize(gpu)
    return out


def _assert_equal(out, ref, tag):
    assert torch.equal(out.valid.cpu(), torch.from_numpy(ref["valid"])), f"{tag}: valid"
    for name in ("returns", "returns_norm", "advantage"):
        got = getattr(out, name)
        if got is None:
            continue
        got, want = got.cpu().numpy(), ref[name]
        assert not np.isnan(want).any() and not np.isnan(got).any(), f"{tag}: {name} has NaN"
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{tag}: {name} differs at {len(bad)} elements, first (t, n) = {bad[0]}: " \
                              f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("T,N", [(1, 323), (2, 64), (37, 323), (130, 323), (1000, 70)])
def test_targets_bit_equal_restatement(gpu, T, N):
    env = _env(gpu, N)
    rewards, dones, values, bootstrap = _crafted(T, N, seed=T)
    # gamma 0.99 with a bootstrap carried into the horizon-cut runs
    out = _run(env, gpu, rewards, dones, values, bootstrap, 0.99)
    ref = a2c_targets_ref(rewards, dones, values, bootstrap, 0.99, EPS)
    _assert_equal(out, ref, "gamma 0.99 + bootstrap")
    if T >= 3:
        assert ref["valid"][T // 2, 2] == 0 and out.returns_norm[T // 2, 2] == 0 and out.advantage[T // 2, 2] == 0
    assert (ref["valid"][:, 4] == 0).all()
    # gamma 0: R = r, so the constant-reward episodes have std 0 and normalise to exactly 0
    out0 = _run(env, gpu, rewards, dones, values, None, 0.0, as_bool=False)
    ref0 = a2c_targets_ref(rewards, dones, values, None, 0.0, EPS)
    _assert_equal(out0, ref0, "gamma 0")
    if T >= 2:
        assert (out0.valid[:, 5] == 1).all() and (out0.returns_norm[:, 5] == 0).all()
    # the optional outputs left out: the required ones do not change
    out1 = _run(env, gpu, rewards, dones, values, bootstrap, 0.99, with_adv=False, with_returns=False)
    assert torch.equal(out1.returns_norm, out.returns_norm) and torch.equal(out1.valid, out.valid)
    env.close()


def test_two_calls_are_bit_identical(gpu):
    T, N = 130, 323
    env = _env(gpu, N)
    rewards, dones, values, bootstrap = _crafted(T, N, seed=9)
    a = _run(env, gpu, rewards, dones, values, bootstrap, 0.99)
    b = _run(env, gpu, rewards, dones, values, bootstrap, 0.99)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    env.close()


def test_public_call_validates_and_allocates(gpu):
    import gym_ballenv_amd as gb
    T, N = 37, 323
    env = _env(gpu, N)
    rewards, dones, values, bootstrap = _crafted(T, N, seed=5)
    r, d, v = (torch.from_numpy(x).to(gpu) for x in (rewards, dones, values))
    tg = gb.a2c_targets(env, r, d, v, gamma=0.99, bootstrap=torch.from_numpy(bootstrap).to(gpu))
    torch.cuda.synchronize(gpu)
    _assert_equal(tg, a2c_targets_ref(rewards, dones, values, bootstrap, 0.99, EPS), "a2c_targets")
    assert gb.a2c_targets(env, r, d).advantage is None
    for bad in (dict(rewards=r.float()), dict(rewards=r[:, :-1]), dict(rewards=r.t().contiguous().t()),
                dict(rewards=r.cpu()), dict(dones=d.to(torch.int32)), dict(values=v.double()),
                dict(bootstrap=torch.zeros(N, device=gpu))):
        kw = dict(rewards=r, dones=d, values=v, bootstrap=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            gb.a2c_targets(env, kw["rewards"], kw["dones"], kw["values"], bootstrap=kw["bootstrap"])
    env.close()


@pytest.fixture(scope="module")
def rollout20(gpu):
    """A real 20-step, 512-env backend="hip" rollout, shared (and left unchanged) by the tests below."""
    from gym_ballenv_amd import Rollout
    from gym_ballenv_amd.policy import Policy
    env = _env(gpu, 512, W=10, seed=0x1234)
    env.reset()
    torch.manual_seed(0)
    ro = Rollout(env, Policy(10), horizon=20, backend="hip")
    ro.run_eager()
    torch.cuda.synchronize(gpu)
    yield ro
    ro.close()
    env.close()


def test_returns_equal_discounted_returns(gpu, rollout20):
    ro = rollout20
    tg = ro.targets(0.99)
    assert torch.equal(tg.returns, ro.discounted_returns(0.99))
    boot = torch.linspace(-3, 3, 512, dtype=torch.float64, device=gpu)
    assert torch.equal(ro.targets(0.9, bootstrap=boot).returns, ro.discounted_returns(0.9, bootstrap=boot))
    ref = a2c_targets_ref(ro.rewards.cpu().numpy(), ro.dones.cpu().numpy(), ro.values.cpu().numpy(), None, 0.99, EPS)
    _assert_equal(tg, ref, "rollout")


def test_graph_capture_matches_eager(gpu, rollout20):
    """Captured on one stream and replayed twice.  The capture stream is the test's own HIP stream,
    destroyed at the end: a stream taken from torch's pool keeps its hardware queue for the life of
    the process, and which queue the streams of later tests land on (tests/test_gpu_graph.py checks
    that a side stream and the default stream run side by side) would then depend on this test."""
    import ctypes
    from gym_ballenv_amd.rollout import A2CTargets, a2c_targets_into
    ro = rollout20
    eager = ro.targets(0.99)
    torch.cuda.synchronize(gpu)
    out = A2CTargets(*(torch.full_like(x, 3) for x in eager))
    hip = ctypes.CDLL("libamdhip64.so")
    handle = ctypes.c_void_p()
    with torch.cuda.device(gpu):
        assert hip.hipStreamCreate(ctypes.byref(handle)) == 0
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.ExternalStream(handle.value, device=gpu)):
            a2c_targets_into(ro.env, ro.rewards, ro.dones, ro.values, 0.99, EPS, None, out)
        for _ in range(2):
            for x in out:
                x.fill_(3)
            g.replay()
            torch.cuda.synchronize(gpu)
            for x, y in zip(out, eager):
                assert torch.equal(x, y)
        del g
    finally:
        torch.cuda.synchronize(gpu)
        assert hip.hipStreamDestroy(handle) == 0


def test_a2c_update_with_hip_targets(gpu):
    """Mirror of test_gpu_policy.py::test_a2c_update_on_gpu_rollout with targets="hip": the loss is
    finite, the weights move and the rollout's kernel is re-packed."""
    from gym_ballenv_amd import Rollout, a2c_update
    from gym_ballenv_amd.policy import Policy, reference_weights
    path = reference_weights(10)
    torch.manual_seed(0)
    pol = (Policy.from_npz(path, 10) if path else Policy(10)).to(gpu)
    w0 = copy.deepcopy(pol.state_dict())
    env = _env(gpu, 512, W=10, seed=3)
    env.reset()
    ro = Rollout(env, pol, horizon=32, backend="hip", record_obs=True, seed=2)
    ro.run_eager()
    a_old = ro.hp.act(seed=9)[1].clone()
    opt = torch.optim.Adam(pol.parameters(), lr=1e-2)
    loss = a2c_update(ro, opt, gamma=0.99, targets="hip")
    assert np.isfinite(loss)
    assert not torch.equal(w0["fc1.weight"], pol.fc1.weight.detach())
    assert not torch.equal(ro.hp.act(seed=9)[1], a_old)        # re-packed: the log-probs moved
    with pytest.raises(ValueError):
        a2c_update(ro, opt, 0.99, targets="cuda")
    ro.close()
    env.close()
