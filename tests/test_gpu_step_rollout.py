"""GPU: the one T-step loop (rollout.StepRollout) under the three policies' rollouts, at a shape where the env
count is no multiple of a wave (64) or of the pixel kernel's tile (4) and the horizon is no multiple of the
chunk: captured == eager bit for bit (both issue the same launches), close() twice, and step(t) of a fused
rollout raises."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T, CHUNK = 70, 5, 2


def _a2c(env, backend="hip"):
    from gym_ballenv_amd.policy import Policy, reference_weights
    from gym_ballenv_amd.rollout import Rollout
    return Rollout(env, Policy.from_npz(reference_weights(5), 5), horizon=T, backend=backend, seed=99)


def _block(env, backend="hip"):
    from gym_ballenv_amd.block_policy import BlockPolicy, BlockRollout, reference_block_weights
    pol = BlockPolicy.from_npz(reference_block_weights("supervised3"))
    return BlockRollout(env, pol, horizon=T, backend=backend, seed=99)


def _pixel(env, backend="hip"):
    from gym_ballenv_amd.pixel_policy import PixelRollout
    from pixel_policy_cases import random_policy
    assert backend == "hip"
    return PixelRollout(env, random_policy(0), horizon=T, seed=99)     # the trained one always moves one way here


@pytest.mark.parametrize("make,fused", [(_a2c, True), (_block, True), (_pixel, False)], ids=["a2c", "block", "pixel"])
def test_shared_loop_graph_equals_eager(gpu, make, fused):
    import gym_ballenv_amd as gb
    outs = []
    for mode in ("eager", "graph"):
        env = gb.BatchedBallEnv(N, 5, gb.EnvConfig(time_limit=3), device=gpu, seed=21)
        env.reset()
        ro = make(env)
        if mode == "eager":
            with pytest.raises(RuntimeError, match=r"capture\(\) first"):
                ro.run()
            ro.run_eager()
        else:
            ro.capture(chunk=CHUNK)
            assert len(ro._graphs) == 3             # 2 + 2 + 1 steps
            ro.run()
        torch.cuda.synchronize()
        outs.append([x.cpu().clone() for x in (ro.actions, ro.log_probs, ro.rewards, ro.dones)])
        assert tuple(ro.actions.shape) == (T, N) and (ro.values is not None) == (make is _a2c)
        env.status()
        hp = ro.hp
        ro.close()
        assert hp._h is None and ro._graphs == []
        ro.close()                                  # a second close is harmless
        hp.close()
        assert hp._h is None
        env.close()
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert int(outs[0][3].sum()) > 0                # the time limit ended episodes inside the horizon
    assert len(set(outs[0][0].reshape(-1).tolist())) > 1
    if fused:
        env = gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=gpu, seed=21)
        env.reset()
        ro = make(env, backend="fused")
        with pytest.raises(RuntimeError, match="fused"):
            ro.step(0)
        ro.capture(chunk=CHUNK)
        assert ro._graphs == []                     # nothing to capture
        ro.close()
        env.close()
