"""CPU tests of the block-count policy's Python side (gym_ballenv_amd/block_policy.py): the
reference's weights load, torch_block_select_action is Categorical's distribution, and
reinforce_losses is finish_episode (examples/ball_env_reinforce.py:88-108) run per env and per
episode.  No compute call of the library is made."""
import copy
import os

import numpy as np
import pytest
import torch

from gym_ballenv_amd import _abi
from gym_ballenv_amd.block_policy import (BlockPolicy, reference_block_weights, reinforce_losses,
                                          torch_block_select_action)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_reference_fixtures_load():
    sup = BlockPolicy.from_npz(reference_block_weights("supervised3"))
    assert (sup.layers, sup.final_relu, sup.num_actions) == (3, False, 9)
    assert {k: tuple(v.shape) for k, v in sup.state_dict().items()} == {
        "affine1.weight": (128, 29), "affine1.bias": (128,), "affine2.weight": (128, 128), "affine2.bias": (128,),
        "affine3.weight": (9, 128), "affine3.bias": (9,)}
    rf = BlockPolicy.from_npz(reference_block_weights("reinforce2"))
    assert (rf.layers, rf.final_relu, rf.num_actions) == (2, True, 9)
    assert {k: tuple(v.shape) for k, v in rf.state_dict().items()} == {
        "affine1.weight": (128, 29), "affine1.bias": (128,), "affine2.weight": (9, 128), "affine2.bias": (9,)}
    for kind in ("supervised3", "reinforce2"):
        d = np.load(os.path.join(GOLDEN, f"block_policy_{kind}.npz"), allow_pickle=False)
        assert str(d["source"]).startswith("examples/stored_models/")
        assert all(d[k].dtype == np.float32 for k in d.files if k.startswith("affine"))
    with pytest.raises(ValueError):
        reference_block_weights("nope")


@pytest.mark.parametrize("layers,final_relu", [(3, True), (2, False)])
def test_torch_select_action_is_categorical(layers, final_relu):
    torch.manual_seed(layers)
    pol = BlockPolicy(layers, (40, 24), num_actions=7, final_relu=final_relu)
    blocks = torch.randint(0, 5, (500, 29), dtype=torch.uint8)
    u = torch.rand(500)
    with torch.no_grad():
        a, lp, probs = torch_block_select_action(pol, blocks, u)
        cat = torch.distributions.Categorical(probs=pol(blocks.float()))
    # Categorical divides the probabilities by their sum once more: 1 up to a few fp32 roundings
    assert (probs - cat.probs).abs().max().item() <= 1e-6
    assert (lp - cat.log_prob(a)).abs().max().item() <= 1e-6
    # the inverse CDF: cdf[a-1] <= u < cdf[a] (the last action takes what rounding leaves of [0, 1))
    cdf = probs.cumsum(-1)
    lo = torch.where(a > 0, cdf.gather(-1, (a - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1), torch.zeros(500))
    hi = cdf.gather(-1, a.unsqueeze(-1)).squeeze(-1)
    assert bool((lo <= u).all()) and bool(((u < hi) | (a == 6)).all())
    # u = 1 - 2^-24 with a zero-probability tail: clamped to the last action with p > 0
    p2 = torch.tensor([[0.5, 0.5, 0.0]])

    class Fixed(torch.nn.Module):
        def forward(self, x):
            return p2

    a2, _, _ = torch_block_select_action(Fixed(), torch.zeros(1, 29), torch.tensor([1.0]))
    assert int(a2) == 1


def record(T=40, N=6, seed=3):
    """A small record with dones, a one-step episode and horizon-cut episodes."""
    g = torch.Generator().manual_seed(seed)
    blocks = torch.randint(0, 4, (T, N, 29), generator=g, dtype=torch.uint8)
    actions = torch.randint(0, 9, (T, N), generator=g, dtype=torch.uint8)
    rewards = torch.randn(T, N, generator=g, dtype=torch.float64)
    dones = torch.zeros(T, N, dtype=torch.bool)
    dones[7, 0] = dones[8, 0] = True          # env 0: steps 0..7, the one-step episode 8, then 9..39 cut
    dones[39, 1] = True                       # env 1: one episode that ends at the horizon
    dones[0, 2] = dones[20, 2] = True         # env 2: a one-step episode first
    dones[11, 3] = dones[25, 3] = dones[38, 3] = True     # env 3: ..., 26..38, then the one-step 39 cut
    dones[5, 5] = True                        # env 4: no done at all; env 5: 0..5, 6..39 cut
    return blocks, actions, rewards, dones


def finish_episode_loop(pol, blocks, actions, rewards, dones, gamma, dtype=torch.float32):
    """ball_env_reinforce.py:88-108 per env and per episode; the episodes' losses summed in f64.
    dtype=torch.float64 (with pol.double()): the same targets and the same clamp of the probabilities,
    the network and the loss in f64."""
    eps = float(np.finfo(np.float32).eps)                 # :22
    T, N = rewards.shape
    total, count, ones = 0.0, 0, 0
    for n in range(N):
        s = 0
        for e in range(T):
            if not (bool(dones[e, n]) or e == T - 1):
                continue
            if e == s:                                    # std() of one element is NaN: never trained on
                ones += 1
            else:
                R, rs = 0, []
                for r in rewards[s:e + 1, n].tolist()[::-1]:
                    R = r + gamma * R
                    rs.insert(0, R)
                rs = torch.tensor(rs)
                rs = (rs - rs.mean()) / (rs.std() + eps)
                policy_loss = []
                for t, reward in zip(range(s, e + 1), rs):
                    probs = pol(blocks[t, n].to(dtype).unsqueeze(0))
                    a = actions[t, n].long().unsqueeze(0)
                    if dtype == torch.float32:
                        logp = torch.distributions.Categorical(probs).log_prob(a)
                    else:       # Categorical's fp32 rule restated: renormalise, clamp to fp32's [eps, 1 - eps], log
                        logp = torch.log((probs / probs.sum(-1, keepdim=True)).clamp(eps, 1 - eps))[0, a]
                    policy_loss.append(-logp * reward.to(dtype))
                total = total + torch.cat(policy_loss).sum().double()
                count += 1
            s = e + 1
    return total, count, ones


@pytest.mark.parametrize("kind", ["supervised3", "reinforce2"])
def test_reinforce_losses_equal_finish_episode(kind):
    pol = BlockPolicy.from_npz(reference_block_weights(kind))
    blocks, actions, rewards, dones = record()
    ref, count, ones = finish_episode_loop(pol, blocks, actions, rewards, dones, 0.99)
    assert count >= 8 and ones >= 3
    pol.zero_grad()
    ref.backward()
    gref = {k: p.grad.clone() for k, p in pol.named_parameters()}
    pol.zero_grad()
    loss = reinforce_losses(pol, blocks, actions, rewards, dones, 0.99)
    loss.backward()
    rel = abs(float(loss.detach()) - float(ref.detach())) / abs(float(ref.detach()))
    print(f"{kind}: loss {float(loss.detach()):.9g} loop {float(ref.detach()):.9g} rel {rel:.3g}")
    assert rel <= 1e-6
    g32 = {k: p.grad.clone() for k, p in pol.named_parameters()}
    # The gradient: the loop's own .grad is an fp32 running sum over ~230 rows, so the two are compared
    # through an f64 run of the loop (the same fp32 targets, the network in f64) by the rule of
    # tests/test_gpu_policy.py: no farther from it than 4x the fp32 loop is, + 1e-6 of the largest entry.
    p64 = copy.deepcopy(pol).double()
    p64.zero_grad()
    finish_episode_loop(p64, blocks, actions, rewards, dones, 0.99, torch.float64)[0].backward()
    for k, p in p64.named_parameters():
        scale = p.grad.abs().max().item()
        err = (g32[k].double() - p.grad).abs().max().item()
        err_loop = (gref[k].double() - p.grad).abs().max().item()
        print(f"  grad {k}: |batched - f64| {err:.3g}, |loop32 - f64| {err_loop:.3g}, max |g| {scale:.3g}")
        assert err <= 4 * err_loop + 1e-6 * scale


def test_reinforce_losses_takes_given_targets():
    from gym_ballenv_amd.block_policy import _episode_targets
    pol = BlockPolicy.from_npz(reference_block_weights("reinforce2"))
    blocks, actions, rewards, dones = record()
    Rn, valid = _episode_targets(rewards, dones, 0.99, float(np.finfo(np.float32).eps))
    with torch.no_grad():
        a = reinforce_losses(pol, blocks, actions, rewards, dones, 0.99)
        b = reinforce_losses(pol, blocks, actions, rewards, dones, 0.99, targets=(Rn.reshape(40, 6), valid.reshape(40, 6)))
        assert torch.equal(a, b)
        with pytest.raises(ValueError):
            reinforce_losses(pol, blocks, actions, rewards, dones, 0.99, targets=(Rn, valid))


def test_library_exports_block_policy_entry_points():
    L = _abi.lib()
    for name in ("be_mlp_create", "be_mlp_load", "be_mlp_act", "be_mlp_bytes", "be_mlp_destroy"):
        assert hasattr(L, name), name
        assert name in _abi.EXPORTS
    assert L.be_abi_version() == 7
    import gym_ballenv_amd as gb
    for name in ("BlockPolicy", "HipBlockPolicy", "BlockRollout", "torch_block_select_action", "reinforce_losses",
                 "reinforce_update", "reference_block_weights"):
        assert getattr(gb, name) is not None
