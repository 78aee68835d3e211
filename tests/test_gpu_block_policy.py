"""GPU: be_mlp_act (csrc/mlp_policy.hip), HipBlockPolicy, BlockRollout and reinforce_update vs the
reference's REINFORCE / supervised policy (examples/ball_env_reinforce.py:57-85,
examples/train_supervise.py:11-28) run in plain PyTorch fp32 on the CPU.

Floating point, so a tolerance -- the rule of tests/test_gpu_policy.py, restated:
* probs, log_prob: |hip - torch32| <= 2e-5 (abs), and the HIP error against an fp64 evaluation of the
  same weights is at most 4x torch fp32's own error + 1e-6;
* action: identical to the inverse-CDF draw on the torch probs with the same Philox uniform
  (oracle.policy_uniforms), except where that uniform lies within 1e-5 of a CDF boundary; those
  cases are counted and capped at max(4, N // 1000).
Everything else (the blocks record, blocks_in against the fused path, tiles against stand-alone
runs, captured against eager) is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = 2e-5


def make(dev, N, seed=0x1234, W=5):
    import gym_ballenv_amd as gb
    env = gb.BatchedBallEnv(N, W, gb.EnvConfig(), device=dev, seed=seed)
    env.reset()
    return env


def ref_policy(kind):
    from gym_ballenv_amd.block_policy import BlockPolicy, reference_block_weights
    return BlockPolicy.from_npz(reference_block_weights(kind))


def random_policy(layers, h1, h2, A, final_relu, seed):
    from gym_ballenv_amd.block_policy import BlockPolicy
    torch.manual_seed(seed)
    pol = BlockPolicy(layers, (h1, h2), num_actions=A, final_relu=final_relu)
    with torch.no_grad():
        for prm in pol.parameters():
            prm.mul_(3.0)        # wider logits than init
    return pol


def random_rows(N, seed):
    """Counts in 0..19, then all-zero rows and a row with all 18 obstacles in one cell."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, 20, (N, 29), generator=g, dtype=torch.uint8)
    rows[N // 10: N // 5] = 0
    rows[0] = 0
    rows[0, 1] = 1
    rows[0, 16] = 1
    rows[0, 9] = 18
    return rows


def uniforms(env, seed):
    ep = env.episode.cpu().numpy().view(np.uint32)
    return torch.from_numpy(oracle.policy_uniforms(env._abi_cfg, ep, env.ep_len.cpu().numpy(), seed))


def reference(pol, rows, u):
    """(action, log_prob, probs) of torch fp32 and the fp64 probs, on the CPU."""
    from gym_ballenv_amd.block_policy import torch_block_select_action
    with torch.no_grad():
        ra, rlp, rpr = torch_block_select_action(pol.float(), rows, u)
        pr64 = pol.double()(rows.double())
        pol.float()
    return ra, rlp, rpr, pr64


def near_boundary(rpr, u):
    return ((rpr.cumsum(-1) - u.unsqueeze(-1)).abs() < 1e-5).any(-1)


def check(got, ref, u):
    a, lp, pr = (x.cpu() for x in got)
    ra, rlp, rpr, pr64 = ref
    err_hip = (pr.double() - pr64).abs().max().item()
    err_t32 = (rpr.double() - pr64).abs().max().item()
    d = (pr - rpr).abs().max().item()
    near = near_boundary(rpr, u)
    mism = a.long() != ra
    ok = ~mism
    dlp = (lp[ok] - rlp[ok]).abs().max().item()
    print(f"|probs - t32| {d:.3g}  |log_prob - t32| {dlp:.3g}  err_hip {err_hip:.3g}  err_t32 {err_t32:.3g}  "
          f"near {int(near.sum())}  mismatches {int(mism.sum())} of {a.shape[0]}")
    assert d <= TOL
    assert err_hip <= 4 * err_t32 + 1e-6, (err_hip, err_t32)
    assert not (mism & ~near).any(), f"{int((mism & ~near).sum())} action mismatches away from CDF boundaries"
    assert int(near.sum()) <= max(4, a.shape[0] // 1000)
    assert dlp <= TOL


def check_env(env, pol, hp, seed, rows=None):
    """act() on the env's state (rows=None) or on given rows, against torch on the same rows."""
    src = env.observe_blocks() if rows is None else rows
    got = [x.clone() for x in hp.act(rows, seed=seed)]
    u = uniforms(env, seed)
    check(got, reference(pol, src.cpu(), u), u)
    return got


@pytest.mark.parametrize("kind", ["supervised3", "reinforce2"])
def test_reference_weights_on_env_states(gpu, kind):
    """The reference's trained weights on env states along a random rollout, blocks_in = NULL; the
    blocks record equals be_observe_blocks."""
    from gym_ballenv_amd.block_policy import HipBlockPolicy
    env = make(gpu, 4096)
    pol = ref_policy(kind)
    hp = HipBlockPolicy(env, pol, probs=True)
    acts = env.sample_actions(40, seed=9)
    rec = torch.zeros(4096, 29, dtype=torch.uint8, device=gpu)
    seen = 0
    for t in range(40):
        env.step(acts[t])
        if t % 8 == 7:
            check_env(env, pol, hp, seed=77 + t)
            want = env.observe_blocks()
            rec.fill_(255)
            a = hp.act(record=rec, seed=77 + t)[0].clone()
            assert torch.equal(rec, want)
            assert torch.equal(a, hp.act(seed=77 + t)[0])          # the record changes nothing
            seen += int((want[:, 4:].sum(1) > 1).sum())             # byte 16 is the agent's own cell
    assert seen > 0          # some rows have a nonzero obstacle count
    hp.close(); env.close()


def test_blocks_in_equals_fused_path(gpu):
    from gym_ballenv_amd.block_policy import HipBlockPolicy
    env = make(gpu, 3000, seed=8)
    acts = env.sample_actions(30, seed=4)
    for t in range(30):
        env.step(acts[t])
    for kind in ("supervised3", "reinforce2"):
        hp = HipBlockPolicy(env, ref_policy(kind), probs=True)
        fused = [x.clone() for x in hp.act(seed=6)]
        given = [x.clone() for x in hp.act(blocks=env.observe_blocks(), seed=6)]
        for x, y in zip(fused, given):
            assert torch.equal(x, y)
        # both at once: the forward runs on the caller's rows, the record is still the state's
        other = env.observe_blocks().roll(1, 0).contiguous()
        want = [x.clone() for x in hp.act(blocks=other, seed=6)]
        rec = torch.full((3000, 29), 255, dtype=torch.uint8, device=gpu)
        both = hp.act(blocks=other, record=rec, seed=6)
        for x, y in zip(want, both):
            assert torch.equal(x, y)
        assert torch.equal(rec, env.observe_blocks()) and not torch.equal(want[2], fused[2])
        hp.close()
    env.close()


SHAPES = [(3, 128, 128, 9, True, 1000), (3, 100, 37, 5, False, 333), (2, 128, 0, 9, True, 130),
          (2, 16, 0, 1, False, 70), (3, 1, 1, 15, True, 64), (3, 17, 128, 15, False, 65)]


@pytest.mark.parametrize("layers,h1,h2,A,final_relu,N", SHAPES)
def test_shapes_random_weights_and_rows(gpu, layers, h1, h2, A, final_relu, N):
    """Random weights x3 on random counts, all-zero rows and 18 obstacles in one cell: hidden sizes off and
    on multiples of 16, both ends of the action bound, N on both sides of a wave and a tile edge."""
    from gym_ballenv_amd.block_policy import HipBlockPolicy
    env = make(gpu, N)
    pol = random_policy(layers, h1, h2, A, final_relu, seed=1000 * h1 + A)
    hp = HipBlockPolicy(env, pol, probs=True)
    check_env(env, pol, hp, seed=5, rows=random_rows(N, N).to(gpu))
    hp.close(); env.close()


def test_tile_loop(gpu):
    """Every wave of the persistent grid takes more than one tile, the last tile is partial; a tile of a
    later round equals a stand-alone run of its 16 rows, and the same rows in a first-round tile.
    The rows are env states: on the trained weights, counts of 0..19 in every cell give logits near 190,
    where torch fp32's own log_prob is 6e-5 from fp64 -- no fp32 forward meets 2e-5 there."""
    from gym_ballenv_amd.block_policy import HipBlockPolicy, TILE, WAVES
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    slots = cus * WAVES                                   # waves of the grid = tiles per round
    N = 2 * slots * TILE + 5 * TILE + 7
    ntiles = -(-N // TILE)
    assert ntiles >= 2 * slots and ntiles % slots != 0 and N % TILE != 0
    env = make(gpu, N, W=3)
    pol = ref_policy("supervised3")
    hp = HipBlockPolicy(env, pol, probs=True)
    acts = env.sample_actions(10, seed=5)
    for t in range(10):
        env.step(acts[t])
    rows = env.observe_blocks()
    full = check_env(env, pol, hp, seed=21)               # blocks_in = NULL: the tile loop loads the state
    late, first = (slots + 3) * TILE, 3 * TILE            # wave 0 of workgroup 3: its second and first round
    alone = torch.zeros_like(rows)
    alone[late:late + TILE] = rows[late:late + TILE]
    alone[first:first + TILE] = rows[late:late + TILE]
    got = [x.clone() for x in hp.act(alone, seed=21)]
    for x, y in zip(got, full):
        assert torch.equal(x[late:late + TILE], y[late:late + TILE])
    assert torch.equal(got[2][first:first + TILE], full[2][late:late + TILE])
    last = (ntiles - 1) * TILE                            # the partial tile, on its own
    alone.zero_()
    alone[last:] = rows[last:]
    got = [x.clone() for x in hp.act(alone, seed=21)]
    for x, y in zip(got, full):
        assert torch.equal(x[last:], y[last:])
    hp.close(); env.close()


def test_determinism_and_reload(gpu):
    from gym_ballenv_amd.block_policy import HipBlockPolicy
    env = make(gpu, 2048)
    pol = ref_policy("supervised3")
    hp = HipBlockPolicy(env, pol, probs=True)
    r1 = [x.clone() for x in hp.act(seed=3)]
    r2 = [x.clone() for x in hp.act(seed=3)]
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)
    assert not torch.equal(r1[0], hp.act(seed=4)[0])
    pol2 = random_policy(3, 128, 128, 9, False, seed=11)
    hp.load(pol2)
    check_env(env, pol2, hp, seed=3)
    with pytest.raises(ValueError):
        hp.load(ref_policy("reinforce2"))
    with pytest.raises(ValueError):
        hp.act(blocks=torch.zeros(2048, 28, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError):
        hp.act(record=torch.zeros(2048, 29, dtype=torch.float32, device=gpu))
    hp.close(); env.close()


def test_rejections(gpu):
    """Bad arguments return an error with a be_last_error text; nothing is launched."""
    from gym_ballenv_amd import _abi
    from gym_ballenv_amd.block_policy import HipBlockPolicy
    L = _abi.lib()
    env = make(gpu, 256)

    def last_error():
        return (L.be_last_error(env._ctx) or b"").decode()

    for args, word in (((4, 128, 128, 9, 1), "layers"), ((3, 129, 128, 9, 1), "hidden1"),
                       ((3, 128, 128, 16, 1), "num_actions"), ((3, 128, 129, 9, 1), "hidden2"),
                       ((2, 128, 0, 0, 1), "num_actions")):
        h = C.c_void_p()
        assert L.be_mlp_create(env._ctx, *args, C.byref(h)) == _abi.BE_E_INVALID
        assert not h.value and word in last_error()
    hp = HipBlockPolicy(env, ref_policy("reinforce2"))
    action = torch.full((256,), 200, dtype=torch.uint8, device=gpu)
    value = torch.zeros(256, dtype=torch.float32, device=gpu)
    out = _abi.BeActOut(action.data_ptr(), None, value.data_ptr(), None)
    rc = L.be_mlp_act(hp._h, C.byref(env._st), None, None, C.byref(out), 1, env._stream())
    assert rc == _abi.BE_E_INVALID and "value" in last_error()
    out = _abi.BeActOut(None, None, None, None)
    assert L.be_mlp_act(hp._h, C.byref(env._st), None, None, C.byref(out), 1, env._stream()) == _abi.BE_E_INVALID
    assert "action" in last_error()
    torch.cuda.synchronize()
    assert bool((action == 200).all())                    # no launch wrote it
    env.status()
    hp.close(); env.close()


def test_block_rollout_graph_eager_and_hand_loop(gpu):
    """Captured == eager == a hand loop of HipBlockPolicy.act() + env.step(), bit for bit; blocks[t] is the
    observation actions[t] was drawn from."""
    from gym_ballenv_amd.block_policy import BlockRollout, HipBlockPolicy
    pol = ref_policy("supervised3")
    N, T = 1024, 64
    outs = []
    for chunk in (None, 32, 64, 24):          # eager; two graphs, one graph, ragged chunks (24, 24, 16)
        env = make(gpu, N, seed=21)
        ro = BlockRollout(env, pol, horizon=T, record_obs=True, seed=99)
        if chunk is None:
            ro.run_eager()
        else:
            ro.capture(chunk=chunk)
            assert len(ro._graphs) == -(-T // chunk)
            ro.run()
        torch.cuda.synchronize()
        outs.append([x.cpu().clone() for x in (ro.actions, ro.log_probs, ro.rewards, ro.dones, ro.blocks)])
        env.status()
        ro.close(); env.close()
    env = make(gpu, N, seed=21)
    hp = HipBlockPolicy(env, pol, seed=99)
    hand = [[], [], [], [], []]
    for t in range(T):
        hand[4].append(env.observe_blocks().cpu())
        a, lp, _ = hp.act()
        hand[0].append(a.cpu()); hand[1].append(lp.cpu())
        _, r, d, _ = env.step(a)
        hand[2].append(r.cpu()); hand[3].append(d.cpu())
    outs.append([torch.stack(x) for x in hand])
    hp.close(); env.close()
    assert int(outs[0][3].sum()) > 0                      # some episodes ended inside the horizon
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x, y)


def test_reinforce_update(gpu):
    """captured rollout (HIP) -> reinforce_update (be_a2c_targets + torch autograd on the recorded rows) ->
    re-pack, three times: the loss is finite, the weights move, and the kernel then acts with the new weights."""
    import copy
    from gym_ballenv_amd.block_policy import BlockRollout, reinforce_update
    pol = ref_policy("supervised3").to(gpu)
    w0 = copy.deepcopy(pol.state_dict())
    env = make(gpu, 512, seed=3)
    ro = BlockRollout(env, pol, horizon=32, record_obs=True, seed=2)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-2)
    ro.capture(chunk=32)                      # the replays must pick up each re-pack of the weights
    for it in range(3):
        ro.run()
        loss = reinforce_update(ro, opt, gamma=0.99)
        assert np.isfinite(loss)
    for k, v in pol.state_dict().items():
        assert not torch.equal(w0[k], v), k
    from gym_ballenv_amd.block_policy import HipBlockPolicy
    hp2 = HipBlockPolicy(env, pol, probs=True)
    a_new = check_env(env, copy.deepcopy(pol).cpu(), hp2, seed=9)[0]
    assert torch.equal(ro.hp.act(seed=9)[0], a_new)       # the rollout's kernel was re-packed
    hp2.close(); ro.close(); env.close()
