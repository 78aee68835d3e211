"""GPU: be_cnn_act (csrc/cnn_policy.hip), HipPixelPolicy and PixelRollout vs the reference's pixel
policy (examples/ball_cnn_reinforce.py:60-95) run in plain PyTorch fp32 on the CPU
(torch_pixel_select_action), in both BatchNorm modes.

Floating point, so a tolerance -- the rule of tests/test_gpu_block_policy.py, taken over as it stands:
* probs, log_prob: |hip - torch32| <= 2e-5 (abs), and the HIP error against an fp64 evaluation of the
  same weights is at most 4x torch fp32's own error + 1e-6;
* the centred logits z = log p - mean log p, which a saturated softmax cannot hide:
  |z_hip - z64| <= 4 |z_t32 - z64| + 8 * 2**-23 * (1 + max|z64|) (pixel_policy_cases.logit_bound);
* action: identical to the inverse-CDF draw on the torch probs with the same Philox uniform
  (oracle.policy_uniforms), except where that uniform lies within 1e-5 of a CDF boundary; those
  cases are counted and capped at max(4, N // 1000).
Everything else (rolled rows, tiles against stand-alone runs, the paths of act(), captured against
eager, the rollouts) is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle
from pixel_policy_cases import (ACTION_COUNTS, ACTION_N, ACTION_SEED, CALIBRATED_SHAPES, CASES, RANDOM_SHAPES, Case, case_inputs,
                                centred_logits, given_images, logit_bound, random_policy, reference, trained_policy)

pytestmark = pytest.mark.gpu

TOL = 2e-5


def make(dev, N, seed=0x1234, W=10, time_limit=1000):
    import gym_ballenv_amd as gb
    env = gb.BatchedBallEnv(N, W, gb.EnvConfig(time_limit=time_limit), device=dev, seed=seed)
    env.reset()
    return env


def uniforms(env, seed):
    ep = env.episode.cpu().numpy().view(np.uint32)
    return torch.from_numpy(oracle.policy_uniforms(env._abi_cfg, ep, env.ep_len.cpu().numpy(), seed))


def env_quadrant(env):
    return env.observe_blocks()[:, :4].argmax(1).to(torch.uint8)


def near_boundary(rpr, u):
    return ((rpr.cumsum(-1) - u.unsqueeze(-1)).abs() < 1e-5).any(-1)


def check(got, ref, u, masked=False):
    """masked: whether the fp64 reference may have probabilities below 1e-30, which the logit comparison leaves
    out (the trained weights; never a random or calibrated policy)."""
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
    # the centred logits log p - mean log p of the f32 probabilities, the log taken in fp64: the bound is from the
    # two references alone (pixel_policy_cases.logit_bound)
    z64, mask = centred_logits(pr64)
    z32, _ = centred_logits(rpr.double(), mask)
    zhip, _ = centred_logits(pr.double(), mask)
    bound = logit_bound(z64, z32)
    zerr_hip, zerr_t32 = (zhip - z64).abs().max().item(), (z32 - z64).abs().max().item()
    print(f"logits: err_hip {zerr_hip:.3g}  err_t32 {zerr_t32:.3g}  logit_bound {bound:.3g}  max|z| {z64.abs().max().item():.3g}  "
          f"min p {pr64.min().item():.3g}  masked {int(mask.sum())} of {mask.numel()}")
    assert torch.isfinite(pr).all()
    assert d <= TOL
    assert err_hip <= 4 * err_t32 + 1e-6, (err_hip, err_t32)
    assert int(mask.sum()) <= (mask.numel() // 100 if masked else 0)
    assert zerr_hip <= bound, (zerr_hip, zerr_t32, bound)
    assert not (mism & ~near).any(), f"{int((mism & ~near).sum())} action mismatches away from CDF boundaries"
    assert int(near.sum()) <= max(4, a.shape[0] // 1000)
    assert dlp <= TOL


def check_env(env, pol, hp, seed, img=None, quad=None, masked=False):
    """act() on the env's state (img = quad = None) or on given inputs, against torch on the same inputs."""
    src = env.observe_pixels() if img is None else img
    q = env_quadrant(env) if quad is None else quad
    got = [x.clone() for x in hp.act(img, quad, seed=seed)]
    u = uniforms(env, seed)
    check(got, reference(pol, src.cpu(), q.cpu(), u, hp.norm), u, masked)
    return got


def test_trained_weights_on_env_states(gpu):
    """The reference's trained weights, its own normalisation, on env states along a random rollout with
    autoreset: act() observes and computes the quadrant itself."""
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy
    N = 301
    env = make(gpu, N, time_limit=30)
    pol = trained_policy()
    hp = HipPixelPolicy(env, pol, norm="sample", probs=True)
    acts = env.sample_actions(40, seed=9)
    resets = 0
    for t in range(40):
        _, _, done, _ = env.step(acts[t])
        resets += int(done.sum())
        if t in (19, 39):
            got = check_env(env, pol, hp, seed=77 + t, masked=True)
            assert got[2].max().item() < 1.0 and got[2].min().item() > 0.0
    assert resets >= N                                   # every env was reset by the time limit
    env.status()
    hp.close(); env.close()


@pytest.mark.parametrize("norm", ["sample", "running"])
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("N,A", RANDOM_SHAPES)
def test_random_weights_given_images(gpu, N, A, seed, norm):
    """Random weights on the fixture images, noise, constant images (every map constant: variance 0, the eps
    path) and a single black pixel; quadrant_in covers 0..3; N on both sides of a tile and of a wave's share,
    both ends of the action bound.  In "running" mode these are the large-logit cases (probabilities down to
    1e-11); half the channels of conv2 and conv3 are dead there, which the calibrated cases make up for."""
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy
    case = Case("random", norm, N, A, seed)
    assert case in CASES
    env = make(gpu, N, W=3)
    pol, img, quad = case_inputs(case)
    hp = HipPixelPolicy(env, pol, norm=norm, probs=True)
    check_env(env, pol, hp, seed=5 + seed, img=img.to(gpu), quad=quad.to(gpu))
    hp.close(); env.close()


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("N,A", CALIBRATED_SHAPES)
def test_calibrated_weights_given_images(gpu, N, A, seed):
    """"running" mode with the running statistics a real eval-mode net has: each layer's pooled statistics over
    the test's images.  Every channel is then alive on some image, and this is the mode in which the conv
    biases matter: tests/test_pixel_policy_coverage_host.py shows that these cases see the whole packed image."""
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy
    case = Case("calibrated", "running", N, A, seed)
    assert case in CASES
    env = make(gpu, N, W=3)
    pol, img, quad = case_inputs(case)
    hp = HipPixelPolicy(env, pol, norm="running", probs=True)
    check_env(env, pol, hp, seed=5 + seed, img=img.to(gpu), quad=quad.to(gpu))
    hp.close(); env.close()


@pytest.mark.parametrize("A", ACTION_COUNTS)
def test_every_action_count(gpu, A):
    """One full tile and a partial one for every number of -inf pad rows of the head: probs, logits and the
    draw against torch; a single action has probability exactly 1."""
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy
    case = Case("actions", "sample", ACTION_N, A, ACTION_SEED)
    assert case in CASES
    env = make(gpu, ACTION_N, W=3)
    pol, img, quad = case_inputs(case)
    hp = HipPixelPolicy(env, pol, norm="sample", probs=True)
    a, lp, pr = check_env(env, pol, hp, seed=40 + A, img=img.to(gpu), quad=quad.to(gpu))
    assert pr.shape == (ACTION_N, A) and int(a.max()) < A
    if A == 1:
        assert bool((pr == 1.0).all()) and bool((a == 0).all()) and bool((lp == 0.0).all())
    hp.close(); env.close()


# goal - agent for 16 envs: dx in {< 0, 0, 0, > 0} crossed with dy in {< 0, 0, 0, > 0}, so each zero meets every
# sign of the other coordinate; and blocks_init's rule dx >= 0 ? (dy >= 0 ? 1 : 2) : (dy >= 0 ? 0 : 3) by hand
CUT_DX = [-7, -7, -7, -7, 0, 0, 0, 0, 0, 0, 0, 0, 5, 5, 5, 5]
CUT_DY = [-3, 0, 0, 9] * 4
CUT_QUADRANT = [3, 0, 0, 0, 2, 1, 1, 1, 2, 1, 1, 1, 2, 1, 1, 1]


def test_quadrant_from_the_state_at_its_cuts(gpu):
    """The kernel restates blocks_init's quadrant rule inline: with quadrant=None it must give what it gives on
    be_observe_blocks' quadrant and on the rule written out by hand, bit for bit, where dx or dy is 0."""
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy
    N = 16
    env = make(gpu, N)
    state = {k: v.clone() for k, v in env.state_dict().items()}
    agent = torch.tensor([[200 + 9 * i, 150 + 5 * i] for i in range(N)], dtype=state["agent"].dtype)
    delta = torch.tensor(list(zip(CUT_DX, CUT_DY)), dtype=state["agent"].dtype)
    assert tuple(state["agent"].shape) == (N, 2) and tuple(state["goal"].shape) == (N, 2)
    state["agent"], state["goal"] = agent, agent + delta
    env.load_state_dict(state)
    assert torch.equal(env.goal.cpu() - env.agent.cpu(), delta)
    by_hand = torch.tensor(CUT_QUADRANT, dtype=torch.uint8, device=gpu)
    assert torch.equal(env_quadrant(env), by_hand) and set(CUT_QUADRANT) == {0, 1, 2, 3}
    pol = random_policy(3)
    for norm in ("sample", "running"):
        hp = HipPixelPolicy(env, pol, norm=norm, probs=True)
        own = check_env(env, pol, hp, seed=12)
        for q in (env_quadrant(env), by_hand):
            for x, y in zip(own, hp.act(quadrant=q, seed=12)):
                assert torch.equal(x, y)
        other = hp.act(quadrant=(by_hand + 1) % 4, seed=12)[2]
        assert bool((other != own[2]).any(1).all())         # the head's quadrant columns matter in every row
        hp.close()
    env.status()
    env.close()


def test_env_offset_keys_the_draw(gpu):
    """The draw's Philox key is the global env id env_offset + e (past 16 bits here); nothing else depends on it."""
    import gym_ballenv_amd as gb
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy
    N, seed = 70, 17
    pol = random_policy(5)
    img, quad = given_images(N, 2)
    outs = []
    for offset in (0, 70000):
        env = gb.BatchedBallEnv(N, 3, gb.EnvConfig(time_limit=1000), device=gpu, seed=0x1234, env_offset=offset)
        env.reset()
        assert env._abi_cfg.env_offset == offset
        hp = HipPixelPolicy(env, pol, norm="sample", probs=True)
        outs.append(check_env(env, pol, hp, seed=seed, img=img.to(gpu), quad=quad.to(gpu)))
        outs[-1].append(uniforms(env, seed))
        env.status()
        hp.close(); env.close()
    assert torch.equal(outs[0][2], outs[1][2])
    assert not torch.equal(outs[0][3], outs[1][3])
    assert not torch.equal(outs[0][0], outs[1][0])


def test_position_independence(gpu):
    """Every workgroup of the persistent grid takes a second round and the last tile is partial.  Rolling the
    rows of image and quadrant_in by 5 rolls probs by 5, and log_prob wherever the rolled run drew the action
    the base run drew for that row (the draw's uniform is keyed by the env, not by the row's content); a tile
    of the second round equals a stand-alone run of its rows, and the same rows in a first-round tile; 64 rows
    also against torch."""
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy, TILE
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    N = 2 * cus * TILE + 3 * TILE + 2
    ntiles = -(-N // TILE)
    assert ntiles >= 2 * cus and ntiles % cus != 0 and N % TILE != 0
    env = make(gpu, N, W=3)
    pol = random_policy(7)
    img, quad = given_images(N, 3)
    img, quad = img.to(gpu), quad.to(gpu)
    for norm in ("sample", "running"):
        hp = HipPixelPolicy(env, pol, norm=norm, probs=True)
        full = [x.clone() for x in hp.act(img, quad, seed=21)]
        rolled = [x.clone() for x in hp.act(img.roll(5, 0).contiguous(), quad.roll(5, 0).contiguous(), seed=21)]
        assert torch.equal(rolled[2], full[2].roll(5, 0))
        same = rolled[0] == full[0].roll(5, 0)
        assert int(same.sum()) >= N // 8
        assert torch.equal(rolled[1][same], full[1].roll(5, 0)[same])
        late, first = (cus + 3) * TILE, 3 * TILE           # workgroup 3: its second and first round
        alone_img, alone_q = torch.zeros_like(img), torch.zeros_like(quad)
        alone_img[late:late + TILE], alone_q[late:late + TILE] = img[late:late + TILE], quad[late:late + TILE]
        alone_img[first:first + TILE], alone_q[first:first + TILE] = img[late:late + TILE], quad[late:late + TILE]
        got = [x.clone() for x in hp.act(alone_img, alone_q, seed=21)]
        for x, y in zip(got, full):
            assert torch.equal(x[late:late + TILE], y[late:late + TILE])
        assert torch.equal(got[2][first:first + TILE], full[2][late:late + TILE])
        last = (ntiles - 1) * TILE                          # the partial tile, on its own
        alone_img.zero_(); alone_q.zero_()
        alone_img[last:], alone_q[last:] = img[last:], quad[last:]
        got = [x.clone() for x in hp.act(alone_img, alone_q, seed=21)]
        for x, y in zip(got, full):
            assert torch.equal(x[last:], y[last:])
        idx = torch.cat([torch.arange(late - 30, late + 30), torch.arange(N - 4, N)])    # both rounds, the partial tile
        u = uniforms(env, 21)[idx]
        check([x[idx.to(gpu)] for x in full], reference(pol, img[idx.to(gpu)].cpu(), quad[idx.to(gpu)].cpu(), u, norm), u)
        hp.close()
    env.close()


def test_paths_agree(gpu):
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy
    N = 301
    env = make(gpu, N, seed=8)
    acts = env.sample_actions(12, seed=4)
    for t in range(12):
        env.step(acts[t])
    pol = trained_policy()
    hp = HipPixelPolicy(env, pol, probs=True)
    state = {k: v.clone() for k, v in env.state_dict().items()}
    own = [x.clone() for x in hp.act(seed=6)]
    given = [x.clone() for x in hp.act(image=env.observe_pixels(), seed=6)]
    quad = [x.clone() for x in hp.act(quadrant=env_quadrant(env), seed=6)]
    again = [x.clone() for x in hp.act(seed=6)]
    for other in (given, quad, again):
        for x, y in zip(own, other):
            assert torch.equal(x, y)
    assert torch.equal(hp.image, env.observe_pixels())          # act() observed into its own buffer
    assert not torch.equal(own[0], hp.act(seed=7)[0])
    for k, v in env.state_dict().items():
        assert torch.equal(v, state[k]), k                       # act changes no state
    env.status()
    pol2 = random_policy(11)
    hp.load(pol2)
    check_env(env, pol2, hp, seed=3)
    from gym_ballenv_amd.pixel_policy import PixelPolicy
    with pytest.raises(ValueError):
        hp.load(PixelPolicy(5))
    with pytest.raises(ValueError):
        hp.act(image=torch.zeros(N, 3, 40, 40, dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError):
        hp.act(quadrant=torch.zeros(N + 1, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError):
        HipPixelPolicy(env, pol, norm="batch")
    hp.close(); env.close()


def test_rejections(gpu):
    """Bad arguments return BE_E_INVALID with a be_last_error text that names them; nothing is launched."""
    from gym_ballenv_amd import _abi
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy
    L = _abi.lib()
    N = 64
    env = make(gpu, N, W=3)

    def last_error():
        return (L.be_last_error(env._ctx) or b"").decode()

    for A in (0, 16, -1):
        h = C.c_void_p()
        assert L.be_cnn_create(env._ctx, A, C.byref(h)) == _abi.BE_E_INVALID
        assert not h.value and "num_actions" in last_error()
    hp = HipPixelPolicy(env, random_policy(0))
    image = torch.zeros(N * 4800 + 16, dtype=torch.uint8, device=gpu)
    action = torch.full((N,), 200, dtype=torch.uint8, device=gpu)
    value = torch.zeros(N, dtype=torch.float32, device=gpu)
    good = _abi.BeActOut(action.data_ptr(), None, None, None)
    st, s = C.byref(env._st), env._stream()
    ptr = image.data_ptr()
    assert ptr % 16 == 0
    for args, word in (((ptr, None, 2, C.byref(good)), "norm"),
                       ((ptr, None, -1, C.byref(good)), "norm"),
                       ((ptr + 4, None, 0, C.byref(good)), "image"),
                       ((None, None, 0, C.byref(good)), "image"),
                       ((ptr, None, 0, C.byref(_abi.BeActOut(action.data_ptr(), None, value.data_ptr(), None))), "value"),
                       ((ptr, None, 0, C.byref(_abi.BeActOut(None, None, None, None))), "action")):
        assert L.be_cnn_act(hp._h, st, *args, 1, s) == _abi.BE_E_INVALID
        assert word in last_error(), (word, last_error())
    h = C.c_void_p()
    assert L.be_cnn_create(env._ctx, 9, C.byref(h)) == _abi.BE_OK
    assert L.be_cnn_act(h, st, ptr, None, 0, C.byref(good), 1, s) == _abi.BE_E_INVALID      # never loaded
    assert "be_cnn_load" in last_error()
    w = _abi.BeCnnWeights()
    assert L.be_cnn_load(h, C.byref(w), s) == _abi.BE_E_INVALID and "conv1_weight" in last_error()
    assert L.be_cnn_act(h, st, ptr, None, 0, C.byref(good), 1, s) == _abi.BE_E_INVALID      # still not loaded
    assert L.be_cnn_destroy(h) == _abi.BE_OK
    torch.cuda.synchronize()
    assert bool((action == 200).all())                    # no launch wrote it
    env.status()
    hp.close(); env.close()


def test_graph_capture(gpu):
    """observe_pixels(out=) + be_cnn_act captured on a side stream; a replay after 9 env steps equals eager on
    the new state."""
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy
    from gym_ballenv_amd.rollout import capture_graph
    N = 301
    env = make(gpu, N, seed=5)
    hp = HipPixelPolicy(env, trained_policy(), probs=True, seed=31)
    hp.act()
    torch.cuda.synchronize()
    g = capture_graph(lambda: hp.act(), gpu, torch.cuda.Stream(gpu))
    acts = env.sample_actions(9, seed=2)
    for t in range(9):
        env.step(acts[t])
    for x in (hp.action, hp.log_prob, hp.probs, hp.image):
        x.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in (hp.action, hp.log_prob, hp.probs, hp.image)]
    want = [x.clone() for x in hp.act()] + [env.observe_pixels()]
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert got[2].sum().item() > 0
    env.status()
    hp.close(); env.close()


def test_pixel_rollout_graph_eager_and_hand_loop(gpu):
    """Captured in ragged chunks == one graph == eager == a hand loop of HipPixelPolicy.act() + env.step(), bit
    for bit; images[t] is the observation actions[t] was drawn from."""
    from gym_ballenv_amd.pixel_policy import HipPixelPolicy, PixelRollout
    pol = trained_policy()
    N, T = 301, 40
    outs = []
    for chunk in (16, 40, None):              # ragged chunks (16, 16, 8); one graph; eager
        env = make(gpu, N, seed=21, time_limit=30)
        ro = PixelRollout(env, pol, horizon=T, seed=99, record_images=True)
        if chunk is None:
            ro.run_eager()
        else:
            ro.capture(chunk=chunk)
            assert len(ro._graphs) == -(-T // chunk)
            ro.run()
        torch.cuda.synchronize()
        outs.append([x.cpu().clone() for x in (ro.actions, ro.log_probs, ro.rewards, ro.dones, ro.images)])
        env.status()
        ro.close(); env.close()
    env = make(gpu, N, seed=21, time_limit=30)
    hp = HipPixelPolicy(env, pol, seed=99)
    hand = [[], [], [], [], []]
    for t in range(T):
        hand[4].append(env.observe_pixels().cpu())
        a, lp, _ = hp.act()
        hand[0].append(a.cpu()); hand[1].append(lp.cpu())
        _, r, d, _ = env.step(a)
        hand[2].append(r.cpu()); hand[3].append(d.cpu())
    outs.append([torch.stack(x) for x in hand])
    hp.close(); env.close()
    assert int(outs[0][3].sum()) > 0                      # some episodes ended inside the horizon
    assert len(set(outs[0][0].reshape(-1).tolist())) > 1
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x, y)
