"""be_a2c_adam on the GPU: bit-equal to the numpy restatement (tests/a2c_adam_ref.py), its re-packed
image equal to a fresh HipPolicy.load of the new weights (select_action and the fused rollout),
deterministic and graph-capturable with the state advancing on the device, a drop-in optimizer for
a2c_update, the engine of A2CTrainer, and interchangeable with torch.optim.Adam's state_dict."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from a2c_adam_ref import PARAMS, adam_step_ref, fresh_state
from a2c_ref import EPS as F32_EPS

pytestmark = pytest.mark.gpu

# (W, hidden, A): the two exact layouts; odd F = 53 < 64 with padded rows inside the last tile; the bounds
# (F = 125: two columns per lane); the generic layout through a non-9 action count
CASES = [(10, 208, 9), (5, 128, 9), (7, 72, 9), (11, 256, 9), (5, 128, 4)]
BETAS, EPS, LR = (0.9, 0.999), 1e-8, 1e-3
SPECIAL = (0.0, 1e-30, -1e-30, 1e4, -1e4)
# the bit-equality test also runs the ends of the accepted ranges: one hidden unit and one action (255
# padded rows), and 15 actions (the value head in lane 15 next to them) with a 17th row alone in its tile
EDGES = [(5, 1, 1), (7, 17, 15)]


def _env(gpu, W, N=256, seed=3):
    import gym_ballenv_amd as gb
    return gb.BatchedBallEnv(N, W, gb.EnvConfig(), device=gpu, seed=seed)


def _policy(gpu, W, H, A, seed=0):
    from gym_ballenv_amd.policy import Policy
    torch.manual_seed(seed)
    return Policy(W, hidden=H, num_actions=A).to(gpu)


def _crafted_grads(gpu, pol, step, seed=11):
    """N(0, 1) with 5 % exact zeros, and 0, +-1e-30, +-1e4 in every tensor (a one-element tensor takes
    them in turn, one per step)."""
    rng = np.random.default_rng(seed + step)
    out = {}
    for k, p in pol.named_parameters():
        g = rng.standard_normal(tuple(p.shape)).astype(np.float32)
        g[rng.random(g.shape) < 0.05] = 0.0
        flat = g.reshape(-1)
        if flat.size >= 2 * len(SPECIAL):
            flat[rng.choice(flat.size, len(SPECIAL), replace=False)] = SPECIAL
        else:
            flat[(step + np.arange(flat.size)) % flat.size] = [SPECIAL[(step + i) % len(SPECIAL)] for i in
                                                               range(flat.size)]
        out[k] = torch.from_numpy(g).to(gpu)
    return out


def _np(d):
    return {k: d[k].detach().cpu().numpy().copy() for k in PARAMS}


def _weights(pol):
    return {k: v.detach().clone() for k, v in pol.named_parameters()}


def _assert_same(a, b, tag):
    for k in PARAMS:
        x, y = a[k], b[k]
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), \
            f"{tag}: {k} differs at {int((x != y).sum())} of {x.size} elements"


def _crafted_obs(gpu, N, F, seed=5):
    """The four empty-window rows e_q (the table pass), one row per column with exactly that cell lit,
    random dense rows for the rest."""
    assert N >= 4 + F + 16
    rng = np.random.default_rng(seed)
    obs = (rng.random((N, F)) < 0.3).astype(np.uint8)
    obs[:4 + F] = 0
    for q in range(4):
        obs[q, q] = 1
    for c in range(F):
        obs[4 + c, c] = 1
    return torch.from_numpy(obs).to(gpu)


def _act(hp, obs):
    out = hp.act(obs, seed=9)
    torch.cuda.synchronize()
    return [x.clone() for x in out]


class _OwnStream:
    """A HIP stream of the test's own, destroyed at exit (tests/test_gpu_a2c.py::test_graph_capture_matches_eager
    says why it is not one from torch's pool)."""

    def __init__(self, gpu):
        self.gpu, self.hip, self.handle = gpu, ctypes.CDLL("libamdhip64.so"), ctypes.c_void_p()

    def __enter__(self):
        with torch.cuda.device(self.gpu):
            assert self.hip.hipStreamCreate(ctypes.byref(self.handle)) == 0
        return torch.cuda.ExternalStream(self.handle.value, device=self.gpu)

    def __exit__(self, *exc):
        torch.cuda.synchronize(self.gpu)
        assert self.hip.hipStreamDestroy(self.handle) == 0


@pytest.mark.parametrize("W,H,A", CASES + EDGES)
def test_step_bit_equal_restatement_and_repack_equals_load(gpu, W, H, A):
    from gym_ballenv_amd import HipAdam, HipPolicy
    env = _env(gpu, W)
    env.reset()
    pol = _policy(gpu, W, H, A)
    if (W + H) % 2:     # the image the step must fully rewrite: another policy's, or never loaded at all
        hp = HipPolicy(env, _policy(gpu, W, H, A, seed=77), probs=True)
    else:
        hp = HipPolicy(env, hidden=H, num_actions=A, probs=True)
    opt = HipAdam(hp, pol, lr=LR, betas=BETAS, eps=EPS, log_rows=2)
    opt.loss_log.fill_(-7.0)
    losses = torch.tensor([1.5, -2.25, 100.0], dtype=torch.float64, device=gpu)
    w, m, v, state = _np(_weights(pol)), _np(opt.exp_avg), _np(opt.exp_avg_sq), fresh_state(LR)
    obs = _crafted_obs(gpu, env.num_envs, env.obs_dim)
    for step in range(3):
        g = _crafted_grads(gpu, pol, step)
        opt.step(g, losses + step)
        torch.cuda.synchronize(gpu)
        adam_step_ref(w, _np(g), m, v, state, *BETAS, EPS)
        if step in (0, 2):
            _assert_same(_weights(pol), w, f"weights after step {step + 1}")
            _assert_same(opt.exp_avg, m, f"exp_avg after step {step + 1}")
            _assert_same(opt.exp_avg_sq, v, f"exp_avg_sq after step {step + 1}")
            assert opt.state.cpu().numpy().tobytes() == state.tobytes()
            assert not any(np.isnan(w[k]).any() for k in PARAMS)
            # the re-packed image against a fresh load of the module's new weights
            fresh = HipPolicy(env, pol, probs=True)
            for got, want, name in zip(_act(hp, obs), _act(fresh, obs), ("action", "log_prob", "value", "probs")):
                assert torch.equal(got, want), f"{name} after step {step + 1}: re-pack != load"
            fresh.close()
    assert opt.step_count() == 3
    log = opt.loss_log.cpu().numpy()     # rows t % 2 of t = 0, 1, 2: row 0 holds step 2's, row 1 step 1's
    assert np.array_equal(log, (losses.cpu().numpy() + np.array([[2.0], [1.0]])))
    hp.close()
    env.close()


@pytest.mark.parametrize("W,H,A", CASES)
def test_fused_rollout_same_after_step(gpu, W, H, A):
    """8 steps of be_policy_rollout at 512 envs: the stepped policy and a freshly loaded one leave
    the same trajectory and env state."""
    from gym_ballenv_amd import HipAdam, Rollout
    pol = _policy(gpu, W, H, A, seed=1)
    res = []
    for which in ("stepped", "loaded"):
        env = _env(gpu, W, N=512, seed=21)
        env.reset()
        if which == "stepped":
            ro = Rollout(env, pol, horizon=8, backend="fused", seed=4)
            HipAdam(ro.hp, pol, lr=1e-2).step(_crafted_grads(gpu, pol, 0))
        else:
            ro = Rollout(env, pol, horizon=8, backend="fused", seed=4)      # loads the updated module
        ro.run()
        torch.cuda.synchronize(gpu)
        res.append([x.clone() for x in (ro.actions, ro.log_probs, ro.values, ro.rewards, ro.dones, env.obs,
                                        env.agent, env.goal, env.ep_len, env.episode, env.ep_return)])
        ro.close()
        env.close()
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), f"output {i} differs between the stepped and the loaded policy"


def _random_rows(gpu, env, A, rows=320, seed=8):
    rng = np.random.default_rng(seed)
    obs = torch.from_numpy((rng.random((rows, env.obs_dim)) < 0.1).astype(np.uint8)).to(gpu)
    actions = torch.from_numpy(rng.integers(0, A, rows).astype(np.uint8)).to(gpu)
    rn = torch.from_numpy(rng.standard_normal(rows).astype(np.float32)).to(gpu)
    valid = torch.from_numpy((rng.random(rows) < 0.9).astype(np.uint8)).to(gpu)
    return obs, actions, rn, valid


def test_two_optimizers_agree_and_captured_chain_advances(gpu):
    """The chain gradients -> Adam + re-pack, twice: eager on one optimizer, captured once and replayed
    twice on its twin.  The second replay is step 2 (the state advanced on the device, its gradients
    come from the weights step 1 wrote), and everything agrees bit for bit."""
    from gym_ballenv_amd import A2CGrad, HipAdam, HipPolicy
    W, H, A = 10, 208, 9
    env = _env(gpu, W)
    env.reset()
    data = _random_rows(gpu, env, A)
    sides = []
    for _ in range(2):
        pol = _policy(gpu, W, H, A, seed=2)
        hp = HipPolicy(env, pol, probs=True)
        sides.append((pol, hp, A2CGrad(env, pol), HipAdam(hp, pol, lr=1e-2, log_rows=4)))
    (pe, hpe, age, ope), (pc, hpc, agc, opc) = sides
    for _ in range(2):
        ope.step(age(*data), age._losses)
    torch.cuda.synchronize(gpu)
    with _OwnStream(gpu) as s:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            opc.step(agc(*data), agc._losses)
        torch.cuda.synchronize(gpu)
        assert opc.step_count() == 0          # capturing runs nothing
        for i in range(2):
            g.replay()
            torch.cuda.synchronize(gpu)
            assert opc.step_count() == i + 1
        del g
    _assert_same(_weights(pc), _weights(pe), "weights")
    _assert_same(opc.exp_avg, ope.exp_avg, "exp_avg")
    _assert_same(opc.exp_avg_sq, ope.exp_avg_sq, "exp_avg_sq")
    assert torch.equal(opc.state, ope.state) and torch.equal(opc.loss_log, ope.loss_log)
    assert not torch.equal(ope.loss_log[0], ope.loss_log[1]) and (ope.loss_log[2:] == 0).all()
    obs = _crafted_obs(gpu, env.num_envs, env.obs_dim)
    for a, b in zip(_act(hpc, obs), _act(hpe, obs)):
        assert torch.equal(a, b)
    hpe.close()
    hpc.close()
    env.close()


def _torch_adam_f64(w0, grads, lr):
    ps = [torch.nn.Parameter(w0[k].detach().double().cpu().clone()) for k in PARAMS]
    opt = torch.optim.Adam(ps, lr=lr, betas=BETAS, eps=EPS)
    for p, k in zip(ps, PARAMS):
        p.grad = grads[k].detach().double().cpu().clone()
    opt.step()
    return {k: p.detach().numpy() for p, k in zip(ps, PARAMS)}


def test_a2c_update_with_hip_adam(gpu):
    """a2c_update(ro, HipAdam, targets="hip", grads="hip") on the (32, 512, W = 10) rollout of
    test_gpu_a2c_grad.py::test_a2c_update_with_hip_grads, next to the same update with torch.optim.Adam:
    the loss to 1e-4 relative; the weights against f64 torch Adam on the same gradients under the
    host test's rule, err = max|w - w64| / max|w64 - w0| <= 4 err_torch_f32 + 1e-6; the re-packed
    log-probs move.  One update only: after it the two runs' sampled actions may differ."""
    from gym_ballenv_amd import HipAdam, Rollout, a2c_update
    from gym_ballenv_amd.policy import Policy
    runs = {}
    for which in ("torch", "hip"):
        torch.manual_seed(0)
        pol = Policy(10).to(gpu)
        env = _env(gpu, 10, N=512, seed=3)
        env.reset()
        ro = Rollout(env, pol, horizon=32, backend="hip", record_obs=True, seed=2)
        ro.run_eager()
        w0 = _weights(pol)
        lp_old = ro.hp.act(seed=9)[1].clone()
        opt = torch.optim.Adam(pol.parameters(), lr=1e-2, betas=BETAS, eps=EPS) if which == "torch" else \
            HipAdam(ro.hp, pol, lr=1e-2, betas=BETAS, eps=EPS)
        loss = a2c_update(ro, opt, gamma=0.99, targets="hip", grads="hip")
        torch.cuda.synchronize(gpu)
        runs[which] = dict(loss=loss, w0=w0, w=_weights(pol), grads={k: v.clone() for k, v in ro._a2c_grad.grads.items()},
                           moved=not torch.equal(ro.hp.act(seed=9)[1], lp_old), pol=pol)
        if which == "hip":
            assert all(p.grad is None for p in pol.parameters())      # no .grad copies on this path
            assert opt.step_count() == 1
            with pytest.raises(ValueError):                             # bound to another HipPolicy
                other = Rollout(env, pol, horizon=2, backend="hip", record_obs=True)
                try:
                    a2c_update(other, opt, targets="hip", grads="hip")
                finally:
                    other.close()
        ro.close()
        env.close()
    t, h = runs["torch"], runs["hip"]
    assert np.isfinite(h["loss"]) and abs(h["loss"] - t["loss"]) <= 1e-4 * abs(t["loss"]), (h["loss"], t["loss"])
    _assert_same(h["w0"], t["w0"], "initial weights")
    _assert_same(h["grads"], t["grads"], "gradients")
    w64 = _torch_adam_f64(h["w0"], h["grads"], 1e-2)
    for k in PARAMS:
        moved = np.abs(w64[k] - h["w0"][k].double().cpu().numpy()).max()
        err_hip = np.abs(h["w"][k].double().cpu().numpy() - w64[k]).max() / moved
        err_t32 = np.abs(t["w"][k].double().cpu().numpy() - w64[k]).max() / moved
        print(f"{k}: err_hip={err_hip:.3e} err_torch_f32={err_t32:.3e}")
        assert err_hip <= 4 * err_t32 + 1e-6, (k, err_hip, err_t32)
    assert h["moved"] and t["moved"]


@pytest.mark.parametrize("backend,W", [("fused", 10), ("hip", 5)])
@pytest.mark.parametrize("captured", [False, True])
def test_trainer_equals_hand_written_loop(gpu, backend, W, captured):
    """A2CTrainer.train(3) against rollout -> a2c_targets_into -> A2CGrad -> HipAdam.step written out by
    hand, bit for bit; the loss log rows are each iteration's A2CGrad.losses(); a learning-rate change
    between iterations takes effect (under the captured graph too: the hand loop is eager)."""
    from gym_ballenv_amd import A2CGrad, A2CTrainer, HipAdam, Rollout
    from gym_ballenv_amd.policy import Policy
    from gym_ballenv_amd.rollout import A2CTargets, a2c_targets_into
    T, N = 16, 256
    torch.manual_seed(3)
    pol_t = Policy(W).to(gpu)
    pol_h = copy.deepcopy(pol_t)
    env_t, env_h = _env(gpu, W, N=N, seed=5), _env(gpu, W, N=N, seed=5)
    env_t.reset()
    env_h.reset()
    tr = A2CTrainer(env_t, pol_t, horizon=T, gamma=0.99, backend=backend, lr=1e-2, seed=6, log_rows=8)
    ro = Rollout(env_h, pol_h, horizon=T, backend=backend, record_obs=True, seed=6)
    tg = A2CTargets(torch.zeros(T, N, dtype=torch.float32, device=gpu), None,
                    torch.zeros(T, N, dtype=torch.uint8, device=gpu), None)
    ag, opt = A2CGrad(env_h, pol_h), HipAdam(ro.hp, pol_h, lr=1e-2)
    hand_losses = []

    def hand(iterations):
        for _ in range(iterations):
            ro.run() if backend == "fused" else ro.run_eager()
            a2c_targets_into(env_h, ro.rewards, ro.dones, None, 0.99, F32_EPS, None, tg)
            opt.step(ag(ro.obs[:-1], ro.actions, tg.returns_norm, tg.valid), ag._losses)
            hand_losses.append(ag.losses())

    def compare(tag):
        torch.cuda.synchronize(gpu)
        _assert_same(_weights(pol_t), _weights(pol_h), f"{tag}: weights")
        _assert_same(tr.opt.exp_avg, opt.exp_avg, f"{tag}: exp_avg")
        _assert_same(tr.opt.exp_avg_sq, opt.exp_avg_sq, f"{tag}: exp_avg_sq")
        assert torch.equal(tr.opt.state, opt.state), tag
        for a, b in ((tr.rollout.actions, ro.actions), (tr.rollout.rewards, ro.rewards), (env_t.obs, env_h.obs),
                     (env_t.ep_len, env_h.ep_len), (tr.targets.returns_norm, tg.returns_norm)):
            assert torch.equal(a, b), tag
        log = tr.losses().numpy()
        assert log.shape == (len(hand_losses), 3)
        assert np.array_equal(log, np.array(hand_losses, dtype=np.float64)), tag

    hand(3)
    with _OwnStream(gpu) as s:
        if captured:
            tr.capture(stream=s)
        tr.train(3)
        compare("3 iterations")
        assert hand_losses[0] != hand_losses[1] and hand_losses[0][2] > 0
        tr.opt.lr = 2e-3
        opt.lr = 2e-3
        w_before = _weights(pol_t)
        tr.train(1)
        hand(1)
        compare("after the learning-rate change")
        assert tr.opt.state[3].item() == 2e-3 and tr.opt.step_count() == 4
        assert not torch.equal(w_before["fc1.weight"], pol_t.fc1.weight.detach())
        tr.close()
    ro.close()
    env_t.close()
    env_h.close()


def test_state_dict_interchange(gpu):
    """HipAdam -> torch.optim.Adam -> HipAdam, and a HipAdam save / load round trip that continues
    bit for bit."""
    from gym_ballenv_amd import HipAdam, HipPolicy
    W, H, A = 5, 128, 9
    env = _env(gpu, W)
    env.reset()
    pol = _policy(gpu, W, H, A, seed=4)
    hp = HipPolicy(env, pol, probs=True)
    opt = HipAdam(hp, pol, lr=3e-3, betas=(0.8, 0.99), eps=1e-7)
    assert opt.state_dict()["state"] == {}                              # as a fresh torch.optim.Adam
    for step in range(2):
        opt.step(_crafted_grads(gpu, pol, step))
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(6)) and float(sd["state"][0]["step"]) == 2.0
    g2 = _crafted_grads(gpu, pol, 2)

    # the round trip: a second HipAdam on a copy of the module continues exactly as the first
    pol_b = copy.deepcopy(pol)
    hp_b = HipPolicy(env, pol_b, probs=True)
    opt_b = HipAdam(hp_b, pol_b)
    opt_b.load_state_dict(copy.deepcopy(sd))
    assert opt_b.lr == 3e-3 and opt_b.betas == (0.8, 0.99) and opt_b.eps == 1e-7
    assert torch.equal(opt_b.state, opt.state)

    # into torch.optim.Adam: it continues from step 2 with HipAdam's moments
    pol_t = copy.deepcopy(pol)
    opt_t = torch.optim.Adam(pol_t.parameters())
    opt_t.load_state_dict(copy.deepcopy(sd))
    assert opt_t.param_groups[0]["lr"] == 3e-3 and tuple(opt_t.param_groups[0]["betas"]) == (0.8, 0.99)
    for k, p in pol_t.named_parameters():
        p.grad = g2[k].clone()
    w_before = _weights(pol)
    opt_t.step()
    opt.step(g2)
    opt_b.step(g2)
    torch.cuda.synchronize(gpu)
    _assert_same(_weights(pol_b), _weights(pol), "round trip: weights")
    _assert_same(opt_b.exp_avg, opt.exp_avg, "round trip: exp_avg")
    _assert_same(opt_b.exp_avg_sq, opt.exp_avg_sq, "round trip: exp_avg_sq")
    assert torch.equal(opt_b.state, opt.state)
    obs = _crafted_obs(gpu, env.num_envs, env.obs_dim)
    for a, b in zip(_act(hp_b, obs), _act(hp, obs)):
        assert torch.equal(a, b)
    # torch's third step from HipAdam's state lands where HipAdam's does: both round the same step to
    # f32, so at most one f32 ulp of the weight apart, plus the 1e-5 of the step that the two
    # arithmetics differ by (tests/test_a2c_adam_host.py prints that error)
    for k, p in pol_t.named_parameters():
        mine, w0 = dict(pol.named_parameters())[k].detach(), w_before[k]
        bound = 2.0 ** -23 * float(mine.abs().max()) + 1e-5 * float((mine - w0).abs().max())
        assert float((p.detach() - mine).abs().max()) <= bound, k
    assert float(opt_t.state_dict()["state"][0]["step"]) == 3.0

    # and back: torch's state into a HipAdam
    opt_c = HipAdam(hp_b, pol_b)
    opt_c.load_state_dict(opt_t.state_dict())
    assert opt_c.step_count() == 3
    want = fresh_state(3e-3)
    for _ in range(3):
        want[1:3] *= (0.8, 0.99)
    want[0] = 3
    assert opt_c.state.cpu().numpy().tobytes() == want.tobytes()
    tsd = opt_t.state_dict()["state"]
    for i, k in enumerate(PARAMS):
        assert torch.equal(opt_c.exp_avg[k], tsd[i]["exp_avg"]) and torch.equal(opt_c.exp_avg_sq[k], tsd[i]["exp_avg_sq"])
    opt_c.step(g2)
    torch.cuda.synchronize(gpu)
    assert opt_c.step_count() == 4 and all(torch.isfinite(p).all() for p in pol_b.parameters())
    with pytest.raises(ValueError):
        bad = opt_t.state_dict()
        bad["param_groups"][0]["weight_decay"] = 0.1
        opt_c.load_state_dict(bad)
    hp.close()
    hp_b.close()
    env.close()


def test_argument_errors_are_rejected_before_any_launch(gpu):
    import ctypes as C

    from gym_ballenv_amd import HipAdam, HipPolicy, _abi
    W, H, A = 5, 128, 9
    env = _env(gpu, W)
    env.reset()
    pol = _policy(gpu, W, H, A, seed=6)
    hp = HipPolicy(env, pol, probs=True)
    opt = HipAdam(hp, pol, log_rows=2)
    g = _crafted_grads(gpu, pol, 0)
    losses = torch.ones(3, dtype=torch.float64, device=gpu)
    torch.cuda.synchronize(gpu)
    before = (_weights(pol), {k: x.clone() for k, x in opt.exp_avg.items()}, opt.state.clone(), opt.loss_log.clone())
    L = _abi.lib()
    ptrs = lambda d: [d[k].data_ptr() for k in PARAMS]                   # noqa: E731
    good = dict(params=ptrs(_weights_live(pol)), grads=ptrs(g), exp_avg=ptrs(opt.exp_avg),
                exp_avg_sq=ptrs(opt.exp_avg_sq))

    def call(pol_h=hp._h, state=opt.state.data_ptr(), beta1=0.9, beta2=0.999, eps=1e-8, losses_p=None, log_p=None,
             rows=0, null_struct=None, **sets):
        args = []
        for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
            args.append(None if name == null_struct else C.byref(_abi.BeA2CTensors(*sets.get(name, good[name]))))
        return L.be_a2c_adam(pol_h, *args, state, beta1, beta2, eps, losses_p, log_p, rows, env._stream())

    def rejected(msg, **kw):
        assert call(**kw) == _abi.BE_E_INVALID, kw
        err = L.be_last_error(env._ctx).decode()
        assert "be_a2c_adam" in err and msg in err, (err, msg)

    fields = ("fc1_weight", "fc1_bias", "action_head_weight", "action_head_bias", "value_head_weight",
              "value_head_bias")
    for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
        rejected(f"{name} is NULL", null_struct=name)
        for i, f in enumerate(fields):                                   # each NULL pointer, named
            p = list(good[name])
            p[i] = None
            rejected(f"{name}->{f}", **{name: p})
        p = list(good[name])
        p[0] += 2
        rejected(f"{name}->fc1_weight", **{name: p})                     # misaligned
    rejected("state", state=None)
    rejected("state", state=opt.state.data_ptr() + 4)
    rejected("beta1", beta1=1.0)
    rejected("beta2", beta2=-0.1)
    rejected("eps", eps=-1.0)
    rejected("losses and loss_log", losses_p=losses.data_ptr())
    rejected("losses and loss_log", log_p=opt.loss_log.data_ptr(), rows=2)
    rejected("log_rows", losses_p=losses.data_ptr(), log_p=opt.loss_log.data_ptr(), rows=0)

    # the Python surface: ValueError for the wrong dtype, shape, device or contiguity
    from gym_ballenv_amd.policy import Policy
    for bad_pol in (copy.deepcopy(pol).double(), Policy(W, hidden=H - 16).to(gpu), Policy(W, hidden=H, num_actions=4).to(gpu),
                    copy.deepcopy(pol).cpu(), Policy(10).to(gpu)):
        with pytest.raises(ValueError):
            HipAdam(hp, bad_pol)
    other_env = _env(gpu, 10)                                            # a policy from another ctx
    other_hp = HipPolicy(other_env, hidden=H, num_actions=A)
    with pytest.raises(ValueError):
        HipAdam(other_hp, pol)
    for k, bad in (("fc1.weight", g["fc1.weight"].double()), ("fc1.weight", g["fc1.weight"].t().contiguous().t()),
                   ("fc1.bias", g["fc1.bias"][:-1]), ("value_head.bias", g["value_head.bias"].cpu())):
        with pytest.raises(ValueError):
            opt.step({**g, k: bad})
    with pytest.raises(ValueError):
        opt.step()                                                       # no .grad yet
    with pytest.raises(ValueError):
        opt.step(g, losses.float())
    torch.cuda.synchronize(gpu)
    _assert_same(_weights(pol), before[0], "weights after the rejected calls")
    _assert_same(opt.exp_avg, before[1], "exp_avg after the rejected calls")
    assert torch.equal(opt.state, before[2]) and torch.equal(opt.loss_log, before[3])
    # .grad is the default source of the gradients
    for k, p in pol.named_parameters():
        p.grad = g[k].clone()
    opt.step()
    assert opt.step_count() == 1
    opt.zero_grad()
    assert all(p.grad is None for p in pol.parameters())
    other_hp.close()
    other_env.close()
    hp.close()
    env.close()


def _weights_live(pol):
    return {k: v.detach() for k, v in pol.named_parameters()}
