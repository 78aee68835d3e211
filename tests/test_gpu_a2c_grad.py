"""be_a2c_grad on the GPU: against torch f64 autograd under the project's error rule
(tests/test_gpu_policy.py), exact zeros when nothing is active, inactive rows, bit-reproducible,
graph-capturable, the A2CGrad wrapper, a2c_update(grads="hip") and the argument checks."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from a2c_grad_ref import PARAMS, a2c_grad_ref, kink_rows, make_inputs, torch_reference, weights64

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
HIDDEN = {10: 208, 5: 128, 7: 72, 11: 256}


def _env(gpu, W, N=64, seed=3):
    import gym_ballenv_amd as gb
    return gb.BatchedBallEnv(N, W, gb.EnvConfig(), device=gpu, seed=seed)


def _policy(W, fixture=False):
    from gym_ballenv_amd.policy import Policy, reference_weights
    if fixture:
        return Policy.from_npz(reference_weights(W), W)
    torch.manual_seed(0)
    return Policy(W, hidden=HIDDEN[W])


@functools.lru_cache(maxsize=None)
def _case(W, rows, fixture=False):
    """Policy, inputs with the relu-kink rows' valid cleared (at most 1 % of the rows), the f64
    reference (torch f64 autograd on the CPU) and the restatement's loss scales.  Computed once."""
    pol = _policy(W, fixture)
    # seed 1000 + rows: with seed `rows` one of the 63 rows of the (10, 63) case lies on a kink (> 1 %)
    obs, actions, rn, valid = make_inputs(np.random.default_rng(1000 + rows), rows, W)
    kink = kink_rows(weights64(pol), obs)
    assert kink.sum() <= 0.01 * rows, f"{kink.sum()} of {rows} rows on a relu kink"
    valid = np.where(kink, 0, valid).astype(np.uint8)
    g64, l64 = torch_reference(pol, obs, actions, rn, valid, torch.float64)
    ref = a2c_grad_ref(weights64(pol), obs, actions, rn, valid)
    return dict(pol=pol, obs=obs, actions=actions, rn=rn, valid=valid, g64=g64, l64=l64,
                abs_terms=ref["abs_terms"], count=ref["losses"][2])


def _run(gpu, ag, obs, actions, rn, valid):
    """One A2CGrad call on sentinel-filled outputs: ({name: f32 numpy}, losses f64 numpy)."""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    for g in ag.grads.values():
        g.fill_(SENTINEL)
    ag._losses.fill_(SENTINEL)
    ag(t(obs), t(actions), t(rn), t(valid))
    torch.cuda.synchronize(gpu)
    return {k: v.cpu().numpy().copy() for k, v in ag.grads.items()}, ag._losses.cpu().numpy().copy()


def _assert_rule(got, losses, g64, l64, g32, l32, abs_terms, tag):
    """err_hip <= 4 * err_torch32 + 1e-6 per gradient tensor (max-abs error against f64 over the f64
    tensor's max-abs) and per loss (over the f64 sum of the absolute terms)."""
    for k in PARAMS:
        scale = np.abs(g64[k]).max()
        assert scale > 0, (tag, k)
        e_hip = np.abs(got[k].astype(np.float64) - g64[k]).max() / scale
        e_t32 = np.abs(g32[k] - g64[k]).max() / scale
        print(f"{tag} {k}: err_hip {e_hip:.3g} err_torch32 {e_t32:.3g}")
        assert np.isfinite(got[k]).all() and e_hip <= 4 * e_t32 + 1e-6, (tag, k, e_hip, e_t32)
    for i, name in enumerate(("policy_loss", "value_loss")):
        e_hip = abs(losses[i] - l64[i]) / abs_terms[i]
        e_t32 = abs(l32[i] - l64[i]) / abs_terms[i]
        print(f"{tag} {name}: err_hip {e_hip:.3g} err_torch32 {e_t32:.3g}")
        assert e_hip <= 4 * e_t32 + 1e-6, (tag, name, e_hip, e_t32)


CASES = [(10, 1, False), (10, 63, False), (10, 257, False), (10, 11951, False), (10, 11951, True),
         (5, 1, False), (5, 300, False), (5, 11951, False), (7, 1000, False),
         (11, 321, False)]       # the bounds (F = 125, hidden 256): the kernel instance for any shape


@pytest.mark.parametrize("W,rows,fixture", CASES)
def test_against_f64(gpu, W, rows, fixture):
    from gym_ballenv_amd import A2CGrad
    c = _case(W, rows, fixture)
    env = _env(gpu, W)
    pol = copy.deepcopy(c["pol"]).to(gpu)
    ag = A2CGrad(env, pol)
    got, losses = _run(gpu, ag, c["obs"], c["actions"], c["rn"], c["valid"])
    g32, l32 = torch_reference(c["pol"], c["obs"], c["actions"], c["rn"], c["valid"], torch.float32, device=gpu)
    assert losses[2] == c["count"]
    if c["count"] == 0:             # a single row that drew valid = 0: exact zeros
        assert all((g == 0).all() for g in got.values()) and (losses == 0).all()
    else:
        _assert_rule(got, losses, c["g64"], c["l64"], g32, l32, c["abs_terms"], f"W={W} rows={rows}")
    env.close()


def test_nothing_active(gpu):
    from gym_ballenv_amd import A2CGrad
    c = _case(10, 257)
    env = _env(gpu, 10)
    ag = A2CGrad(env, copy.deepcopy(c["pol"]).to(gpu))
    got, losses = _run(gpu, ag, c["obs"], c["actions"], c["rn"], np.zeros(257, np.uint8))
    for k, g in got.items():
        assert (g == 0.0).all(), k
    assert (losses == 0.0).all(), losses
    env.close()


def test_one_active_row_among_257(gpu):
    from gym_ballenv_amd import A2CGrad
    c = _case(10, 257)
    row = int(np.flatnonzero(c["valid"])[-1])
    assert row >= 192
    valid = np.zeros(257, np.uint8)
    valid[row] = 1
    env = _env(gpu, 10)
    ag = A2CGrad(env, copy.deepcopy(c["pol"]).to(gpu))
    got, losses = _run(gpu, ag, c["obs"], c["actions"], c["rn"], valid)
    s = slice(row, row + 1)
    got1, losses1 = _run(gpu, ag, c["obs"][s], c["actions"][s], c["rn"][s], valid[s])
    assert losses.tobytes() == losses1.tobytes() and losses[2] == 1
    for k in PARAMS:
        assert got[k].tobytes() == got1[k].tobytes(), k
    g64, l64 = torch_reference(c["pol"], c["obs"], c["actions"], c["rn"], valid, torch.float64)
    g32, l32 = torch_reference(c["pol"], c["obs"], c["actions"], c["rn"], valid, torch.float32, device=gpu)
    ref = a2c_grad_ref(weights64(c["pol"]), c["obs"], c["actions"], c["rn"], valid)
    _assert_rule(got, losses, g64, l64, g32, l32, ref["abs_terms"], "one row")
    env.close()


def test_out_of_range_action_is_inactive(gpu):
    from gym_ballenv_amd import A2CGrad
    c = _case(10, 257)
    env = _env(gpu, 10)
    ag = A2CGrad(env, copy.deepcopy(c["pol"]).to(gpu))
    rows = np.flatnonzero(c["valid"])[[0, -1]]
    for bad in (9, 255):
        actions = c["actions"].copy()
        actions[rows] = bad
        valid = c["valid"].copy()
        valid[rows] = 0
        a, la = _run(gpu, ag, c["obs"], actions, c["rn"], c["valid"])
        b, lb = _run(gpu, ag, c["obs"], c["actions"], c["rn"], valid)
        assert la.tobytes() == lb.tobytes() and la[2] == c["count"] - 2
        for k in PARAMS:
            assert a[k].tobytes() == b[k].tobytes(), (bad, k)
    env.close()


def test_two_calls_are_bit_identical(gpu):
    from gym_ballenv_amd import A2CGrad
    c = _case(10, 11951)
    env = _env(gpu, 10)
    ag = A2CGrad(env, copy.deepcopy(c["pol"]).to(gpu))
    a, la = _run(gpu, ag, c["obs"], c["actions"], c["rn"], c["valid"])
    ag.workspace.fill_(-1)               # every byte 0xFF
    b, lb = _run(gpu, ag, c["obs"], c["actions"], c["rn"], c["valid"])
    assert la.tobytes() == lb.tobytes()
    for k in PARAMS:
        assert a[k].tobytes() == b[k].tobytes(), k
    env.close()


def test_graph_capture_matches_eager(gpu):
    """Captured on the test's own HIP stream, destroyed at the end, for the reason given in
    tests/test_gpu_a2c.py::test_graph_capture_matches_eager; two replays equal the eager result."""
    from gym_ballenv_amd import A2CGrad
    c = _case(5, 300)
    env = _env(gpu, 5)
    ag = A2CGrad(env, copy.deepcopy(c["pol"]).to(gpu))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    ins = (t(c["obs"]), t(c["actions"]), t(c["rn"]), t(c["valid"]))
    ag(*ins)
    torch.cuda.synchronize(gpu)
    eager = {k: v.clone() for k, v in ag.grads.items()}
    eager_l = ag._losses.clone()
    hip = C.CDLL("libamdhip64.so")
    handle = C.c_void_p()
    with torch.cuda.device(gpu):
        assert hip.hipStreamCreate(C.byref(handle)) == 0
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.ExternalStream(handle.value, device=gpu)):
            ag(*ins)
        for _ in range(2):
            for x in ag.grads.values():
                x.fill_(3)
            ag._losses.fill_(3)
            ag.workspace.fill_(-1)
            g.replay()
            torch.cuda.synchronize(gpu)
            assert torch.equal(ag._losses, eager_l)
            for k in PARAMS:
                assert torch.equal(ag.grads[k], eager[k]), k
        del g
    finally:
        torch.cuda.synchronize(gpu)
        assert hip.hipStreamDestroy(handle) == 0
    env.close()


def test_wrapper_shapes_and_errors(gpu):
    from gym_ballenv_amd import A2CGrad
    c = _case(5, 300)
    env = _env(gpu, 5)
    pol = copy.deepcopy(c["pol"]).to(gpu)
    ag = A2CGrad(env, pol)
    assert list(ag.grads) == list(pol.state_dict())
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    obs, actions, rn, valid = t(c["obs"]), t(c["actions"]), t(c["rn"]), t(c["valid"])

    def bits(*a):
        ag(*a)
        torch.cuda.synchronize(gpu)
        return [v.clone() for v in ag.grads.values()] + [ag._losses.clone()]

    flat = bits(obs, actions, rn, valid)
    T, N = 20, 15
    for other in (bits(obs.reshape(T, N, -1), actions.reshape(T, N), rn.reshape(T, N), valid.reshape(T, N)),
                  bits(obs, actions, rn, valid.bool()),
                  bits(obs.reshape(T, N, -1), actions.reshape(T, N), rn.reshape(T, N), valid.reshape(T, N).bool())):
        assert all(torch.equal(x, y) for x, y in zip(flat, other))
    pl, vl, n = ag.losses()
    assert isinstance(pl, float) and isinstance(vl, float) and isinstance(n, int) and n == c["count"]
    for bad in (dict(obs=obs.float()), dict(obs=obs[:, :-1].contiguous()), dict(obs=obs[:-1]), dict(obs=obs.cpu()),
                dict(obs=obs.reshape(T, N, -1).transpose(0, 1)), dict(actions=actions.long()),
                dict(actions=actions.reshape(T, N)), dict(actions=actions.cpu()), dict(rn=rn.double()),
                dict(rn=rn[:-1]), dict(rn=torch.stack((rn, rn), 1)[:, 0]), dict(valid=valid.float()),
                dict(valid=valid[:-1]), dict(valid=valid.cpu())):
        kw = dict(obs=obs, actions=actions, rn=rn, valid=valid)
        kw.update(bad)
        with pytest.raises(ValueError):
            ag(kw["obs"], kw["actions"], kw["rn"], kw["valid"])
    env10 = _env(gpu, 10)
    with pytest.raises(ValueError):
        A2CGrad(env10, pol)             # a Policy(5) on a W = 10 env
    env10.close()
    env.close()


def test_a2c_update_with_hip_grads(gpu):
    """a2c_update(targets="hip", grads="hip") on a real rollout: the loss agrees with the torch path's,
    the weights move, the HIP policy is re-packed, and the gradients agree with autograd under the
    rule of test_against_f64 once the relu-kink rows' valid is cleared through targets=."""
    from gym_ballenv_amd import A2CGrad, Rollout, a2c_update
    from gym_ballenv_amd.policy import Policy
    from gym_ballenv_amd.rollout import a2c_losses
    SEED = 0        # the first of 0, 1, 2, ... whose rollout keeps the kink share <= 1 %: measured 0 of 16 384 rows
    torch.manual_seed(SEED)
    pol = Policy(10).to(gpu)
    env = _env(gpu, 10, N=512, seed=3)
    env.reset()
    ro = Rollout(env, pol, horizon=32, backend="hip", record_obs=True, seed=2)
    ro.run_eager()
    torch.cuda.synchronize(gpu)
    T, N = 32, 512
    tg = ro.targets(0.99, with_returns=False)
    obs = ro.obs[:-1].reshape(T * N, -1).cpu().numpy()
    actions, rn = ro.actions.reshape(-1).cpu().numpy(), tg.returns_norm.reshape(-1).cpu().numpy()
    pol0 = copy.deepcopy(pol).cpu()
    kink = kink_rows(weights64(pol0), obs)
    print(f"kink share of the seed-{SEED} rollout: {kink.mean():.4%}")
    assert kink.sum() <= 0.01 * T * N
    valid = np.where(kink, 0, tg.valid.reshape(-1).cpu().numpy()).astype(np.uint8)
    assert valid.sum() > 0.5 * T * N
    ag = A2CGrad(env, pol)
    got, losses = _run(gpu, ag, obs, actions, rn, valid)
    g64, l64 = torch_reference(pol0, obs, actions, rn, valid, torch.float64)
    g32, l32 = torch_reference(pol0, obs, actions, rn, valid, torch.float32, device=gpu)
    ref = a2c_grad_ref(weights64(pol0), obs, actions, rn, valid)
    assert losses[2] == ref["losses"][2]
    _assert_rule(got, losses, g64, l64, g32, l32, ref["abs_terms"], "rollout")
    # the update itself
    with torch.no_grad():
        pl, vl = a2c_losses(copy.deepcopy(pol), ro.obs[:-1], ro.actions, ro.rewards, ro.dones, 0.99,
                            targets=(tg.returns_norm, tg.valid))
    want = float(pl + vl)
    w0 = copy.deepcopy(pol.state_dict())
    a_old = ro.hp.act(seed=9)[1].clone()
    opt = torch.optim.Adam(pol.parameters(), lr=1e-2)
    assert all(p.grad is None for p in pol.parameters())
    loss = a2c_update(ro, opt, gamma=0.99, targets="hip", grads="hip")
    assert np.isfinite(loss) and abs(loss - want) <= 1e-4 * abs(want), (loss, want)
    assert all(p.grad is not None for p in pol.parameters())
    assert not torch.equal(w0["fc1.weight"], pol.fc1.weight.detach())
    assert not torch.equal(ro.hp.act(seed=9)[1], a_old)        # re-packed: the log-probs moved
    loss2 = a2c_update(ro, opt, gamma=0.99, targets="torch", grads="hip")      # .grad exists now: copied into
    assert np.isfinite(loss2)
    with pytest.raises(ValueError):
        a2c_update(ro, opt, 0.99, grads="cuda")
    ro.close()
    env.close()


def test_argument_errors(gpu):
    """BE_E_INVALID with a message naming the argument, before any launch."""
    from gym_ballenv_amd import _abi
    env = _env(gpu, 5)
    L, rows, F, H, A = _abi.lib(), 70, 29, 128, 9
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=gpu)
    obs, actions, valid, rn = z(rows, F, dt=torch.uint8), z(rows, dt=torch.uint8), z(rows, dt=torch.uint8), z(rows)
    ws = [z(H, F), z(H), z(A, H), z(A), z(1, H), z(1)]
    gs = [torch.full_like(w, SENTINEL) for w in ws]
    losses = torch.full((3,), SENTINEL, dtype=torch.float64, device=gpu)
    nbytes = L.be_a2c_grad_workspace_bytes(env._ctx, H, A)
    assert nbytes > 0 and nbytes == L.be_a2c_grad_workspace_bytes(env._ctx, H, A)
    work = z((nbytes + 7) // 8, dt=torch.int64)
    P = lambda x: None if x is None else x.data_ptr()

    def call(obs=obs, actions=actions, rn=rn, valid=valid, rows=rows, ws=ws, hidden=H, num_actions=A, gs=gs,
             losses=losses, work=work, work_bytes=nbytes, null_w=False, null_g=False):
        w = _abi.BeA2CWeights(*(P(x) for x in ws), hidden, num_actions)
        g = _abi.BeA2CGrads(*(P(x) for x in gs), P(losses))
        return L.be_a2c_grad(env._ctx, P(obs), P(actions), P(rn), P(valid), rows, None if null_w else C.byref(w),
                             P(work), work_bytes, None if null_g else C.byref(g), env._stream())

    assert call() == _abi.BE_OK
    drop = lambda xs, i: [None if j == i else x for j, x in enumerate(xs)]
    bad = [("obs", dict(obs=None)), ("actions", dict(actions=None)), ("returns_norm", dict(rn=None)),
           ("valid", dict(valid=None)), ("weights", dict(null_w=True)), ("grads", dict(null_g=True)),
           ("rows", dict(rows=-1)), ("hidden", dict(hidden=0)), ("hidden", dict(hidden=257)),
           ("num_actions", dict(num_actions=0)), ("num_actions", dict(num_actions=16)),
           ("workspace", dict(work_bytes=nbytes - 1)), ("workspace", dict(work=None)), ("losses", dict(losses=None))]
    bad += [("weight pointer", dict(ws=drop(ws, i))) for i in range(6)]
    bad += [("gradient pointer", dict(gs=drop(gs, i))) for i in range(6)]
    for word, kw in bad:
        assert call(**kw) == _abi.BE_E_INVALID, (word, kw.keys())
        assert word.encode() in L.be_last_error(env._ctx), (word, L.be_last_error(env._ctx))
    assert L.be_a2c_grad_workspace_bytes(env._ctx, 257, A) == _abi.BE_E_INVALID
    assert L.be_a2c_grad_workspace_bytes(env._ctx, H, 16) == _abi.BE_E_INVALID
    assert call(rows=0) == _abi.BE_OK          # valid: writes zeros
    torch.cuda.synchronize(gpu)
    assert all((g == 0).all() for g in gs) and (losses == 0).all()
    env.close()
