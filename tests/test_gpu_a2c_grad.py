"""be_a2c_grad on the GPU: against torch f64 autograd under the project's error rule
(tests/test_gpu_policy.py), exact zeros when nothing is active, inactive rows, bit-reproducible,
graph-capturable, the A2CGrad wrapper, a2c_update(grads="hip") and the argument checks.

The kernel's grid is persistent (one workgroup per CU, each looping over 64-row tiles), so the
multi-tile tests size their rows from the device's CU count and assert rows > 64 CUs: against f64,
a later round alone against a stand-alone call byte for byte, and observations off the 4-byte grid
(fetch_tile's byte path) against the aligned call byte for byte."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from a2c_grad_ref import (PARAMS, SHAPE_CASES, TILE_EDGE_CASES, a2c_grad_ref, case_inputs, case_policy, kink_rows,
                          make_inputs, multi_tile_cases, torch_reference, weights64)

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def _env(gpu, W, N=64, seed=3):
    import gym_ballenv_amd as gb
    return gb.BatchedBallEnv(N, W, gb.EnvConfig(), device=gpu, seed=seed)


def _slots(gpu):
    """Workgroups of be_a2c_grad's persistent grid on this device: what grad_slots() queries."""
    return min(torch.cuda.get_device_properties(gpu).multi_processor_count, 1024)


def _policy(W, fixture=False, hidden=None, num_actions=9):
    return case_policy(W, hidden, num_actions, fixture)


@functools.lru_cache(maxsize=None)
def _case(W, rows, fixture=False, hidden=None, num_actions=9, force_valid=False):
    """Policy, inputs with the relu-kink rows' valid cleared (at most 1 % of the rows), the f64
    reference (torch f64 autograd on the CPU) and the restatement's loss scales.  Computed once.
    hidden=None: HIDDEN[W].  force_valid: every row's valid is 1 before the kink rows are cleared."""
    pol = _policy(W, fixture, hidden, num_actions)
    # seed 1000 + rows: with seed `rows` one of the 63 rows of the (10, 63) case lies on a kink (> 1 %)
    obs, actions, rn, valid, kink = case_inputs(pol, W, rows, num_actions)
    assert kink.sum() <= 0.01 * rows, f"{kink.sum()} of {rows} rows on a relu kink"
    if force_valid:
        valid = np.ones_like(valid)
    valid = np.where(kink, 0, valid).astype(np.uint8)
    g64, l64 = torch_reference(pol, obs, actions, rn, valid, torch.float64)
    ref = a2c_grad_ref(weights64(pol), obs, actions, rn, valid)
    return dict(pol=pol, obs=obs, actions=actions, rn=rn, valid=valid, g64=g64, l64=l64,
                abs_terms=ref["abs_terms"], count=ref["losses"][2])


def _run(gpu, ag, obs, actions, rn, valid):
    """One A2CGrad call on sentinel-filled outputs: ({name: f32 numpy}, losses f64 numpy)."""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    return _run_t(gpu, ag, t(obs), t(actions), t(rn), t(valid))


def _run_t(gpu, ag, obs, actions, rn, valid):
    """_run on device tensors, passed to A2CGrad as they are."""
    for g in ag.grads.values():
        g.fill_(SENTINEL)
    ag._losses.fill_(SENTINEL)
    ag(obs, actions, rn, valid)
    torch.cuda.synchronize(gpu)
    return {k: v.cpu().numpy().copy() for k, v in ag.grads.items()}, ag._losses.cpu().numpy().copy()


def _same_bytes(a, b, tag):
    (ga, la), (gb, lb) = a, b
    assert la.tobytes() == lb.tobytes(), (tag, la, lb)
    for k in PARAMS:
        assert ga[k].tobytes() == gb[k].tobytes(), (tag, k, float(np.abs(ga[k] - gb[k]).max()))


# With one action log pi = 0 whatever the weights: the f64 action-head gradients and the policy loss
# are identically zero, and the kernel's must be too (its expf(z - lse) - 1 is exact there).
ZERO_AT_A1 = ("action_head.weight", "action_head.bias", "policy_loss")


def _assert_rule(got, losses, g64, l64, g32, l32, abs_terms, tag, zero=()):
    """err_hip <= 4 * err_torch32 + 1e-6 per gradient tensor (max-abs error against f64 over the f64
    tensor's max-abs) and per loss (over the f64 sum of the absolute terms).  The tensors and losses
    named in `zero` have an all-zero f64 reference instead, and the kernel's are all zero."""
    for k in zero:
        if k in PARAMS:
            assert (g64[k] == 0).all() and (got[k] == 0).all(), (tag, k)
        else:
            i = ("policy_loss", "value_loss").index(k)
            assert abs_terms[i] == 0 and l64[i] == 0 and losses[i] == 0, (tag, k, losses[i])
        print(f"{tag} {k}: exact zero")
    for k in PARAMS:
        if k in zero:
            continue
        scale = np.abs(g64[k]).max()
        assert scale > 0, (tag, k)
        e_hip = np.abs(got[k].astype(np.float64) - g64[k]).max() / scale
        e_t32 = np.abs(g32[k] - g64[k]).max() / scale
        print(f"{tag} {k}: err_hip {e_hip:.3g} err_torch32 {e_t32:.3g}")
        assert np.isfinite(got[k]).all() and e_hip <= 4 * e_t32 + 1e-6, (tag, k, e_hip, e_t32)
    for i, name in enumerate(("policy_loss", "value_loss")):
        if name in zero:
            continue
        e_hip = abs(losses[i] - l64[i]) / abs_terms[i]
        e_t32 = abs(l32[i] - l64[i]) / abs_terms[i]
        print(f"{tag} {name}: err_hip {e_hip:.3g} err_torch32 {e_t32:.3g}")
        assert e_hip <= 4 * e_t32 + 1e-6, (tag, name, e_hip, e_t32)


CASES = [(10, 1, False), (10, 63, False), (10, 257, False), (10, 11951, False), (10, 11951, True),
         (5, 1, False), (5, 300, False), (5, 11951, False), (7, 1000, False),
         (11, 321, False)]       # the bounds (F = 125, hidden 256): the kernel instance for any shape


def _check_against_f64(gpu, c, W, tag, zero=()):
    from gym_ballenv_amd import A2CGrad
    env = _env(gpu, W)
    pol = copy.deepcopy(c["pol"]).to(gpu)
    ag = A2CGrad(env, pol)
    got, losses = _run(gpu, ag, c["obs"], c["actions"], c["rn"], c["valid"])
    g32, l32 = torch_reference(c["pol"], c["obs"], c["actions"], c["rn"], c["valid"], torch.float32, device=gpu)
    assert losses[2] == c["count"]
    if c["count"] == 0:             # a single row that drew valid = 0: exact zeros
        assert all((g == 0).all() for g in got.values()) and (losses == 0).all()
    else:
        _assert_rule(got, losses, c["g64"], c["l64"], g32, l32, c["abs_terms"], tag, zero)
    env.close()


@pytest.mark.parametrize("W,rows,fixture", CASES)
def test_against_f64(gpu, W, rows, fixture):
    _check_against_f64(gpu, _case(W, rows, fixture), W, f"W={W} rows={rows}")


@pytest.mark.parametrize("name", list(multi_tile_cases(1)))
def test_against_f64_multi_tile(gpu, name):
    """More than one tile per workgroup, sized from this device's CU count: the prefetch of the next
    tile, its store after step 5, the fetch past the end, the per-row inputs of a later tile and the
    accumulators that live across tiles, under test_against_f64's rule."""
    slots = _slots(gpu)
    W, hidden, A, rows, fixture = multi_tile_cases(slots)[name]
    assert rows > 64 * slots, (rows, slots)
    c = _case(W, rows, fixture, hidden, A)
    assert c["count"] > 0.5 * rows
    _check_against_f64(gpu, c, W, f"multi-tile {name} W={W} hidden={hidden} A={A} rows={rows} slots={slots}")


@pytest.mark.parametrize("W,hidden,A,rows", SHAPE_CASES + TILE_EDGE_CASES)
def test_against_f64_shapes(gpu, W, hidden, A, rows):
    """The padding guards (h < H, j < A, j == A, bz) off the multiples of 8 / 16, every W, both sides
    of each kernel instance's bounds, and rows at a tile's edge."""
    c = _case(W, rows, False, hidden, A)
    assert c["count"] > 0
    _check_against_f64(gpu, c, W, f"W={W} hidden={hidden} A={A} rows={rows}", ZERO_AT_A1 if A == 1 else ())


def test_single_active_row_w5(gpu):
    """(5, 1) of test_against_f64 drew valid = 0; here the row is valid and its action in range."""
    c = _case(5, 1, force_valid=True)
    assert c["count"] == 1 and c["valid"][0] == 1 and c["actions"][0] < 9
    _check_against_f64(gpu, c, 5, "W=5 one active row")


def _rounds(gpu, W, rows, first_tile, slots):
    """make_inputs' rows with valid cleared before tile `first_tile` and from tile first_tile + slots on:
    the whole run against a stand-alone call on the tiles that stay active, byte for byte."""
    from gym_ballenv_amd import A2CGrad
    pol = _policy(W)
    obs, actions, rn, valid = make_inputs(np.random.default_rng(1000 + rows), rows, W)
    lo, hi = 64 * first_tile, min(64 * (first_tile + slots), rows)
    valid = valid.copy()
    valid[:lo] = 0
    valid[hi:] = 0
    n = int(valid.sum())
    assert n > 0.5 * (hi - lo) and (actions < 9).all()
    env = _env(gpu, W)
    ag = A2CGrad(env, copy.deepcopy(pol).to(gpu))
    whole = _run(gpu, ag, obs, actions, rn, valid)
    s = slice(lo, hi)
    alone = _run(gpu, ag, obs[s], actions[s], rn[s], valid[s])
    assert whole[1][2] == n and alone[1][2] == n
    assert all(np.abs(g).max() > 0 for g in alone[0].values())
    _same_bytes(whole, alone, (W, rows, first_tile))
    env.close()


@pytest.mark.parametrize("k", [1, 2])
def test_later_round_alone_is_bit_identical(gpu, k):
    """Only round k's tiles are active (workgroup b's tile b + k slots): inactive rows, with their
    random observations and actions, add exact +0, so the result is the stand-alone call's."""
    slots = _slots(gpu)
    rows = 64 * 3 * slots
    assert rows > 64 * slots
    _rounds(gpu, 10, rows, k * slots, slots)


def test_partial_last_round_alone_is_bit_identical(gpu):
    """Active only in round 3's five whole tiles and its 37-row tile; the stand-alone call launches six
    workgroups, and the slots it lacks would have added +0 in the reduction."""
    slots = _slots(gpu)
    rows = 64 * (2 * slots + 5) + 37
    assert rows > 64 * slots
    _rounds(gpu, 10, rows, 2 * slots, slots)


def _unaligned(gpu, W, rows):
    """obs at byte offset o F of an aligned buffer (fetch_tile's byte path) against the aligned call."""
    from gym_ballenv_amd import A2CGrad
    F = 4 + W * W
    pol = _policy(W)
    obs, actions, rn, valid = make_inputs(np.random.default_rng(1000 + rows), rows, W)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    obs_t, rest = t(obs), (t(actions), t(rn), t(valid))
    assert obs_t.data_ptr() % 4 == 0
    env = _env(gpu, W)
    ag = A2CGrad(env, copy.deepcopy(pol).to(gpu))
    aligned = _run_t(gpu, ag, obs_t, *rest)
    assert aligned[1][2] == int(valid.sum()) and all(np.abs(g).max() > 0 for g in aligned[0].values())
    for o in (1, 2, 3):
        buf = torch.full((rows + o, F), 255, dtype=torch.uint8, device=gpu)
        assert buf.data_ptr() % 4 == 0
        shifted = buf[o:]
        shifted.copy_(obs_t)
        assert shifted.is_contiguous() and shifted.data_ptr() == buf.data_ptr() + o * F
        if (F * o) % 4:
            assert shifted.data_ptr() % 4 != 0
        _same_bytes(_run_t(gpu, ag, shifted, *rest), aligned, (W, rows, o))
    env.close()


@pytest.mark.parametrize("W", [5, 7, 11])
def test_unaligned_obs_is_bit_identical(gpu, W):
    assert (4 + W * W) % 2 == 1          # odd F: every offset o F, o = 1 .. 3, is off the 4-byte grid
    _unaligned(gpu, W, 300)


def test_unaligned_obs_multi_tile(gpu):
    slots = _slots(gpu)
    rows = multi_tile_cases(slots)["w5"][3]
    assert rows > 64 * slots
    _unaligned(gpu, 5, rows)


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
