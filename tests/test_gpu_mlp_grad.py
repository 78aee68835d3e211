"""be_mlp_grad on the GPU: both losses against the f64 restatement (tests/mlp_grad_ref.py) under the
project's error rule, exact zeros when nothing is active or everything is clamped, inactive rows,
bit-reproducible, graph-capturable, the BlockGrad wrapper, reinforce_update(grads="hip"),
supervised_update(grads="hip") and the argument checks.

The rule is tests/test_gpu_a2c_grad.py's, restated: per gradient tensor, err_hip <= 4 * err_torch32 + 1e-6
with both errors the max-abs distance from f64 over the f64 tensor's max-abs; for the loss the
distance from the f64 loss over the f64 sum of the rows' absolute terms.  torch32 is torch autograd
in fp32 on the same device.

REINFORCE's gradient jumps where p_a crosses Categorical's clamp at eps or 1 - eps, so rows whose
*f64* p_a lies in [eps / 2, 2 eps] or [1 - 2 eps, 1 - eps / 2] get valid = 0 in all three evaluations;
at most max(4, rows // 1000) rows may be masked (the cap of tests/test_gpu_block_policy.py).  The
tolerance cases draw the actions from the policy's own probabilities, which keeps p_a off the lower
band; the reference's saturated `reinforce2` weights are used in the bit-for-bit tests only.

The kernel's grid is persistent (one workgroup per CU, each looping over GRAD_TILE-row tiles), so the
multi-tile tests size their rows from the device's CU count and assert rows > GRAD_TILE * CUs."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mlp_grad_ref import (EPS, REINFORCE, XENT, clamp_band, mlp_grad_ref, param_names, sample_actions, torch_reference,
                          weights64)
from test_gpu_block_policy import SHAPES, random_policy, ref_policy

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
LOSSES = (REINFORCE, XENT)
ROW_EDGES = (1, 15, 16, 17, 63, 64, 65)


def _env(gpu, N=64, seed=3):
    import gym_ballenv_amd as gb
    return gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=gpu, seed=seed)


def _slots(gpu):
    """Workgroups of be_mlp_grad's persistent grid on this device."""
    from gym_ballenv_amd.block_policy import GRAD_MAX_SLOTS
    return min(torch.cuda.get_device_properties(gpu).multi_processor_count, GRAD_MAX_SLOTS)


@functools.lru_cache(maxsize=None)
def _fixture():
    from gym_ballenv_amd.block_policy import reference_supervise_data
    d = np.load(reference_supervise_data(), allow_pickle=False)
    return d["blocks"], d["labels"]


def _env_rows(rows, seed):
    """`rows` rows of the reference's recorded trial (env states: counts 0..3), drawn with replacement."""
    blocks = _fixture()[0]
    return blocks[np.random.default_rng(seed).integers(0, blocks.shape[0], rows)]


@functools.lru_cache(maxsize=None)
def _policy(key):
    """"supervised3" / "reinforce2": the reference's trained weights; an index: SHAPES[index] with
    random weights x3 (test_gpu_block_policy.random_policy)."""
    if isinstance(key, str):
        return ref_policy(key)
    layers, h1, h2, A, final_relu, _ = SHAPES[key]
    return random_policy(layers, h1, h2, A, final_relu, seed=1000 * h1 + A)


@functools.lru_cache(maxsize=None)
def _case(key, rows, loss, blocks_from_fixture=False):
    """Policy, env-like rows, actions drawn from the policy's own f64 probabilities, random coefficients,
    90 % valid rows (row 0 always), the clamp-band rows' valid cleared under the cap, and the f64
    reference.  Computed once."""
    pol = _policy(key)
    w = weights64(pol)
    rng = np.random.default_rng(1000 + rows)
    blocks = _fixture()[0][:rows] if blocks_from_fixture else _env_rows(rows, 2000 + rows)
    assert blocks.shape[0] == rows
    probs = mlp_grad_ref(w, blocks, np.zeros(rows, np.uint8), None, None, XENT, pol.final_relu)["probs"]
    actions = sample_actions(probs, rng)
    coef = rng.standard_normal(rows).astype(np.float32)
    valid = (rng.random(rows) < 0.9).astype(np.uint8)
    valid[0] = 1
    masked = 0
    if loss == REINFORCE:
        band = clamp_band(probs[np.arange(rows), actions])
        masked = int(band.sum())
        assert masked <= max(4, rows // 1000), f"{masked} of {rows} rows in the clamp bands"
        valid = np.where(band, 0, valid).astype(np.uint8)
    ref = mlp_grad_ref(w, blocks, actions, coef, valid, loss, pol.final_relu)
    return dict(pol=pol, blocks=blocks, actions=actions, coef=coef, valid=valid, loss=loss, ref=ref, masked=masked)


def _dev(gpu, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _run_t(gpu, bg, blocks, actions, coef, valid, loss, scale=1.0):
    """One BlockGrad call on sentinel-filled outputs: ({name: f32 numpy}, losses f64 numpy)."""
    for g in bg.grads.values():
        g.fill_(SENTINEL)
    bg.losses.fill_(SENTINEL)
    bg(blocks, actions, coef, valid, loss=loss, scale=scale)
    torch.cuda.synchronize(gpu)
    return {k: v.cpu().numpy().copy() for k, v in bg.grads.items()}, bg.losses.cpu().numpy().copy()


def _run(gpu, bg, blocks, actions, coef, valid, loss, scale=1.0):
    return _run_t(gpu, bg, _dev(gpu, blocks), _dev(gpu, actions), _dev(gpu, coef), _dev(gpu, valid), loss, scale)


def _same_bytes(a, b, tag):
    (ga, la), (gb, lb) = a, b
    assert la.tobytes() == lb.tobytes(), (tag, la, lb)
    for k in ga:
        assert ga[k].tobytes() == gb[k].tobytes(), (tag, k, float(np.abs(ga[k] - gb[k]).max()))


def _assert_rule(got, losses, ref, g32, l32, tag):
    """err_hip <= 4 * err_torch32 + 1e-6 per gradient tensor and for the loss.  A tensor (or a loss) whose
    f64 reference is identically zero -- one action, every active row clamped -- is exactly zero."""
    for k, g64 in ref["grads"].items():
        scale = np.abs(g64).max()
        assert np.isfinite(got[k]).all(), (tag, k)
        if scale == 0:
            assert (got[k] == 0).all(), (tag, k)
            print(f"{tag} {k}: exact zero")
            continue
        e_hip = np.abs(got[k].astype(np.float64) - g64).max() / scale
        e_t32 = np.abs(g32[k] - g64).max() / scale
        print(f"{tag} {k}: err_hip {e_hip:.3g} err_torch32 {e_t32:.3g}")
        assert e_hip <= 4 * e_t32 + 1e-6, (tag, k, e_hip, e_t32)
    l64, abs_terms = ref["losses"][0], ref["abs_terms"]
    if abs_terms == 0:
        assert losses[0] == 0, (tag, losses)
        print(f"{tag} loss: exact zero")
    else:
        e_hip, e_t32 = abs(losses[0] - l64) / abs_terms, abs(l32 - l64) / abs_terms
        print(f"{tag} loss: err_hip {e_hip:.3g} err_torch32 {e_t32:.3g}")
        assert e_hip <= 4 * e_t32 + 1e-6, (tag, e_hip, e_t32)


def _check(gpu, bg, c, tag, scale=1.0):
    ref = c["ref"] if scale == 1.0 else mlp_grad_ref(weights64(c["pol"]), c["blocks"], c["actions"], c["coef"],
                                                     c["valid"], c["loss"], c["pol"].final_relu, scale=scale)
    got, losses = _run(gpu, bg, c["blocks"], c["actions"], c["coef"], c["valid"], c["loss"], scale)
    g32, l32 = torch_reference(c["pol"], c["blocks"], c["actions"], c["coef"], c["valid"], c["loss"], torch.float32,
                               scale=scale, device=gpu)
    assert losses[1] == ref["losses"][1], (tag, losses)
    _assert_rule(got, losses, ref, g32, l32, f"{tag} masked={c['masked']}")
    return got, losses


def _grad(gpu, env, key):
    from gym_ballenv_amd import BlockGrad
    return BlockGrad(env, copy.deepcopy(_policy(key)).to(gpu))


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_against_f64_shapes(gpu, shape, loss):
    """Hidden sizes off and on multiples of 16, both ends of the action bound, both layer counts and
    final_relu values; rows on both sides of a wave's 16 rows and of a tile."""
    env = _env(gpu)
    bg = _grad(gpu, env, shape)
    for rows in ROW_EDGES:
        c = _case(shape, rows, loss)
        assert c["ref"]["losses"][1] > 0
        _check(gpu, bg, c, f"{SHAPES[shape][:5]} {loss} rows={rows}")
    env.close()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("key", ["supervised3", 0, 2])
def test_against_f64_recorded_trial(gpu, key, loss):
    """The 3 186 rows of the reference's recorded trial, in order (50 tiles, the last partial), with the
    reference's trained supervised weights and with random weights of both layer counts; scale = 1 / rows."""
    env = _env(gpu)
    c = _case(key, 3186, loss, True)
    assert c["ref"]["losses"][1] > 0.8 * 3186
    _check(gpu, _grad(gpu, env, key), c, f"{key} {loss} trial", scale=1.0 / 3186)
    env.close()


def _multi_rows(gpu):
    from gym_ballenv_amd.block_policy import GRAD_TILE
    slots = _slots(gpu)
    rows = GRAD_TILE * (2 * slots + 5) + 37
    assert rows > GRAD_TILE * slots and rows % GRAD_TILE != 0 and -(-rows // GRAD_TILE) >= 2 * slots
    return slots, rows


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("key", ["supervised3", 2])
def test_against_f64_multi_tile(gpu, key, loss):
    """Every workgroup takes at least two rounds and the last tile is partial: the prefetch of the next
    tile, its store after step 8, the fetch past the end, the per-row inputs of a later tile and the
    accumulators that live across tiles."""
    slots, rows = _multi_rows(gpu)
    c = _case(key, rows, loss)
    assert c["ref"]["losses"][1] > 0.5 * rows
    env = _env(gpu)
    _check(gpu, _grad(gpu, env, key), c, f"multi-tile {key} {loss} rows={rows} slots={slots}")
    env.close()


@pytest.mark.parametrize("key,loss,first,last", [("reinforce2", REINFORCE, 1, 2), ("supervised3", XENT, 1, 2),
                                                 ("supervised3", REINFORCE, 2, 3), ("reinforce2", XENT, 2, 3)])
def test_later_round_alone_is_bit_identical(gpu, key, loss, first, last):
    """Only the tiles of rounds first .. last - 1 are active (round 2: five whole tiles and the 37-row one):
    inactive rows add exact +0, so the result is that of a stand-alone call on those rows, whose missing
    slots would have added +0 in the reduction."""
    from gym_ballenv_amd.block_policy import GRAD_TILE
    slots, rows = _multi_rows(gpu)
    pol = _policy(key)
    rng = np.random.default_rng(rows + first)
    blocks = _env_rows(rows, 77)
    actions = rng.integers(0, pol.num_actions, rows).astype(np.uint8)
    coef = rng.standard_normal(rows).astype(np.float32)
    valid = (rng.random(rows) < 0.9).astype(np.uint8)
    lo, hi = GRAD_TILE * first * slots, min(GRAD_TILE * last * slots, rows)
    valid[:lo] = 0
    valid[hi:] = 0
    n = int(valid.sum())
    assert n > 0.5 * (hi - lo)
    env = _env(gpu)
    bg = _grad(gpu, env, key)
    whole = _run(gpu, bg, blocks, actions, coef, valid, loss)
    s = slice(lo, hi)
    alone = _run(gpu, bg, blocks[s], actions[s], coef[s], valid[s], loss)
    assert whole[1][1] == n and alone[1][1] == n
    assert all(np.abs(g).max() > 0 for g in alone[0].values())
    _same_bytes(whole, alone, (key, loss, first))
    env.close()


def test_nothing_active(gpu):
    env = _env(gpu)
    for key, loss in (("supervised3", REINFORCE), ("reinforce2", XENT)):
        c = _case(key, 257, loss)
        bg = _grad(gpu, env, key)
        for actions, valid in ((c["actions"], np.zeros(257, np.uint8)), (np.full(257, 9, np.uint8), None)):
            got, losses = _run(gpu, bg, c["blocks"], actions, c["coef"], valid, loss)
            assert all((g == 0.0).all() for g in got.values()) and (losses == 0.0).all(), (key, losses)
    env.close()


@pytest.mark.parametrize("loss", LOSSES)
def test_one_active_row_among_257(gpu, loss):
    c = _case("supervised3", 257, loss)
    row = int(np.flatnonzero(c["valid"])[-1])
    assert row >= 192
    valid = np.zeros(257, np.uint8)
    valid[row] = 1
    env = _env(gpu)
    bg = _grad(gpu, env, "supervised3")
    whole = _run(gpu, bg, c["blocks"], c["actions"], c["coef"], valid, loss)
    s = slice(row, row + 1)
    _same_bytes(whole, _run(gpu, bg, c["blocks"][s], c["actions"][s], c["coef"][s], valid[s], loss), loss)
    assert whole[1][1] == 1
    one = dict(c, valid=valid, masked=0,
               ref=mlp_grad_ref(weights64(c["pol"]), c["blocks"], c["actions"], c["coef"], valid, loss, False))
    _check(gpu, bg, one, f"one row {loss}")
    env.close()


def test_out_of_range_action_is_inactive(gpu):
    c = _case("supervised3", 257, REINFORCE)
    env = _env(gpu)
    bg = _grad(gpu, env, "supervised3")
    rows = np.flatnonzero(c["valid"])[[0, -1]]
    for loss in LOSSES:
        for bad in (9, 255):
            actions = c["actions"].copy()
            actions[rows] = bad
            valid = c["valid"].copy()
            valid[rows] = 0
            a = _run(gpu, bg, c["blocks"], actions, c["coef"], c["valid"], loss)
            b = _run(gpu, bg, c["blocks"], c["actions"], c["coef"], valid, loss)
            assert a[1][1] == c["ref"]["losses"][1] - 2
            _same_bytes(a, b, (loss, bad))
    env.close()


def test_null_coef_and_valid_equal_ones(gpu):
    c = _case(0, 300, REINFORCE)
    env = _env(gpu)
    bg = _grad(gpu, env, 0)
    ones_f, ones_u = np.ones(300, np.float32), np.ones(300, np.uint8)
    for loss in LOSSES:
        full = _run(gpu, bg, c["blocks"], c["actions"], ones_f, ones_u, loss)
        assert full[1][1] == 300
        for coef, valid in ((None, ones_u), (ones_f, None), (None, None)):
            _same_bytes(_run(gpu, bg, c["blocks"], c["actions"], coef, valid, loss), full, (loss, coef is None))
    env.close()


def test_scale_is_applied_once(gpu):
    """A power of two scales exactly: scale = 0.5 gives the bits of halving the f64 sums before their one
    rounding, i.e. exactly half of every scale = 1 output (scaling twice would give a quarter); the count
    is not scaled.  scale = 1 / 3 is held to the f64 reference under the rule."""
    env = _env(gpu)
    for loss in LOSSES:
        c = _case("supervised3", 300, loss)
        bg = _grad(gpu, env, "supervised3")
        one = _run(gpu, bg, c["blocks"], c["actions"], c["coef"], c["valid"], loss)
        half = _run(gpu, bg, c["blocks"], c["actions"], c["coef"], c["valid"], loss, scale=0.5)
        want = ({k: (v.astype(np.float64) * 0.5).astype(np.float32) for k, v in one[0].items()},
                np.array([one[1][0] * 0.5, one[1][1]]))
        assert all(np.abs(v).max() > 1e-30 for v in one[0].values())
        _same_bytes(half, want, loss)
        _check(gpu, bg, c, f"scale 1/3 {loss}", scale=1.0 / 3.0)
    env.close()


def test_all_rows_clamped(gpu):
    """Every active row's p_a is past Categorical's clamp -- below 1e-12, or above 1 - 1e-9: the gradients
    are exactly zero and the loss is sum -c log(eps) or sum -c log(1 - eps)."""
    from gym_ballenv_amd import BlockGrad
    from gym_ballenv_amd.block_policy import BlockPolicy
    torch.manual_seed(11)
    pol = BlockPolicy(3, (96, 80), num_actions=9, final_relu=False)
    with torch.no_grad():
        for p in pol.parameters():
            p.mul_(3.0)
        for p in pol.affine3.parameters():
            p.mul_(8.0)
    rng = np.random.default_rng(4)
    blocks = rng.integers(0, 20, (4000, 29)).astype(np.uint8)
    probs = mlp_grad_ref(weights64(pol), blocks, np.zeros(4000, np.uint8), None, None, XENT, False)["probs"]
    keep = np.flatnonzero((probs.max(1) > 1 - 1e-9) & (probs.min(1) < 1e-12))[:150]
    assert keep.size == 150
    blocks, probs = blocks[keep], probs[keep]
    coef = rng.standard_normal(150).astype(np.float32)
    env = _env(gpu)
    bg = BlockGrad(env, copy.deepcopy(pol).to(gpu))
    for actions, bound in ((probs.argmin(1).astype(np.uint8), EPS), (probs.argmax(1).astype(np.uint8), 1 - EPS)):
        got, losses = _run(gpu, bg, blocks, actions, coef, None, REINFORCE)
        assert all((g == 0.0).all() for g in got.values())
        want = float((-coef.astype(np.float64) * np.log(bound)).sum())
        scale = float((np.abs(coef.astype(np.float64)) * abs(np.log(bound))).sum())
        print(f"bound {bound}: loss {losses[0]:.9g} want {want:.9g}")
        assert losses[1] == 150 and abs(losses[0] - want) <= 1e-6 * scale
        got, _ = _run(gpu, bg, blocks, actions, coef, None, XENT)       # no clamp there: the gradient is not zero
        assert np.abs(got["affine3.bias"]).max() > 0 or bound > 0.5
    env.close()


def test_two_calls_are_bit_identical(gpu):
    slots, rows = _multi_rows(gpu)
    env = _env(gpu)
    for key, loss in (("reinforce2", REINFORCE), ("supervised3", XENT)):
        c = _case("supervised3", rows, XENT)
        bg = _grad(gpu, env, key)
        a = _run(gpu, bg, c["blocks"], c["actions"], c["coef"], c["valid"], loss)
        bg.workspace.fill_(-1)               # every byte 0xFF
        b = _run(gpu, bg, c["blocks"], c["actions"], c["coef"], c["valid"], loss)
        assert all(np.abs(g).max() > 0 for g in a[0].values())
        _same_bytes(a, b, key)
    env.close()


def test_graph_capture_matches_eager(gpu):
    """Captured on the test's own HIP stream, destroyed at the end, as tests/test_gpu_a2c_grad.py does;
    two replays equal the eager result."""
    c = _case("supervised3", 300, REINFORCE)
    env = _env(gpu)
    bg = _grad(gpu, env, "supervised3")
    ins = tuple(_dev(gpu, c[k]) for k in ("blocks", "actions", "coef", "valid"))
    bg(*ins, loss=REINFORCE, scale=0.75)
    torch.cuda.synchronize(gpu)
    eager = {k: v.clone() for k, v in bg.grads.items()}
    eager_l = bg.losses.clone()
    hip = C.CDLL("libamdhip64.so")
    handle = C.c_void_p()
    with torch.cuda.device(gpu):
        assert hip.hipStreamCreate(C.byref(handle)) == 0
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.ExternalStream(handle.value, device=gpu)):
            bg(*ins, loss=REINFORCE, scale=0.75)
        for _ in range(2):
            for x in bg.grads.values():
                x.fill_(3)
            bg.losses.fill_(3)
            bg.workspace.fill_(-1)
            g.replay()
            torch.cuda.synchronize(gpu)
            assert torch.equal(bg.losses, eager_l)
            for k in eager:
                assert torch.equal(bg.grads[k], eager[k]), k
        del g
    finally:
        torch.cuda.synchronize(gpu)
        assert hip.hipStreamDestroy(handle) == 0
    env.close()


def test_wrapper_shapes_and_errors(gpu):
    from gym_ballenv_amd import BlockGrad
    from gym_ballenv_amd.block_policy import GRAD_TILE, GRAD_WAVES, TILE, WAVES
    assert (GRAD_TILE, GRAD_WAVES, TILE, WAVES) == (64, 4, 16, 8)
    c = _case("supervised3", 300, REINFORCE)
    env = _env(gpu)
    pol = copy.deepcopy(c["pol"]).to(gpu)
    bg = BlockGrad(env, pol)
    assert list(bg.grads) == list(pol.state_dict()) == param_names(3)
    assert bg.losses.dtype == torch.float64 and tuple(bg.losses.shape) == (2,)
    blocks, actions, coef, valid = (_dev(gpu, c[k]) for k in ("blocks", "actions", "coef", "valid"))

    def bits(*a, **kw):
        out = bg(*a, **kw)
        assert out is bg.grads
        torch.cuda.synchronize(gpu)
        return [v.clone() for v in bg.grads.values()] + [bg.losses.clone()]

    flat = bits(blocks, actions, coef, valid)
    T, N = 20, 15
    for other in (bits(blocks.reshape(T, N, -1), actions.reshape(T, N), coef.reshape(T, N), valid.reshape(T, N)),
                  bits(blocks, actions, coef, valid.bool()), bits(blocks, actions, coef, valid, loss="reinforce")):
        assert all(torch.equal(x, y) for x, y in zip(flat, other))
    # away from the clamp the two losses share dz; the loss value tells them apart
    assert not torch.equal(flat[-1], bits(blocks, actions, coef, valid, loss="xent")[-1])
    assert int(bg.losses[1]) == c["ref"]["losses"][1]
    for bad in (dict(blocks=blocks.float()), dict(blocks=blocks[:, :-1].contiguous()), dict(blocks=blocks[:-1]),
                dict(blocks=blocks.cpu()), dict(blocks=blocks.reshape(T, N, -1).transpose(0, 1)),
                dict(actions=actions.long()), dict(actions=actions.reshape(T, N)), dict(actions=actions.cpu()),
                dict(coef=coef.double()), dict(coef=coef[:-1]), dict(coef=torch.stack((coef, coef), 1)[:, 0]),
                dict(valid=valid.float()), dict(valid=valid[:-1]), dict(valid=valid.cpu()), dict(loss="mse")):
        kw = dict(blocks=blocks, actions=actions, coef=coef, valid=valid, loss="reinforce")
        kw.update(bad)
        with pytest.raises(ValueError):
            bg(kw["blocks"], kw["actions"], kw["coef"], kw["valid"], loss=kw["loss"])
    with pytest.raises(ValueError):
        BlockGrad(env, copy.deepcopy(c["pol"]))(blocks, actions)        # the module's weights are on the CPU
    env.close()


def test_argument_errors(gpu):
    """BE_E_INVALID with a message naming the argument, and nothing launched: the sentinels stay."""
    from gym_ballenv_amd import _abi
    env = _env(gpu)
    L, rows, H, A = _abi.lib(), 70, 128, 9
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=gpu)
    blocks, actions = z(rows, 29, dt=torch.uint8), z(rows, dt=torch.uint8)
    ws = [z(H, 29), z(H), z(H, H), z(H), z(A, H), z(A)]
    gs = [torch.full_like(w, SENTINEL) for w in ws]
    losses = torch.full((2,), SENTINEL, dtype=torch.float64, device=gpu)
    nbytes = L.be_mlp_grad_workspace_bytes(env._ctx, 3, H, H, A)
    assert nbytes > 0 and nbytes % 8 == 0
    assert L.be_mlp_grad_workspace_bytes(env._ctx, 2, H, 0, A) < nbytes
    work = z((nbytes + 7) // 8, dt=torch.int64)
    P = lambda x: None if x is None else x.data_ptr()

    def call(blocks=blocks, actions=actions, rows=rows, loss=0, ws=ws, layers=3, h1=H, h2=H, num_actions=A, gs=gs,
             losses=losses, work=work, work_bytes=nbytes, null_w=False, null_g=False):
        w = _abi.BeMlpWeights(*(P(x) for x in ws), layers, h1, h2, num_actions, 0)
        g = _abi.BeMlpGrads(*(P(x) for x in gs), P(losses))
        return L.be_mlp_grad(env._ctx, P(blocks), P(actions), None, None, rows, loss, 1.0,
                             None if null_w else C.byref(w), P(work), work_bytes, None if null_g else C.byref(g),
                             env._stream())

    drop = lambda xs, *i: [None if j in i else x for j, x in enumerate(xs)]
    bad = [("blocks", dict(blocks=None)), ("actions", dict(actions=None)), ("weights", dict(null_w=True)),
           ("grads", dict(null_g=True)), ("rows", dict(rows=-1)), ("loss", dict(loss=2)), ("loss", dict(loss=-1)),
           ("layers", dict(layers=4)), ("hidden1", dict(h1=0)), ("hidden1", dict(h1=129)), ("hidden2", dict(h2=129)),
           ("hidden2", dict(layers=2)), ("num_actions", dict(num_actions=0)), ("num_actions", dict(num_actions=16)),
           ("workspace", dict(work_bytes=nbytes - 1)), ("workspace", dict(work=None)), ("losses", dict(losses=None)),
           ("w3", dict(ws=drop(ws, 4))), ("w3", dict(ws=drop(ws, 5))), ("w3", dict(gs=drop(gs, 4))),
           ("w3", dict(gs=drop(gs, 5))), ("w3", dict(layers=2, h2=0)), ("w3", dict(layers=2, h2=0, ws=drop(ws, 4, 5)))]
    bad += [("weight pointer", dict(ws=drop(ws, i))) for i in range(4)]
    bad += [("gradient pointer", dict(gs=drop(gs, i))) for i in range(4)]
    for word, kw in bad:
        assert call(**kw) == _abi.BE_E_INVALID, (word, kw.keys())
        assert word.encode() in L.be_last_error(env._ctx), (word, L.be_last_error(env._ctx))
    assert L.be_mlp_grad_workspace_bytes(env._ctx, 3, 129, H, A) == _abi.BE_E_INVALID
    assert L.be_mlp_grad_workspace_bytes(env._ctx, 3, H, H, 16) == _abi.BE_E_INVALID
    assert L.be_mlp_grad_workspace_bytes(env._ctx, 2, H, H, A) == _abi.BE_E_INVALID
    torch.cuda.synchronize(gpu)
    assert all((g == SENTINEL).all() for g in gs) and (losses == SENTINEL).all()      # nothing was launched
    assert call(rows=0) == _abi.BE_OK          # valid: writes zeros
    torch.cuda.synchronize(gpu)
    assert all((g == 0).all() for g in gs) and (losses == 0).all()
    assert call(layers=2, h2=0, ws=drop(ws, 4, 5)[:2] + [ws[4], ws[5], None, None],
                gs=gs[:2] + [gs[4], gs[5], None, None]) == _abi.BE_OK
    torch.cuda.synchronize(gpu)
    env.status()
    env.close()


def test_reinforce_update_with_hip_grads(gpu):
    """captured BlockRollout -> reinforce_update(grads="hip"), three times.  On the first record the
    gradients agree with autograd (grads="torch") under the rule, the loss with reinforce_losses' to 1e-4;
    the weights move and the rollout's kernel then acts with them."""
    from gym_ballenv_amd import BlockGrad, BlockRollout, HipBlockPolicy, a2c_targets, reinforce_losses, reinforce_update
    pol = ref_policy("supervised3").to(gpu)
    w0 = copy.deepcopy(pol.state_dict())
    env = _env(gpu, N=512)
    env.reset()
    T, N = 32, 512
    ro = BlockRollout(env, pol, horizon=T, record_obs=True, seed=2)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-2)
    ro.capture(chunk=T)
    ro.run()
    torch.cuda.synchronize(gpu)
    tg = a2c_targets(env, ro.rewards, ro.dones, None, 0.99, with_returns=False)
    pol0 = copy.deepcopy(pol).cpu()
    blocks, actions = ro.blocks.reshape(T * N, 29).cpu().numpy(), ro.actions.reshape(-1).cpu().numpy()
    coef, valid = tg.returns_norm.reshape(-1).cpu().numpy(), tg.valid.reshape(-1).cpu().numpy()
    w = weights64(pol0)
    band = clamp_band(mlp_grad_ref(w, blocks, actions, coef, valid, REINFORCE, False)["pa"]) & (valid != 0)
    print(f"{int(band.sum())} of {T * N} recorded rows in the clamp bands")
    assert band.sum() <= max(4, T * N // 1000)
    masked = np.where(band, 0, valid).astype(np.uint8)
    assert masked.sum() > 0.5 * T * N
    c = dict(pol=pol0, blocks=blocks, actions=actions, coef=coef, valid=masked, loss=REINFORCE, masked=int(band.sum()),
             ref=mlp_grad_ref(w, blocks, actions, coef, masked, REINFORCE, False))
    _check(gpu, BlockGrad(env, pol), c, "rollout")
    with torch.no_grad():
        want = float(reinforce_losses(copy.deepcopy(pol), ro.blocks, ro.actions, ro.rewards, ro.dones, 0.99,
                                      targets=(tg.returns_norm, tg.valid)))
    assert all(p.grad is None for p in pol.parameters())
    loss = reinforce_update(ro, opt, gamma=0.99, targets="hip", grads="hip")
    print(f"loss {loss:.9g} torch {want:.9g}")
    assert np.isfinite(loss) and abs(loss - want) <= 1e-4 * abs(want), (loss, want)
    assert all(p.grad is not None for p in pol.parameters())
    for it in range(2):
        ro.run()
        assert np.isfinite(reinforce_update(ro, opt, gamma=0.99, grads="hip"))
    for k, v in pol.state_dict().items():
        assert not torch.equal(w0[k], v), k
    hp2 = HipBlockPolicy(env, pol)
    assert torch.equal(ro.hp.act(seed=9)[0], hp2.act(seed=9)[0])        # the rollout's kernel was re-packed
    with pytest.raises(ValueError):
        reinforce_update(ro, opt, 0.99, targets="torch", grads="hip")
    with pytest.raises(ValueError):
        reinforce_update(ro, opt, 0.99, grads="cuda")
    hp2.close(); ro.close(); env.close()


def test_supervised_update_with_hip_grads(gpu):
    """examples/train_supervise.py's loop on the reference's own data: the first minibatch of 200 and the
    last of 186 (a partial tile) under the rule, then one epoch lowers the full-data cross-entropy."""
    from gym_ballenv_amd import BlockGrad, BlockPolicy, supervised_losses, supervised_update
    blocks, labels = _fixture()
    torch.manual_seed(0)
    pol = BlockPolicy(3, 128, 9, final_relu=False).to(gpu)
    env = _env(gpu)
    bg = BlockGrad(env, pol)
    pol0 = copy.deepcopy(pol).cpu()
    for s in (slice(0, 200), slice(3000, 3186)):
        n = s.stop - s.start
        ref = mlp_grad_ref(weights64(pol0), blocks[s], labels[s], None, None, XENT, False, scale=1.0 / n)
        got, losses = _run(gpu, bg, blocks[s], labels[s], None, None, XENT, scale=1.0 / n)
        g32, l32 = torch_reference(pol0, blocks[s], labels[s], None, None, XENT, torch.float32, scale=1.0 / n, device=gpu)
        assert losses[1] == n
        _assert_rule(got, losses, ref, g32, l32, f"minibatch of {n}")
        with torch.no_grad():
            mean = float(supervised_losses(pol, _dev(gpu, blocks[s]), _dev(gpu, labels[s])))
        assert abs(losses[0] - mean) <= 1e-5 * abs(mean)
    bt, lt = _dev(gpu, blocks), _dev(gpu, labels)
    opt = torch.optim.SGD(pol.parameters(), lr=1e-2)
    with torch.no_grad():
        before = float(supervised_losses(pol, bt, lt))
    for i in range(0, 3186, 200):
        j = i + 200 if i + 200 < 3186 else 3186
        assert np.isfinite(supervised_update(pol, bt[i:j], lt[i:j], opt, grads="hip", grad=bg))
    with torch.no_grad():
        after = float(supervised_losses(pol, bt, lt))
    print(f"full-data cross-entropy {before:.4f} -> {after:.4f}")
    assert after < before
    env.close()
