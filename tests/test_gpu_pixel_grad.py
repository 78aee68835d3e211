"""be_cnn_grad on the GPU: the REINFORCE loss and the 14 gradients of the pixel agent against the f64
restatement (tests/cnn_grad_ref.py) under the project's error rule, the probabilities against be_cnn_act bit
for bit, exact zeros for the conv biases, for inactive rows and for clamped rows, bit-reproducibility, graph
capture, the PixelGrad wrapper, PixelRollout's recording, pixel_reinforce_update(grads="hip") and the argument
checks.

The rule, per tensor other than the conv biases: err_hip <= 4 * err_torch32 + 1e-6, both errors the max-abs
distance from the f64 restatement over its max-abs; for the loss the distance over the f64 sum of the rows'
absolute terms.  torch32 is torch autograd in fp32 on the same device.  The conv biases have no gradient in
"sample" mode (the per-map mean subtracts them): the kernel writes exact +0 and the tests ask for that.

Constant images make every feature map constant, and 1 / sqrt(var + 1e-5) = 316 then multiplies rounding
noise: torch fp32 itself is off by per cent on the early layers there.  The tolerance cases therefore leave
the constant images out; one case keeps them and holds the early layers to finiteness only.

The kernel's grid is persistent (one workgroup per CU, each looping over GRAD_TILE-row tiles), so the
multi-round tests size their rows from the device's CU count."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cnn_grad_ref as R
from pixel_policy_cases import given_images, random_policy, trained_policy

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
TILE = 2
LATE = ("conv3.weight", "bn3.weight", "bn3.bias", "head.weight", "head.bias", "loss")


def _env(gpu, N=4, seed=3):
    import gym_ballenv_amd as gb
    return gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=gpu, seed=seed)


def _slots(gpu):
    from gym_ballenv_amd.pixel_policy import GRAD_MAX_SLOTS
    return min(torch.cuda.get_device_properties(gpu).multi_processor_count, GRAD_MAX_SLOTS)


@functools.lru_cache(maxsize=None)
def _policy(key, A=9):
    return trained_policy() if key == "trained" else random_policy(int(key), A)


@functools.lru_cache(maxsize=None)
def _case(key, A, rows, constant=False, mask_band=True):
    """Policy, inputs and the f64 restatement, computed once."""
    pol = _policy(key, A)
    if mask_band:
        ins = R.inputs(pol, rows, 0 if key == "trained" else int(key), constant)
    else:                                   # A = 1: p_a = 1 on every row, all of them clamped
        img, quad = R.drop_constant(*given_images(rows + 4, 0))
        g = torch.Generator().manual_seed(5)
        ins = (img[:rows].contiguous(), quad[:rows].contiguous(), torch.zeros(rows, dtype=torch.uint8),
               torch.randn(rows, generator=g), torch.ones(rows, dtype=torch.uint8))
    return pol, ins, R.restatement(pol, *ins)


def _grad(gpu, env, pol):
    from gym_ballenv_amd import PixelGrad
    return PixelGrad(env, copy.deepcopy(pol).float().to(gpu))


def _dev(gpu, x):
    return None if x is None else x.contiguous().to(gpu)


def _run(gpu, pg, img, quad, act, coef, valid, scale=1.0, probs=None):
    """One PixelGrad call on sentinel-filled outputs: ({name: f32 cpu tensor}, losses f64 cpu tensor)."""
    for g in pg.grads.values():
        g.fill_(SENTINEL)
    pg.losses.fill_(SENTINEL)
    pg(_dev(gpu, img), _dev(gpu, quad), _dev(gpu, act), _dev(gpu, coef), _dev(gpu, valid), scale=scale, probs=probs)
    torch.cuda.synchronize(gpu)
    return {k: v.cpu().clone() for k, v in pg.grads.items()}, pg.losses.cpu().clone()


def _same_bits(a, b, tag):
    (ga, la), (gb, lb) = a, b
    assert la.numpy().tobytes() == lb.numpy().tobytes(), (tag, la, lb)
    for k in ga:
        assert ga[k].numpy().tobytes() == gb[k].numpy().tobytes(), (tag, k, float((ga[k] - gb[k]).abs().max()))


def _zero_biases(got):
    for k in R.CONV_BIASES:
        assert torch.count_nonzero(got[k]) == 0 and not torch.signbit(got[k]).any(), k


def _check(gpu, pg, pol, ins, ref, tag, keys=None, scale=1.0):
    got, losses = _run(gpu, pg, *ins, scale=scale)
    assert all(torch.isfinite(v).all() for v in got.values()) and torch.isfinite(losses).all()
    _zero_biases(got)
    assert int(losses[1]) == ref.count
    t32 = R.torch_reference(pol, *ins, dtype=torch.float32, device=gpu, scale=scale)
    print(tag)
    R.check_rule((got, float(losses[0])), t32, ref, keys=keys, show=print)
    return got, losses


@pytest.mark.parametrize("A", [1, 9, 15])
@pytest.mark.parametrize("rows", sorted({1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1}))
def test_against_f64_row_counts(gpu, rows, A):
    from gym_ballenv_amd.pixel_policy import GRAD_TILE
    assert GRAD_TILE == TILE
    pol, ins, ref = _case("1" if A == 15 else "0", A, rows, False, A > 1)
    env = _env(gpu)
    got, losses = _check(gpu, _grad(gpu, env, pol), pol, ins, ref, f"rows={rows} A={A}")
    if A == 1:          # p_a = 1 > 1 - eps on every row: the clamp passes no gradient
        assert all(torch.count_nonzero(v) == 0 for v in got.values()) and int(losses[1]) == rows
    else:
        assert all(got[k].abs().max() > 0 for k in got if k not in R.CONV_BIASES)
    env.close()


@pytest.mark.parametrize("key", ["0", "trained"])
def test_against_f64_multi_round(gpu, key):
    slots = _slots(gpu)
    rows = TILE * (2 * slots + 5) + 1
    tiles = (rows + TILE - 1) // TILE
    assert tiles // slots >= 2 and rows % TILE != 0            # every workgroup takes >= 2 rounds; the last tile is partial
    pol, ins, ref = _case(key, 9, rows)
    env = _env(gpu)
    _check(gpu, _grad(gpu, env, pol), pol, ins, ref, f"multi-round {key} rows={rows} slots={slots}")
    env.close()


def test_probs_equal_be_cnn_act_bit_for_bit(gpu):
    from gym_ballenv_amd import HipPixelPolicy
    N = 33                                              # the constant images among them; a partial last tile
    img, quad = given_images(N, 0)
    assert sum(len(torch.unique(i)) == 1 for i in img) >= 2
    for key, A in (("0", 9), ("trained", 9), ("1", 15)):
        pol = copy.deepcopy(_policy(key, A)).float().to(gpu)
        env = _env(gpu, N)
        hp = HipPixelPolicy(env, pol, probs=True)
        _, _, want = hp.act(_dev(gpu, img), _dev(gpu, quad))
        pg = _grad(gpu, env, pol)
        probs = torch.full((N, A), SENTINEL, dtype=torch.float32, device=gpu)
        _run(gpu, pg, img, quad, torch.zeros(N, dtype=torch.uint8), None, None, probs=probs)
        assert torch.equal(probs.view(torch.int32), want.view(torch.int32)), (key, (probs - want).abs().max().item())
        hp.close()
        env.close()


def test_constant_images_present(gpu):
    pol, ins, ref = _case("0", 9, 9, True)
    assert sum(len(torch.unique(i)) == 1 for i in ins[0]) == 2          # white and black
    env = _env(gpu)
    # every output finite and the conv biases exact zeros (_check); the late layers under the rule
    _check(gpu, _grad(gpu, env, pol), pol, ins, ref, "constant images", keys=LATE)
    env.close()


def test_nothing_active(gpu):
    pol, ins, _ = _case("0", 9, 7)
    img, quad, act, coef, _ = ins
    env = _env(gpu)
    pg = _grad(gpu, env, pol)
    for actions, valid in ((act, torch.zeros(7, dtype=torch.uint8)), (torch.full((7,), 9, dtype=torch.uint8), None)):
        got, losses = _run(gpu, pg, img, quad, actions, coef, valid)
        assert all(torch.count_nonzero(g) == 0 for g in got.values()) and torch.count_nonzero(losses) == 0
    env.close()


def test_out_of_range_action_is_inactive(gpu):
    pol, ins, ref = _case("0", 9, 7)
    img, quad, act, coef, valid = ins
    rows = torch.nonzero(valid).flatten()[[0, -1]]
    env = _env(gpu)
    pg = _grad(gpu, env, pol)
    for bad in (9, 255):
        a2, v2 = act.clone(), valid.clone()
        a2[rows] = bad
        v2[rows] = 0
        a = _run(gpu, pg, img, quad, a2, coef, valid)
        b = _run(gpu, pg, img, quad, act, coef, v2)
        assert int(a[1][1]) == ref.count - 2
        _same_bits(a, b, bad)
    env.close()


@pytest.mark.parametrize("row", [4, 5])
def test_one_active_row_among_many(gpu, row):
    """Row 4 is a tile's first row, row 5 its second: alone it is the first row of tile 0."""
    slots = _slots(gpu)
    pol, ins, _ = _case("0", 9, 7)
    img, quad, act, coef, _ = ins
    valid = torch.zeros(7, dtype=torch.uint8)
    valid[row] = 1
    env = _env(gpu)
    pg = _grad(gpu, env, pol)
    whole = _run(gpu, pg, img, quad, act, coef, valid)
    s = slice(row, row + 1)
    alone = _run(gpu, pg, img[s], quad[s], act[s], coef[s], valid[s])
    assert int(whole[1][1]) == 1 and all(alone[0][k].abs().max() > 0 for k in alone[0] if k not in R.CONV_BIASES)
    _same_bits(whole, alone, row)
    # and far into the rows of another workgroup's later round
    pol, ins, _ = _case("0", 9, TILE * (2 * slots + 5) + 1)
    img, quad, act, coef, _ = ins
    far = TILE * (slots + 3) + row % TILE
    valid = torch.zeros(img.shape[0], dtype=torch.uint8)
    valid[far] = 1
    s = slice(far, far + 1)
    _same_bits(_run(gpu, pg, img, quad, act, coef, valid), _run(gpu, pg, img[s], quad[s], act[s], coef[s], valid[s]), far)
    env.close()


def test_later_round_alone_is_bit_identical(gpu):
    """Only the tiles of round 1 are active: inactive rows add exact +0, so the result is that of a stand-alone
    call on those rows, whose missing slots would have added +0 in the reduction."""
    slots = _slots(gpu)
    pol, ins, _ = _case("0", 9, TILE * (2 * slots + 5) + 1)
    img, quad, act, coef, valid = ins
    lo, hi = TILE * slots, 2 * TILE * slots
    v = valid.clone()
    v[:lo] = 0
    v[hi:] = 0
    n = int(v.sum())
    assert n > 0.5 * (hi - lo)
    env = _env(gpu)
    pg = _grad(gpu, env, pol)
    whole = _run(gpu, pg, img, quad, act, coef, v)
    s = slice(lo, hi)
    alone = _run(gpu, pg, img[s], quad[s], act[s], coef[s], v[s])
    assert int(whole[1][1]) == n == int(alone[1][1])
    assert all(alone[0][k].abs().max() > 0 for k in alone[0] if k not in R.CONV_BIASES)
    _same_bits(whole, alone, "round 1")
    env.close()


def test_null_coef_and_valid_equal_ones(gpu):
    pol, ins, _ = _case("0", 9, 7)
    img, quad, act, _, _ = ins
    env = _env(gpu)
    pg = _grad(gpu, env, pol)
    ones_f, ones_u = torch.ones(7), torch.ones(7, dtype=torch.uint8)
    full = _run(gpu, pg, img, quad, act, ones_f, ones_u)
    assert int(full[1][1]) == 7
    for coef, valid in ((None, ones_u), (ones_f, None), (None, None)):
        _same_bits(_run(gpu, pg, img, quad, act, coef, valid), full, (coef is None, valid is None))
    env.close()


def test_scale_is_applied_once(gpu):
    """A power of two scales exactly: scale = 0.5 gives exactly half of every scale = 1 output; the count is
    not scaled."""
    pol, ins, _ = _case("0", 9, 7)
    env = _env(gpu)
    pg = _grad(gpu, env, pol)
    one = _run(gpu, pg, *ins)
    half = _run(gpu, pg, *ins, scale=0.5)
    want = ({k: (v.double() * 0.5).float() for k, v in one[0].items()}, torch.stack((one[1][0] * 0.5, one[1][1])))
    _same_bits(half, want, "half")
    env.close()


def test_all_rows_clamped(gpu):
    """Every active row's p_a is above 1 - 1e-9 in f64: the gradients are exactly zero and the loss is
    sum -c log(1 - eps)."""
    from gym_ballenv_amd.pixel_policy import torch_pixel_forward
    pol = copy.deepcopy(_policy("0", 9))
    img, quad = R.drop_constant(*given_images(64, 0))
    keep = torch.zeros(0, dtype=torch.long)
    for _ in range(12):
        with torch.no_grad():
            for p in pol.head.parameters():
                p.mul_(2.0)
            p64 = torch_pixel_forward(copy.deepcopy(pol).double(), img.double() / 255.0,
                                      torch.eye(4, dtype=torch.float64)[quad.long()], "sample")
        keep = torch.nonzero(p64.max(1).values > 1 - 1e-9).flatten()
        if keep.numel() >= 16:
            break
    assert keep.numel() >= 16
    keep = keep[:17]
    img, quad, act = img[keep].contiguous(), quad[keep].contiguous(), p64[keep].argmax(1).to(torch.uint8)
    g = torch.Generator().manual_seed(2)
    coef = torch.randn(keep.numel(), generator=g)
    env = _env(gpu)
    got, losses = _run(gpu, _grad(gpu, env, pol), img, quad, act, coef, None)
    assert all(torch.count_nonzero(v) == 0 for v in got.values())
    want = float((-coef.double() * np.log(1 - R.EPS)).sum())
    scale = float((coef.double().abs() * abs(np.log(1 - R.EPS))).sum())
    print(f"loss {float(losses[0]):.9g} want {want:.9g}")
    assert int(losses[1]) == keep.numel() and abs(float(losses[0]) - want) <= 1e-6 * scale
    env.close()


def test_two_calls_are_bit_identical(gpu):
    slots = _slots(gpu)
    pol, ins, _ = _case("0", 9, TILE * (2 * slots + 5) + 1)
    env = _env(gpu)
    pg = _grad(gpu, env, pol)
    a = _run(gpu, pg, *ins)
    pg.workspace.fill_(-1)               # every byte 0xFF
    b = _run(gpu, pg, *ins)
    assert all(a[0][k].abs().max() > 0 for k in a[0] if k not in R.CONV_BIASES)
    _same_bits(a, b, "0xFF")
    env.close()


def test_graph_capture_matches_eager(gpu):
    """Captured on the test's own HIP stream, destroyed at the end, as tests/test_gpu_mlp_grad.py does; two
    replays equal the eager result."""
    pol, ins, _ = _case("0", 9, 7)
    env = _env(gpu)
    pg = _grad(gpu, env, pol)
    dins = tuple(_dev(gpu, x) for x in ins)
    pg(*dins, scale=0.75)
    torch.cuda.synchronize(gpu)
    eager = {k: v.clone() for k, v in pg.grads.items()}
    eager_l = pg.losses.clone()
    hip = C.CDLL("libamdhip64.so")
    handle = C.c_void_p()
    with torch.cuda.device(gpu):
        assert hip.hipStreamCreate(C.byref(handle)) == 0
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.ExternalStream(handle.value, device=gpu)):
            pg(*dins, scale=0.75)
        for _ in range(2):
            for x in pg.grads.values():
                x.fill_(3)
            pg.losses.fill_(3)
            pg.workspace.fill_(-1)
            g.replay()
            torch.cuda.synchronize(gpu)
            assert torch.equal(pg.losses, eager_l)
            for k in eager:
                assert torch.equal(pg.grads[k], eager[k]), k
        del g
    finally:
        torch.cuda.synchronize(gpu)
        assert hip.hipStreamDestroy(handle) == 0
    env.close()


def test_wrapper_shapes_and_errors(gpu):
    from gym_ballenv_amd import PixelGrad
    from gym_ballenv_amd.pixel_policy import GRAD_MAX_SLOTS, GRAD_TILE, GRAD_WAVES
    assert (GRAD_TILE, GRAD_WAVES, GRAD_MAX_SLOTS) == (2, 8, 1024)
    pol, ins, ref = _case("0", 9, 6, False, True)
    env = _env(gpu)
    dpol = copy.deepcopy(pol).float().to(gpu)
    pg = PixelGrad(env, dpol)
    assert list(pg.grads) == [k for k, _ in dpol.named_parameters()] == list(R.PARAMS)
    assert pg.losses.dtype == torch.float64 and tuple(pg.losses.shape) == (2,)
    img, quad, act, coef, valid = (_dev(gpu, x) for x in ins)

    def bits(*a, **kw):
        out = pg(*a, **kw)
        assert out is pg.grads
        torch.cuda.synchronize(gpu)
        return [v.clone() for v in pg.grads.values()] + [pg.losses.clone()]

    flat = bits(img, quad, act, coef, valid)
    T, N = 3, 2
    for other in (bits(img.reshape(T, N, 3, 40, 40), quad.reshape(T, N), act.reshape(T, N), coef.reshape(T, N),
                       valid.reshape(T, N)), bits(img, quad, act, coef, valid.bool())):
        assert all(torch.equal(x, y) for x, y in zip(flat, other))
    assert int(pg.losses[1]) == ref.count
    pr = torch.zeros(T, N, 9, device=gpu)
    pg(img.reshape(T, N, 3, 40, 40), quad.reshape(T, N), act.reshape(T, N), probs=pr)
    torch.cuda.synchronize(gpu)
    assert (pr.reshape(6, 9).double().cpu() - ref.probs).abs().max().item() < 1e-4
    good = dict(images=img, quadrants=quad, actions=act, coef=coef, valid=valid, probs=None)
    for bad in (dict(images=img.float()), dict(images=img[:, :, :-1].contiguous()), dict(images=img[:-1]),
                dict(images=img.cpu()), dict(images=img.reshape(T, N, 3, 40, 40).transpose(0, 1)),
                dict(quadrants=quad.long()), dict(quadrants=quad[:-1]), dict(quadrants=quad.cpu()),
                dict(actions=act.long()), dict(actions=act.reshape(T, N)), dict(actions=act.cpu()),
                dict(coef=coef.double()), dict(coef=coef[:-1]), dict(coef=torch.stack((coef, coef), 1)[:, 0]),
                dict(valid=valid.float()), dict(valid=valid[:-1]), dict(valid=valid.cpu()),
                dict(probs=torch.zeros(6, 8, device=gpu)), dict(probs=torch.zeros(6, 9)),
                dict(probs=torch.zeros(6, 9, dtype=torch.float64, device=gpu))):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError):
            pg(kw["images"], kw["quadrants"], kw["actions"], kw["coef"], kw["valid"], probs=kw["probs"])
    with pytest.raises(ValueError):
        PixelGrad(env, copy.deepcopy(pol))(img, quad, act)        # the module's weights are on the CPU
    env.close()


def test_argument_errors(gpu):
    """BE_E_INVALID with a message naming the argument, and nothing launched: the sentinels stay."""
    from gym_ballenv_amd import _abi
    env = _env(gpu)
    L, rows, A = _abi.lib(), 5, 9
    pol = copy.deepcopy(_policy("0", 9)).float().to(gpu)
    sd = dict(pol.named_parameters())
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=gpu)
    images, quads, actions = z(rows + 1, 3, 40, 40, dt=torch.uint8), z(rows, dt=torch.uint8), z(rows, dt=torch.uint8)
    gs = {k: torch.full_like(sd[k].detach(), SENTINEL) for k in _abi.CNN_PARAMS}
    losses = torch.full((2,), SENTINEL, dtype=torch.float64, device=gpu)
    nbytes = L.be_cnn_grad_workspace_bytes(env._ctx, A)
    assert nbytes > 0 and nbytes % 16 == 0
    work = z((nbytes + 7) // 8, dt=torch.int64)
    P = lambda x: None if x is None else x.data_ptr()

    def call(images=images.data_ptr(), quads=quads, actions=actions, rows=rows, num_actions=A, work=work.data_ptr(),
             work_bytes=nbytes, losses=losses, drop_w=None, drop_g=None, null_w=False, null_g=False, running=False):
        w = _abi.BeCnnWeights(*(None if k == drop_w or k not in sd else sd[k].data_ptr() for k in _abi.CNN_TENSORS))
        if running:
            w = _abi.BeCnnWeights(*(pol.state_dict()[k].data_ptr() for k in _abi.CNN_TENSORS))
        g = _abi.BeCnnGrads(*(None if k == drop_g else gs[k].data_ptr() for k in _abi.CNN_PARAMS), P(losses), None)
        return L.be_cnn_grad(env._ctx, images, P(quads), P(actions), None, None, rows, 1.0,
                             None if null_w else C.byref(w), num_actions, work, work_bytes,
                             None if null_g else C.byref(g), env._stream())

    bad = [("images is NULL", dict(images=None)), ("images must be 16-byte aligned", dict(images=images.data_ptr() + 8)),
           ("quadrants", dict(quads=None)), ("actions", dict(actions=None)), ("rows", dict(rows=-1)),
           ("num_actions", dict(num_actions=0)), ("num_actions", dict(num_actions=16)), ("weights is NULL", dict(null_w=True)),
           ("grads is NULL", dict(null_g=True)), ("grads->losses", dict(losses=None)),
           ("workspace", dict(work=None)), ("workspace", dict(work=work.data_ptr() + 8)),
           ("workspace is smaller", dict(work_bytes=nbytes - 1))]
    bad += [(f"weights->{k.replace('.', '_')}", dict(drop_w=k)) for k in _abi.CNN_PARAMS]
    bad += [(f"grads->{k.replace('.', '_')}", dict(drop_g=k)) for k in _abi.CNN_PARAMS]
    for word, kw in bad:
        assert call(**kw) == _abi.BE_E_INVALID, (word, kw.keys())
        assert word.encode() in L.be_last_error(env._ctx), (word, L.be_last_error(env._ctx))
    assert L.be_cnn_grad_workspace_bytes(env._ctx, 0) == _abi.BE_E_INVALID
    assert L.be_cnn_grad_workspace_bytes(env._ctx, 16) == _abi.BE_E_INVALID
    assert b"num_actions" in L.be_last_error(env._ctx)
    assert L.be_observe_quadrant(env._ctx, C.byref(env._st), None, env._stream()) == _abi.BE_E_INVALID
    assert b"out" in L.be_last_error(env._ctx)
    torch.cuda.synchronize(gpu)
    assert all((g == SENTINEL).all() for g in gs.values()) and (losses == SENTINEL).all()      # nothing was launched
    assert call(rows=0) == _abi.BE_OK          # valid: writes zeros
    torch.cuda.synchronize(gpu)
    assert all(torch.count_nonzero(g) == 0 for g in gs.values()) and torch.count_nonzero(losses) == 0
    assert call(running=True) == _abi.BE_OK    # the running statistics may be given: they are not read
    torch.cuda.synchronize(gpu)
    env.status()
    env.close()


def test_recorded_rollout(gpu):
    """Recording the images and quadrants changes no step, and the quadrants are observe_blocks' one-hot."""
    from gym_ballenv_amd import PixelRollout
    N, T = 64, 8
    pol = copy.deepcopy(_policy("trained")).float().to(gpu)
    outs = []
    for record in (False, True):
        env = _env(gpu, N, seed=11)
        env.reset()
        ro = PixelRollout(env, pol, T, seed=5, record_images=record)
        if record:
            want_q = []
            for t in range(T):
                want_q.append(env.observe_blocks()[:, :4].argmax(1).to(torch.uint8).clone())
                ro.step(t)
            torch.cuda.synchronize(gpu)
            assert ro.quadrants.dtype == torch.uint8 and tuple(ro.quadrants.shape) == (T, N)
            assert torch.equal(ro.quadrants, torch.stack(want_q))
            assert tuple(ro.images.shape) == (T, N, 3, 40, 40)
        else:
            assert ro.images is None and ro.quadrants is None
            ro.run_eager()
            torch.cuda.synchronize(gpu)
        outs.append([x.clone() for x in (ro.actions, ro.log_probs, ro.rewards, ro.dones)])
        ro.close()
        env.close()
    for a, b in zip(*outs):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_pixel_reinforce_update_with_hip_grads(gpu):
    from gym_ballenv_amd import HipPixelPolicy, PixelRollout, pixel_reinforce_losses, pixel_reinforce_update
    from gym_ballenv_amd.rollout import a2c_targets
    N, T, gamma = 64, 16, 0.99
    pol = copy.deepcopy(_policy("trained")).float().to(gpu)
    env = _env(gpu, N, seed=7)
    env.reset()
    ro = PixelRollout(env, pol, T, seed=3, record_images=True)
    ro.run_eager()
    torch.cuda.synchronize(gpu)
    t = a2c_targets(env, ro.rewards, ro.dones, None, gamma, with_returns=False)
    want_loss = float(pixel_reinforce_losses(pol, ro.images, ro.quadrants, ro.actions, ro.rewards, ro.dones, gamma,
                                             targets=(t.returns_norm, t.valid)).detach())
    flat = (ro.images.reshape(T * N, 3, 40, 40).cpu(), ro.quadrants.reshape(-1).cpu(), ro.actions.reshape(-1).cpu(),
            t.returns_norm.reshape(-1).cpu(), t.valid.reshape(-1).cpu())
    cpu_pol = copy.deepcopy(pol).cpu()
    ref = R.restatement(cpu_pol, *flat)
    pa = ref.probs.gather(1, flat[2].long()[:, None]).squeeze(1)[flat[4] != 0]
    assert not (((pa < 2 * R.EPS) | (pa > 1 - 2 * R.EPS)).any())          # no recorded row in a clamp band
    t32 = R.torch_reference(cpu_pol, *flat, dtype=torch.float32, device=gpu)
    before = {k: v.detach().clone() for k, v in pol.named_parameters()}
    opt = torch.optim.SGD(pol.parameters(), lr=1e-2)
    loss = pixel_reinforce_update(ro, opt, gamma, targets="hip", grads="hip")
    torch.cuda.synchronize(gpu)
    pg = ro._pixel_grad
    got = {k: v.cpu() for k, v in pg.grads.items()}
    _zero_biases(got)
    R.check_rule((got, loss), t32, ref, show=print)
    print(f"loss {loss:.9g} torch {want_loss:.9g}")
    assert abs(loss - want_loss) <= 1e-4 * abs(want_loss) and int(pg.losses[1]) == ref.count
    for k, v in pol.named_parameters():
        assert torch.equal(v.grad, pg.grads[k])
        if k in R.CONV_BIASES:
            assert torch.equal(v.detach(), before[k])
        else:
            assert not torch.equal(v.detach(), before[k]), k
    a, lp, _ = ro.hp.act(seed=9)
    a, lp = a.clone(), lp.clone()
    fresh = HipPixelPolicy(env, pol)
    b, lq, _ = fresh.act(seed=9)
    assert torch.equal(a, b) and torch.equal(lp.view(torch.int32), lq.view(torch.int32))
    fresh.close()
    with pytest.raises(ValueError):
        pixel_reinforce_update(PixelRollout(env, pol, 2), opt)                               # no images
    with pytest.raises(ValueError):
        pixel_reinforce_update(PixelRollout(env, pol, 2, norm="running", record_images=True), opt, grads="hip")
    with pytest.raises(ValueError):
        pixel_reinforce_update(ro, opt, targets="torch", grads="hip")
    ro.close()
    env.close()
