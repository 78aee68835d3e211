"""be_mlp_opt on the GPU: bit-equal to the numpy restatements (tests/a2c_adam_ref.py's Adam,
tests/mlp_opt_ref.py's SGD), its re-packed image equal to a fresh HipBlockPolicy.load of the new weights,
the state advancing on the device and graph-capturable, interchangeable with torch.optim's state_dicts,
a drop-in optimizer for reinforce_update / supervised_update, and the engine of BlockTrainer and
SupervisedTrainer."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from a2c_adam_ref import adam_step_ref, fresh_state
from a2c_ref import EPS as F32_EPS
from mlp_opt_ref import names, sgd_step_ref
from test_gpu_a2c_adam import _OwnStream, _crafted_grads
from test_gpu_block_policy import SHAPES, make, random_policy, random_rows, ref_policy

pytestmark = pytest.mark.gpu

BETAS, EPS, LR = (0.9, 0.999), 1e-8, 1e-2
KINDS = ("adam", "sgd")


def _np(d):
    return {k: d[k].detach().cpu().numpy().copy() for k in d}


def _weights(pol):
    return {k: v.detach().clone() for k, v in pol.named_parameters()}


def _same(a, b, tag):
    assert list(a) == list(b), tag
    for k in a:
        x, y = a[k], b[k]
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), \
            f"{tag}: {k} differs at {int((x != y).sum())} of {x.size} elements"


def _ref_step(kind, w, g, m, v, state):
    if kind == "adam":
        adam_step_ref(w, g, m, v, state, *BETAS, EPS)
    else:
        sgd_step_ref(w, g, state)


def _moments(opt, kind):
    if kind == "adam":
        return _np(opt.exp_avg), _np(opt.exp_avg_sq)
    return None, None


def _never_loaded(hp):
    """Replace the HipBlockPolicy's handle with one straight from be_mlp_create: an image no be_mlp_load
    has written."""
    from gym_ballenv_amd import _abi
    torch.cuda.synchronize()
    _abi.check(hp._lib.be_mlp_destroy(hp._h))
    h = C.c_void_p()
    _abi.check(hp._lib.be_mlp_create(hp.env._ctx, hp.layers, hp.hidden1, hp.hidden2, hp.num_actions,
                                     int(hp.final_relu), C.byref(h)), hp.env._ctx)
    hp._h = h


def _act(hp, rows):
    out = hp.act(rows, seed=9)
    torch.cuda.synchronize()
    return [x.clone() for x in out if x is not None]


@functools.lru_cache(maxsize=None)
def _fixture():
    from gym_ballenv_amd.block_policy import reference_supervise_data
    d = np.load(reference_supervise_data(), allow_pickle=False)
    return d["blocks"], d["labels"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_step_bit_equal_restatement_and_repack_equals_load(gpu, kind, case):
    from gym_ballenv_amd import HipBlockOptim, HipBlockPolicy
    layers, h1, h2, A, final_relu, _ = SHAPES[case]
    N = 64
    env = make(gpu, N)
    pol = random_policy(layers, h1, h2, A, final_relu, seed=case).to(gpu)
    # the image the step must complete: another policy's weights, or never loaded at all
    hp = HipBlockPolicy(env, random_policy(layers, h1, h2, A, final_relu, seed=77).to(gpu), probs=True)
    if (case + KINDS.index(kind)) % 2:
        _never_loaded(hp)
    opt = HipBlockOptim(hp, pol, kind, lr=LR, betas=BETAS, eps=EPS, log_rows=2)
    opt.loss_log.fill_(-7.0)
    losses = torch.tensor([1.5, 100.0], dtype=torch.float64, device=gpu)
    w, state = _np(_weights(pol)), fresh_state(LR)
    assert list(w) == names(layers)
    m, v = _moments(opt, kind)
    rows = random_rows(N, seed=case).to(gpu)
    for step in range(3):
        g = _crafted_grads(gpu, pol, step)
        opt.step(g, losses + step)
        torch.cuda.synchronize(gpu)
        _ref_step(kind, w, _np(g), m, v, state)
        _same(_weights(pol), w, f"weights after step {step + 1}")
        if kind == "adam":
            _same(opt.exp_avg, m, f"exp_avg after step {step + 1}")
            _same(opt.exp_avg_sq, v, f"exp_avg_sq after step {step + 1}")
        assert opt.state.cpu().numpy().tobytes() == state.tobytes()
        assert not any(np.isnan(w[k]).any() for k in w)
        fresh = HipBlockPolicy(env, pol, probs=True)
        for got, want, name in zip(_act(hp, rows), _act(fresh, rows), ("action", "log_prob", "probs")):
            assert torch.equal(got, want), f"{name} after step {step + 1}: re-pack != load"
        fresh.close()
    assert opt.step_count() == 3
    log = opt.loss_log.cpu().numpy()     # rows t % 2 of t = 0, 1, 2: row 0 holds step 2's, row 1 step 1's
    assert np.array_equal(log, (losses.cpu().numpy() + np.array([[2.0], [1.0]])))
    hp.close()
    env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_state_and_learning_rate(gpu, kind):
    """opt.lr = x is stream-ordered: the step enqueued before it keeps the old rate, the next one takes
    the new; the step count advances by one per call."""
    from gym_ballenv_amd import HipBlockOptim, HipBlockPolicy
    layers, h1, h2, A, final_relu, _ = SHAPES[1]
    env = make(gpu, 64)
    pol = random_policy(layers, h1, h2, A, final_relu, seed=5).to(gpu)
    hp = HipBlockPolicy(env, pol)
    opt = HipBlockOptim(hp, pol, kind, lr=LR, betas=BETAS, eps=EPS)
    w, state = _np(_weights(pol)), fresh_state(LR)
    m, v = _moments(opt, kind)
    gs = [_crafted_grads(gpu, pol, s) for s in range(3)]
    torch.cuda.synchronize(gpu)
    assert opt.step_count() == 0
    opt.step(gs[0])
    opt.lr = 2.5e-3                       # no synchronise in between
    opt.step(gs[1])
    torch.cuda.synchronize(gpu)
    assert opt.lr == 2.5e-3 and opt.step_count() == 2
    _ref_step(kind, w, _np(gs[0]), m, v, state)
    state[3] = 2.5e-3
    _ref_step(kind, w, _np(gs[1]), m, v, state)
    _same(_weights(pol), w, "weights after the learning-rate change")
    assert opt.state.cpu().numpy().tobytes() == state.tobytes()
    opt.step(gs[2])
    assert opt.step_count() == 3
    _ref_step(kind, w, _np(gs[2]), m, v, state)
    _same(_weights(pol), w, "weights after step 3")
    hp.close()
    env.close()


def _random_batch(gpu, A, rows=320, seed=8):
    rng = np.random.default_rng(seed)
    blocks = torch.from_numpy(rng.integers(0, 4, (rows, 29)).astype(np.uint8)).to(gpu)
    actions = torch.from_numpy(rng.integers(0, A, rows).astype(np.uint8)).to(gpu)
    coef = torch.from_numpy(rng.standard_normal(rows).astype(np.float32)).to(gpu)
    valid = torch.from_numpy((rng.random(rows) < 0.9).astype(np.uint8)).to(gpu)
    return blocks, actions, coef, valid


@pytest.mark.parametrize("kind", KINDS)
def test_captured_chain_equals_eager(gpu, kind):
    """BlockGrad + step, captured once on a stream of the test's own and replayed: 3 replays equal 3 eager
    iterations bit for bit (each replay's gradients come from the weights the one before wrote); after 5
    steps the 2-row ring holds step 3's losses in row 1 and step 4's in row 0."""
    from gym_ballenv_amd import BlockGrad, BlockPolicy, HipBlockOptim, HipBlockPolicy
    env = make(gpu, 64)
    data = _random_batch(gpu, 9)
    sides = []
    for _ in range(2):
        torch.manual_seed(3)             # torch's initialisation and the cross-entropy: the softmax does not
        pol = BlockPolicy(3, 128, final_relu=False).to(gpu)      # saturate, so every step moves the loss
        hp = HipBlockPolicy(env, pol, probs=True)
        sides.append((pol, hp, BlockGrad(env, pol), HipBlockOptim(hp, pol, kind, lr=LR, log_rows=2)))
    (pe, hpe, bge, ope), (pc, hpc, bgc, opc) = sides
    seen = []

    def eager(n):
        for _ in range(n):
            ope.step(bge(*data, "xent", 1.0 / 320), bge.losses)
            torch.cuda.synchronize(gpu)
            seen.append(bge.losses.clone())

    def compare(tag):
        _same(_weights(pc), _weights(pe), f"{tag}: weights")
        if kind == "adam":
            _same(opc.exp_avg, ope.exp_avg, f"{tag}: exp_avg")
            _same(opc.exp_avg_sq, ope.exp_avg_sq, f"{tag}: exp_avg_sq")
        assert torch.equal(opc.state, ope.state) and torch.equal(opc.loss_log, ope.loss_log), tag

    eager(3)
    with _OwnStream(gpu) as s:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            opc.step(bgc(*data, "xent", 1.0 / 320), bgc.losses)
        torch.cuda.synchronize(gpu)
        assert opc.step_count() == 0          # capturing runs nothing
        for i in range(3):
            g.replay()
            torch.cuda.synchronize(gpu)
            assert opc.step_count() == i + 1
        compare("3 steps")
        eager(2)
        for i in range(2):
            g.replay()
        torch.cuda.synchronize(gpu)
        compare("5 steps")
        del g
    assert opc.step_count() == 5
    assert torch.equal(opc.loss_log[1], seen[3]) and torch.equal(opc.loss_log[0], seen[4])
    assert not torch.equal(seen[3], seen[4]) and seen[4][1] > 0
    rows = random_rows(64, seed=1).to(gpu)
    for a, b in zip(_act(hpc, rows), _act(hpe, rows)):
        assert torch.equal(a, b)
    hpe.close()
    hpc.close()
    env.close()


def test_argument_errors_are_rejected_before_any_launch(gpu):
    from gym_ballenv_amd import BlockPolicy, HipBlockOptim, HipBlockPolicy, _abi
    env = make(gpu, 64)
    SENT = 123.25
    hps, good, pols, opts = {}, {}, {}, {}
    for layers in (3, 2):
        pol = random_policy(layers, 32, 32 if layers == 3 else 0, 9, True, seed=6).to(gpu)
        with torch.no_grad():
            for p in pol.parameters():
                p.fill_(SENT)
        hp = HipBlockPolicy(env, pol)
        opt = HipBlockOptim(hp, pol, "adam", log_rows=2)
        g = _crafted_grads(gpu, pol, 0)
        ptrs = lambda d: [d[k].data_ptr() for k in names(layers)] + [None] * (6 - 2 * layers)    # noqa: E731
        good[layers] = dict(params=ptrs(dict(pol.named_parameters())), grads=ptrs(g), exp_avg=ptrs(opt.exp_avg),
                            exp_avg_sq=ptrs(opt.exp_avg_sq), keep=g)
        hps[layers], pols[layers], opts[layers] = hp, pol, opt
    opt = opts[3]
    losses = torch.ones(2, dtype=torch.float64, device=gpu)
    torch.cuda.synchronize(gpu)
    before = (opt.state.clone(), opt.loss_log.clone(), {k: x.clone() for k, x in opt.exp_avg.items()})
    L = _abi.lib()
    ADAM, SGD = _abi.MLP_OPT_ADAM, _abi.MLP_OPT_SGD

    def call(layers=3, kind=ADAM, state=opt.state.data_ptr(), beta1=0.9, beta2=0.999, eps=1e-8, losses_p=None,
             log_p=None, rows=0, null_struct=(), **sets):
        args = []
        for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
            args.append(None if name in null_struct else C.byref(_abi.BeMlpTensors(*sets.get(name, good[layers][name]))))
        return L.be_mlp_opt(hps[layers]._h, kind, *args, state, beta1, beta2, eps, losses_p, log_p, rows, env._stream())

    def rejected(msg, **kw):
        assert call(**kw) == _abi.BE_E_INVALID, kw
        err = L.be_last_error(env._ctx).decode()
        assert "be_mlp_opt" in err and msg in err, (err, msg)

    sgd = dict(kind=SGD, null_struct=("exp_avg", "exp_avg_sq"))
    rejected("kind", kind=2)
    rejected("kind", kind=-1)
    fields = ("w1", "b1", "w2", "b2", "w3", "b3")
    for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
        rejected(f"{name} is NULL", null_struct=(name,))
        for layers in (3, 2):
            for i, f in enumerate(fields[:2 * layers]):                  # each NULL pointer, named
                p = list(good[layers][name])
                p[i] = None
                rejected(f"{name}->{f}", layers=layers, **{name: p})
        p = list(good[3][name])
        p[2] += 2
        rejected(f"{name}->w2", **{name: p})                             # misaligned
        for i in (4, 5):                                                 # w3 / b3 given to a 2-layer network
            p = list(good[2][name])
            p[i] = good[3][name][i]
            rejected(f"{name}->{fields[i]}", layers=2, **{name: p})
    for name in ("params", "grads"):                                     # the same under SGD
        rejected(f"{name} is NULL", kind=SGD, null_struct=(name, "exp_avg", "exp_avg_sq"))
        p = list(good[3][name])
        p[5] = None
        rejected(f"{name}->b3", **sgd, **{name: p})
    rejected("exp_avg", kind=SGD)                                        # moment sets given to SGD
    rejected("exp_avg", kind=SGD, null_struct=("exp_avg",))
    rejected("exp_avg", kind=SGD, null_struct=("exp_avg_sq",))
    rejected("state", state=None)
    rejected("state", state=opt.state.data_ptr() + 4)
    rejected("state", state=None, **sgd)
    rejected("beta1", beta1=1.0)
    rejected("beta2", beta2=-0.1)
    rejected("eps", eps=-1.0)
    rejected("losses and loss_log", losses_p=losses.data_ptr())
    rejected("losses and loss_log", log_p=opt.loss_log.data_ptr(), rows=2)
    rejected("not 8-byte aligned", losses_p=losses.data_ptr() + 4, log_p=opt.loss_log.data_ptr(), rows=2)
    rejected("not 8-byte aligned", losses_p=losses.data_ptr(), log_p=opt.loss_log.data_ptr() + 4, rows=2)
    rejected("log_rows", losses_p=losses.data_ptr(), log_p=opt.loss_log.data_ptr(), rows=0)
    rejected("log_rows", losses_p=losses.data_ptr(), log_p=opt.loss_log.data_ptr(), rows=0, **sgd)
    assert L.be_mlp_opt(None, ADAM, None, None, None, None, None, 0.9, 0.999, 1e-8, None, None, 0, None) == \
        _abi.BE_E_INVALID
    assert b"mlp is NULL" in L.be_last_error(None)

    # the Python surface: ValueError for the wrong kind, dtype, shape, device or contiguity
    pol, hp, g = pols[3], hps[3], good[3]["keep"]
    with pytest.raises(ValueError):
        HipBlockOptim(hp, pol, "rmsprop")
    for bad_pol in (copy.deepcopy(pol).double(), BlockPolicy(3, 16, 9).to(gpu), BlockPolicy(3, 32, 4).to(gpu),
                    copy.deepcopy(pol).cpu(), pols[2]):
        with pytest.raises(ValueError):
            HipBlockOptim(hp, bad_pol)
    for kw in (dict(betas=(1.0, 0.999)), dict(eps=-1.0), dict(lr=-1.0)):
        with pytest.raises(ValueError):
            HipBlockOptim(hp, pol, **kw)
    k1 = "affine1.weight"
    for k, bad in ((k1, g[k1].double()), (k1, g[k1].t().contiguous().t()), ("affine1.bias", g["affine1.bias"][:-1]),
                   ("affine3.bias", g["affine3.bias"].cpu())):
        with pytest.raises(ValueError):
            opt.step({**g, k: bad})
    with pytest.raises(ValueError):
        opt.step()                                                       # no .grad yet
    with pytest.raises(ValueError):
        opt.step(g, losses.float())
    torch.cuda.synchronize(gpu)
    for layers in (3, 2):
        for k, p in pols[layers].named_parameters():
            assert bool((p == SENT).all()), f"{k} ({layers} layers) was written by a rejected call"
    assert torch.equal(opt.state, before[0]) and torch.equal(opt.loss_log, before[1])
    _same(opt.exp_avg, before[2], "exp_avg after the rejected calls")
    assert env.status() == 0
    # .grad is the default source of the gradients
    for k, p in pol.named_parameters():
        p.grad = g[k].clone()
    opt.step()
    assert opt.step_count() == 1 and not bool((pol.affine1.weight == SENT).all())
    opt.zero_grad()
    assert all(p.grad is None for p in pol.parameters())
    for hp in hps.values():
        hp.close()
    env.close()


def _rule(w, w64, w32, w0, tag):
    for k in w64:
        moved = np.abs(w64[k] - w0[k].astype(np.float64)).max()
        err = np.abs(w[k].astype(np.float64) - w64[k]).max() / moved
        err32 = np.abs(w32[k].astype(np.float64) - w64[k]).max() / moved
        print(f"{tag} {k}: err={err:.3e} err_torch_f32={err32:.3e}")
        assert err <= 4 * err32 + 1e-6, (tag, k, err, err32)


def _torch_opt(kind, params, lr=LR):
    return torch.optim.Adam(params, lr=lr, betas=BETAS, eps=EPS) if kind == "adam" else torch.optim.SGD(params, lr=lr)


def _torch_run(kind, w0, grads, dtype):
    """`len(grads)` steps of torch's optimiser on copies of w0 in `dtype`, on the CPU."""
    ps = {k: torch.nn.Parameter(torch.from_numpy(w0[k].copy()).to(dtype)) for k in w0}
    opt = _torch_opt(kind, list(ps.values()))
    for g in grads:
        for k, p in ps.items():
            p.grad = torch.from_numpy(g[k].copy()).to(dtype)
        opt.step()
    return {k: p.detach().numpy() for k, p in ps.items()}


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_interchange(gpu, kind):
    """3 steps in HipBlockOptim, its state_dict() into torch's optimiser for 2 more: the 5 steps against
    torch's f64 run under the 4x + 1e-6 rule, next to 5 steps of the restatement.  Back from torch's
    state_dict a HipBlockOptim continues bit-equal to the restatement started from that state."""
    from gym_ballenv_amd import HipBlockOptim, HipBlockPolicy
    layers, h1, h2, A, final_relu, _ = SHAPES[0]
    env = make(gpu, 64)
    pol = random_policy(layers, h1, h2, A, final_relu, seed=4).to(gpu)
    hp = HipBlockPolicy(env, pol)
    opt = HipBlockOptim(hp, pol, kind, lr=LR, betas=BETAS, eps=EPS)
    assert opt.state_dict()["state"] == {}                               # as a fresh torch optimiser
    rng = np.random.default_rng(3)
    w0 = _np(_weights(pol))
    grads = [{k: rng.standard_normal(x.shape).astype(np.float32) for k, x in w0.items()} for _ in range(5)]
    dev = lambda g: {k: torch.from_numpy(x).to(gpu) for k, x in g.items()}     # noqa: E731
    for g in grads[:3]:
        opt.step(dev(g))
    sd = opt.state_dict()
    if kind == "adam":
        assert sorted(sd["state"]) == list(range(2 * layers)) and float(sd["state"][0]["step"]) == 3.0
    else:
        assert sd["state"] == {} and sd["param_groups"][0]["momentum"] == 0
    topt = _torch_opt(kind, list(pol.parameters()), lr=0.5)
    topt.load_state_dict(copy.deepcopy(sd))
    assert topt.param_groups[0]["lr"] == LR
    for g in grads[3:]:
        for k, p in pol.named_parameters():
            p.grad = torch.from_numpy(g[k]).to(gpu)
        topt.step()
    torch.cuda.synchronize(gpu)
    w64, w32 = _torch_run(kind, w0, grads, torch.float64), _torch_run(kind, w0, grads, torch.float32)
    w, state = {k: x.copy() for k, x in w0.items()}, fresh_state(LR)
    m, v = ({k: np.zeros_like(x) for k, x in w0.items()} for _ in range(2))
    for g in grads:
        _ref_step(kind, w, g, m, v, state)
    _rule(w, w64, w32, w0, "restatement, 5 steps")
    _rule(_np(_weights(pol)), w64, w32, w0, "3 HIP + 2 torch steps")
    if kind == "adam":
        assert float(topt.state_dict()["state"][0]["step"]) == 5.0

    # the reverse direction: torch's state into a fresh HipBlockOptim; bit-equal to the restatement from there
    opt_b = HipBlockOptim(hp, pol, kind, lr=0.5)
    opt_b.load_state_dict(topt.state_dict())
    assert opt_b.lr == LR
    w = _np(_weights(pol))
    if kind == "adam":
        assert opt_b.step_count() == 5 and opt_b.betas == BETAS and opt_b.eps == EPS
        tsd = topt.state_dict()["state"]
        m = {k: tsd[i]["exp_avg"].cpu().numpy().copy() for i, k in enumerate(names(layers))}
        v = {k: tsd[i]["exp_avg_sq"].cpu().numpy().copy() for i, k in enumerate(names(layers))}
        state = fresh_state(LR)
        for _ in range(5):
            state[1:3] *= BETAS
        state[0] = 5
    else:
        assert opt_b.step_count() == 0
        m = v = None
        state = fresh_state(LR)
    assert opt_b.state.cpu().numpy().tobytes() == state.tobytes()
    for s in range(2):
        g = _crafted_grads(gpu, pol, s)
        opt_b.step(g)
        _ref_step(kind, w, _np(g), m, v, state)
    torch.cuda.synchronize(gpu)
    _same(_weights(pol), w, "after the load from torch")
    assert opt_b.state.cpu().numpy().tobytes() == state.tobytes()
    if kind == "adam":
        _same(opt_b.exp_avg, m, "exp_avg after the load from torch")
    # a HipBlockOptim round trip
    opt_c = HipBlockOptim(hp, pol, kind)
    opt_c.load_state_dict(copy.deepcopy(opt_b.state_dict()))
    assert opt_c.lr == LR and (kind == "sgd" or torch.equal(opt_c.state, opt_b.state))

    # hyperparameters outside the supported set
    base = topt.state_dict()
    bad_keys = [("weight_decay", 0.1), ("maximize", True)]
    bad_keys += [("amsgrad", True)] if kind == "adam" else [("momentum", 0.9), ("nesterov", True), ("dampening", 0.5)]
    for key, val in bad_keys:
        bad = copy.deepcopy(base)
        bad["param_groups"][0][key] = val
        with pytest.raises(ValueError):
            opt_c.load_state_dict(bad)
    other = _torch_opt("sgd" if kind == "adam" else "adam", list(pol.parameters())).state_dict()
    with pytest.raises(ValueError):
        opt_c.load_state_dict(other)
    hp.close()
    env.close()


def _trainer_env(gpu, N):
    """N envs just reset, the first 64 ten steps before the TimeLimit: their episodes end inside the horizon."""
    env = make(gpu, N, seed=5)
    env.ep_len[:64] = 990
    return env


@pytest.mark.parametrize("captured", [False, True])
def test_block_trainer_equals_hand_loop(gpu, captured):
    """BlockTrainer.train(3), eager and captured, against run_eager() -> a2c_targets -> BlockGrad -> the
    gradients to the host -> adam_step_ref -> the weights back -> HipBlockPolicy.load: the final weights and the
    3 loss-log rows equal bit for bit."""
    from gym_ballenv_amd import BlockGrad, BlockRollout, BlockTrainer, a2c_targets
    T, N = 32, 512
    pol_t = ref_policy("supervised3").to(gpu)
    pol_h = copy.deepcopy(pol_t)
    w_start = _weights(pol_t)
    env_t, env_h = _trainer_env(gpu, N), _trainer_env(gpu, N)
    tr = BlockTrainer(env_t, pol_t, horizon=T, gamma=0.99, lr=LR, betas=BETAS, eps=EPS, seed=6, log_rows=8, chunk=T)
    ro = BlockRollout(env_h, pol_h, horizon=T, record_obs=True, seed=6)
    bg = BlockGrad(env_h, pol_h)
    w = _np(_weights(pol_h))
    m, v = ({k: np.zeros_like(x) for k, x in w.items()} for _ in range(2))
    state, hand_log, ended = fresh_state(LR), [], False
    for _ in range(3):
        ro.run_eager()
        tg = a2c_targets(env_h, ro.rewards, ro.dones, None, 0.99, F32_EPS, with_returns=False)
        g = bg(ro.blocks, ro.actions, tg.returns_norm, tg.valid, "reinforce", 1.0)
        torch.cuda.synchronize(gpu)
        ended = ended or bool(ro.dones[:-1].any())
        hand_log.append(bg.losses.cpu().numpy().copy())
        adam_step_ref(w, _np(g), m, v, state, *BETAS, EPS)
        with torch.no_grad():
            for k, p in pol_h.named_parameters():
                p.copy_(torch.from_numpy(w[k]))
        ro.hp.load(pol_h)
    assert ended, "no episode ended inside the horizon"
    with _OwnStream(gpu) as s:
        if captured:
            tr.capture(stream=s)
        tr.train(3)
        torch.cuda.synchronize(gpu)
        _same(_weights(pol_t), w, "weights")
        _same(tr.opt.exp_avg, m, "exp_avg")
        _same(tr.opt.exp_avg_sq, v, "exp_avg_sq")
        assert tr.opt.state.cpu().numpy().tobytes() == state.tobytes()
        for a, b in ((tr.rollout.actions, ro.actions), (tr.rollout.rewards, ro.rewards), (env_t.ep_len, env_h.ep_len)):
            assert torch.equal(a, b)
        log = tr.losses().numpy()
        assert log.shape == (3, 2) and log.tobytes() == np.array(hand_log).tobytes()
        assert log[0, 1] > 0 and not np.array_equal(log[0], log[1])
        for k, x in w_start.items():
            assert not torch.equal(x, dict(pol_t.named_parameters())[k].detach()), k
        assert env_t.status() == 0
        tr.close()
    ro.close()
    env_t.close()
    env_h.close()


def _hand_supervised(gpu, env, pol, blocks, labels, batch, epochs):
    """train_supervise.py's loop by hand: BlockGrad per minibatch, sgd_step_ref on the host, the weights back."""
    from gym_ballenv_amd import BlockGrad
    bg = BlockGrad(env, pol)
    w, state, log = _np(_weights(pol)), fresh_state(LR), []
    rows = blocks.shape[0]
    for _ in range(epochs):
        for i in range(0, rows, batch):
            j = min(rows, i + batch)
            g = bg(blocks[i:j], labels[i:j], None, None, "xent", 1 / (j - i))
            torch.cuda.synchronize(gpu)
            log.append(bg.losses.cpu().numpy().copy())
            sgd_step_ref(w, _np(g), state)
            with torch.no_grad():
                for k, p in pol.named_parameters():
                    p.copy_(torch.from_numpy(w[k]))
    return w, state, np.array(log)


@pytest.mark.parametrize("rows,batch,sizes", [(None, 200, [200] * 15 + [186]), (150, 63, [63, 63, 24])])
def test_supervised_trainer_equals_hand_loop(gpu, rows, batch, sizes):
    """Two epochs on the reference's recorded trial (all of it at the reference's batch of 200; its first 150
    rows at batch 63, whose slices start at byte offsets that are no multiple of 4): eager == captured == the
    hand loop, bit for bit, and the log's second column is the minibatch sizes, twice."""
    from gym_ballenv_amd import HipBlockPolicy, SupervisedTrainer
    fb, fl = _fixture()
    blocks, labels = torch.from_numpy(fb[:rows]).to(gpu), torch.from_numpy(fl[:rows]).to(gpu)
    env = make(gpu, 64)
    torch.manual_seed(0)
    from gym_ballenv_amd import BlockPolicy
    pol0 = BlockPolicy(3, 128, final_relu=False).to(gpu)
    pol_h = copy.deepcopy(pol0)
    w, state, hand_log = _hand_supervised(gpu, env, pol_h, blocks, labels, batch, 2)
    assert hand_log[:, 1].tolist() == sizes * 2
    probe = random_rows(64, seed=2).to(gpu)
    with _OwnStream(gpu) as s:
        for captured in (False, True):
            pol = copy.deepcopy(pol0)
            tr = SupervisedTrainer(env, pol, blocks, labels, batch_size=batch, lr=LR, log_rows=2 * len(sizes))
            if captured:
                tr.capture(stream=s)
            tr.train(2)
            torch.cuda.synchronize(gpu)
            tag = "captured" if captured else "eager"
            _same(_weights(pol), w, f"{tag}: weights")
            assert tr.opt.state.cpu().numpy().tobytes() == state.tobytes(), tag
            log = tr.losses().numpy()
            assert log.shape == (2 * len(sizes), 2) and log.tobytes() == hand_log.tobytes(), tag
            fresh = HipBlockPolicy(env, pol, probs=True)          # the trainer's own policy acts with the new weights
            assert torch.equal(_act(tr.hp, probe)[0], _act(fresh, probe)[0]), tag
            fresh.close()
            tr.close()
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_supervised_trainer_learns(gpu, seed):
    """4 epochs at the reference's batch and rate from torch.manual_seed(seed): the mean logged loss of epoch 4
    is below epoch 1's."""
    from gym_ballenv_amd import BlockPolicy, SupervisedTrainer
    fb, fl = _fixture()
    blocks, labels = torch.from_numpy(fb).to(gpu), torch.from_numpy(fl).to(gpu)
    env = make(gpu, 64)
    torch.manual_seed(seed)
    pol = BlockPolicy(3, 128, final_relu=False).to(gpu)
    tr = SupervisedTrainer(env, pol, blocks, labels, batch_size=200, lr=1e-2, log_rows=64)
    tr.train(4)
    log = tr.losses().numpy()
    assert log.shape == (64, 2)
    first, last = log[:16, 0].mean(), log[48:, 0].mean()
    print(f"seed {seed}: epoch 1 mean {first:.4f}, epoch 4 mean {last:.4f}")
    assert np.isfinite(log).all() and last < first, (first, last)
    tr.close()
    env.close()


def test_updates_accept_hip_block_optim(gpu):
    """reinforce_update(ro, HipBlockOptim, grads="hip") and supervised_update(..., HipBlockOptim("sgd"),
    grads="hip", grad=bg) leave the weights the trainers' update() leaves on the same inputs, bit for bit, with
    no .grad copies."""
    from gym_ballenv_amd import (BlockGrad, BlockRollout, BlockTrainer, HipBlockOptim, HipBlockPolicy,
                                 SupervisedTrainer, reinforce_update, supervised_update)
    T, N = 16, 128
    pol_t = ref_policy("supervised3").to(gpu)
    pol_u = copy.deepcopy(pol_t)
    env_t, env_u = _trainer_env(gpu, N), _trainer_env(gpu, N)
    tr = BlockTrainer(env_t, pol_t, horizon=T, lr=LR, seed=6, log_rows=2)
    ro = BlockRollout(env_u, pol_u, horizon=T, record_obs=True, seed=6)
    opt = HipBlockOptim(ro.hp, pol_u, "adam", lr=LR)
    tr.rollout.run_eager()
    tr.update()
    ro.run_eager()
    loss = reinforce_update(ro, opt, gamma=0.99, targets="hip", grads="hip")
    torch.cuda.synchronize(gpu)
    _same(_weights(pol_u), _weights(pol_t), "reinforce_update")
    assert loss == float(tr.losses()[0, 0]) and opt.step_count() == 1
    assert all(p.grad is None for p in pol_u.parameters())
    probe = random_rows(N, seed=3).to(gpu)
    for a, b in zip(_act(ro.hp, probe), _act(tr.rollout.hp, probe)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):                                      # bound to another HipBlockPolicy
        other = BlockRollout(env_u, pol_u, horizon=2, record_obs=True)
        try:
            reinforce_update(other, opt, grads="hip")
        finally:
            other.close()
    with pytest.raises(ValueError):
        reinforce_update(ro, opt, targets="hip", grads="torch")
    tr.close()
    ro.close()
    env_t.close()

    fb, fl = _fixture()
    blocks, labels = torch.from_numpy(fb[:200]).to(gpu), torch.from_numpy(fl[:200]).to(gpu)
    torch.manual_seed(1)
    from gym_ballenv_amd import BlockPolicy
    pol_s = BlockPolicy(3, 128, final_relu=False).to(gpu)
    pol_v = copy.deepcopy(pol_s)
    st = SupervisedTrainer(env_u, pol_s, blocks, labels, batch_size=200, lr=LR, log_rows=1)
    st.epoch()
    hp = HipBlockPolicy(env_u, pol_v)
    bg, sopt = BlockGrad(env_u, pol_v), HipBlockOptim(hp, pol_v, "sgd", lr=LR)
    loss = supervised_update(pol_v, blocks, labels, optimizer=sopt, grads="hip", grad=bg)
    torch.cuda.synchronize(gpu)
    _same(_weights(pol_v), _weights(pol_s), "supervised_update")
    assert loss == float(st.losses()[0, 0]) and all(p.grad is None for p in pol_v.parameters())
    with pytest.raises(ValueError):
        supervised_update(pol_s, blocks, labels, optimizer=sopt, grads="hip", grad=st.grad)   # another module's
    st.close()
    hp.close()
    env_u.close()
