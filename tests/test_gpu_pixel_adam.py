"""be_cnn_adam on the GPU: bit-equal to the numpy restatement (tests/a2c_adam_ref.py's Adam), its re-packed
image equal to a fresh HipPixelPolicy.load of the new weights in both BatchNorm modes (the running
statistics' rows survive), the state advancing on the device and graph-capturable, interchangeable with
torch.optim.Adam's state_dict, a drop-in optimizer for pixel_reinforce_update, and the engine of
PixelTrainer."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import cnn_adam_ref as R
from a2c_adam_ref import adam_step_ref, fresh_state
from pixel_policy_cases import calibrated_policy, given_images, random_policy
from test_gpu_a2c_adam import _OwnStream, _crafted_grads
from test_gpu_pixel_grad import _env

pytestmark = pytest.mark.gpu

BETAS, EPS, LR = (0.9, 0.999), 1e-8, 1e-3
N = 4


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


def _grads(gpu, pol, step):
    """_crafted_grads with the conv biases' gradients as be_cnn_grad writes them: exact +0."""
    g = _crafted_grads(gpu, pol, step)
    for k in R.CONV_BIASES:
        g[k].zero_()
    return g


def _act(hp, img, quad, norm):
    hp.norm = norm
    out = hp.act(img, quad, seed=9)
    torch.cuda.synchronize()
    return [x.clone() for x in out if x is not None]


def _never_loaded(hp):
    """Replace the HipPixelPolicy's handle with one straight from be_cnn_create: an image no be_cnn_load has
    written."""
    from gym_ballenv_amd import _abi
    torch.cuda.synchronize()
    _abi.check(hp._lib.be_cnn_destroy(hp._h))
    h = C.c_void_p()
    _abi.check(hp._lib.be_cnn_create(hp.env._ctx, hp.num_actions, C.byref(h)), hp.env._ctx)
    hp._h = h


@pytest.mark.parametrize("A", [1, 9, 15])
def test_step_bit_equal_restatement_and_repack_equals_load(gpu, A):
    from gym_ballenv_amd import HipPixelAdam, HipPixelPolicy
    env = _env(gpu, N)
    env.reset()
    img, quad = given_images(N, 3)             # two noise images, two fixture images: no constant map
    # running statistics calibrated on these images: "running" mode then reaches the weights "sample" mode does
    pol = calibrated_policy(A, A, img).float().to(gpu)
    img, quad = img.to(gpu), quad.to(gpu)
    # the image the step must complete: another policy's weights under the same running statistics
    other = random_policy(77, A).to(gpu)
    with torch.no_grad():
        for bn, src in ((other.bn1, pol.bn1), (other.bn2, pol.bn2), (other.bn3, pol.bn3)):
            bn.running_mean.copy_(src.running_mean)
            bn.running_var.copy_(src.running_var)
    hp = HipPixelPolicy(env, other, probs=True)
    opt = HipPixelAdam(hp, pol, lr=LR, betas=BETAS, eps=EPS, log_rows=2)
    opt.loss_log.fill_(-7.0)
    losses = torch.tensor([1.5, 100.0], dtype=torch.float64, device=gpu)
    w, state = _np(_weights(pol)), fresh_state(LR)
    assert list(w) == list(R.PARAMS)
    biases = {k: w[k].copy() for k in R.CONV_BIASES}
    m, v = _np(opt.exp_avg), _np(opt.exp_avg_sq)
    for step in range(3):
        g = _grads(gpu, pol, step)
        opt.step(g, losses + step)
        torch.cuda.synchronize(gpu)
        adam_step_ref(w, _np(g), m, v, state, *BETAS, EPS)
        _same(_weights(pol), w, f"weights after step {step + 1}")
        _same(opt.exp_avg, m, f"exp_avg after step {step + 1}")
        _same(opt.exp_avg_sq, v, f"exp_avg_sq after step {step + 1}")
        assert opt.state.cpu().numpy().tobytes() == state.tobytes()
        assert not any(np.isnan(w[k]).any() for k in w)
        for k in R.CONV_BIASES:               # zero gradients: the weights and both moments bit-unchanged
            assert w[k].tobytes() == biases[k].tobytes() and not m[k].any() and not v[k].any()
            assert opt.exp_avg[k].cpu().numpy().tobytes() == np.zeros_like(biases[k]).tobytes()
        fresh = HipPixelPolicy(env, pol, probs=True)
        for norm in ("sample", "running"):
            for got, want, name in zip(_act(hp, img, quad, norm), _act(fresh, img, quad, norm),
                                       ("action", "log_prob", "probs")):
                assert torch.isfinite(want.float()).all()
                assert torch.equal(got, want), f"{name} after step {step + 1} ({norm}): re-pack != load"
        fresh.close()
    assert opt.step_count() == 3
    log = opt.loss_log.cpu().numpy()     # rows t % 2 of t = 0, 1, 2: row 0 holds step 2's, row 1 step 1's
    assert np.array_equal(log, (losses.cpu().numpy() + np.array([[2.0], [1.0]])))
    assert env.status() == 0
    hp.close()
    env.close()


def test_state_and_learning_rate(gpu):
    """opt.lr = x is stream-ordered: the step enqueued before it keeps the old rate, the next one takes
    the new; the step count advances by one per call."""
    from gym_ballenv_amd import HipPixelAdam, HipPixelPolicy
    env = _env(gpu, N)
    env.reset()
    pol = random_policy(5).to(gpu)
    hp = HipPixelPolicy(env, pol)
    opt = HipPixelAdam(hp, pol, lr=LR, betas=BETAS, eps=EPS)
    w, state = _np(_weights(pol)), fresh_state(LR)
    m, v = _np(opt.exp_avg), _np(opt.exp_avg_sq)
    gs = [_grads(gpu, pol, s) for s in range(3)]
    torch.cuda.synchronize(gpu)
    assert opt.step_count() == 0
    opt.step(gs[0])
    opt.lr = 2.5e-3                       # no synchronise in between
    opt.step(gs[1])
    torch.cuda.synchronize(gpu)
    assert opt.lr == 2.5e-3 and opt.step_count() == 2
    adam_step_ref(w, _np(gs[0]), m, v, state, *BETAS, EPS)
    state[3] = 2.5e-3
    adam_step_ref(w, _np(gs[1]), m, v, state, *BETAS, EPS)
    _same(_weights(pol), w, "weights after the learning-rate change")
    assert opt.state.cpu().numpy().tobytes() == state.tobytes()
    opt.step(gs[2])
    assert opt.step_count() == 3
    adam_step_ref(w, _np(gs[2]), m, v, state, *BETAS, EPS)
    _same(_weights(pol), w, "weights after step 3")
    hp.close()
    env.close()


def _recorded_rows(gpu, env, pol, T):
    """T steps of every env recorded by a PixelRollout, with their targets: T * N rows."""
    from gym_ballenv_amd import PixelRollout, a2c_targets
    ro = PixelRollout(env, copy.deepcopy(pol), T, seed=5, record_images=True)
    ro.run_eager()
    t = a2c_targets(env, ro.rewards, ro.dones, None, 0.99, with_returns=False)
    torch.cuda.synchronize(gpu)
    data = tuple(x.clone() for x in (ro.images, ro.quadrants, ro.actions, t.returns_norm, t.valid))
    ro.close()
    return data


def test_captured_chain_equals_eager(gpu):
    """PixelGrad + step on 8 recorded rows, captured once on a stream of the test's own and replayed: 3 replays
    equal 3 eager iterations bit for bit (each replay's gradients come from the weights the one before wrote),
    then 2 more; after 5 steps the 2-row ring holds step 3's losses in row 1 and step 4's in row 0."""
    from gym_ballenv_amd import HipPixelAdam, HipPixelPolicy, PixelGrad
    env = _env(gpu, N)
    env.reset()
    data = _recorded_rows(gpu, env, random_policy(3).to(gpu), 2)
    assert data[0].shape[0] * data[0].shape[1] == 8 and int(data[4].sum()) == 8
    sides = []
    for _ in range(2):
        pol = random_policy(3).to(gpu)
        hp = HipPixelPolicy(env, pol, probs=True)
        sides.append((pol, hp, PixelGrad(env, pol), HipPixelAdam(hp, pol, lr=LR, log_rows=2)))
    (pe, hpe, pge, ope), (pc, hpc, pgc, opc) = sides
    seen = []

    def eager(n):
        for _ in range(n):
            ope.step(pge(*data), pge.losses)
            torch.cuda.synchronize(gpu)
            seen.append(pge.losses.clone())

    def compare(tag):
        _same(_weights(pc), _weights(pe), f"{tag}: weights")
        _same(opc.exp_avg, ope.exp_avg, f"{tag}: exp_avg")
        _same(opc.exp_avg_sq, ope.exp_avg_sq, f"{tag}: exp_avg_sq")
        assert torch.equal(opc.state, ope.state) and torch.equal(opc.loss_log, ope.loss_log), tag

    eager(3)
    with _OwnStream(gpu) as s:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            opc.step(pgc(*data), pgc.losses)
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
    assert not torch.equal(seen[3], seen[4]) and seen[4][1] == 8
    img, quad = (x.to(gpu) for x in given_images(N, 3))
    for a, b in zip(_act(hpc, img, quad, "sample"), _act(hpe, img, quad, "sample")):
        assert torch.equal(a, b)
    hpe.close()
    hpc.close()
    env.close()


def test_argument_errors_are_rejected_before_any_launch(gpu):
    from gym_ballenv_amd import HipPixelAdam, HipPixelPolicy, PixelPolicy, _abi
    env = _env(gpu, N)
    env.reset()
    SENT = 123.25
    pol = random_policy(6).to(gpu)
    with torch.no_grad():
        for p in pol.parameters():
            p.fill_(SENT)
    hp = HipPixelPolicy(env, pol)
    opt = HipPixelAdam(hp, pol, log_rows=2)
    for d in (opt.exp_avg, opt.exp_avg_sq):
        for x in d.values():
            x.fill_(SENT)
    opt.loss_log.fill_(SENT)
    g = _grads(gpu, pol, 0)
    ptrs = lambda d: [d[k].data_ptr() for k in R.PARAMS]    # noqa: E731
    good = dict(params=ptrs(dict(pol.named_parameters())), grads=ptrs(g), exp_avg=ptrs(opt.exp_avg),
                exp_avg_sq=ptrs(opt.exp_avg_sq))
    losses = torch.ones(2, dtype=torch.float64, device=gpu)
    torch.cuda.synchronize(gpu)
    before = (opt.state.clone(), opt.loss_log.clone())
    L = _abi.lib()

    def call(handle=None, state=opt.state.data_ptr(), beta1=0.9, beta2=0.999, eps=1e-8, losses_p=None, log_p=None,
             rows=0, null_struct=(), **sets):
        args = [None if name in null_struct else C.byref(_abi.BeCnnTensors(*sets.get(name, good[name])))
                for name in ("params", "grads", "exp_avg", "exp_avg_sq")]
        return L.be_cnn_adam(hp._h if handle is None else handle, *args, state, beta1, beta2, eps, losses_p, log_p, rows,
                             env._stream())

    def rejected(msg, **kw):
        assert call(**kw) == _abi.BE_E_INVALID, kw
        err = L.be_last_error(env._ctx).decode()
        assert "be_cnn_adam" in err and msg in err, (err, msg)

    for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
        rejected(f"{name} is NULL", null_struct=(name,))
        for i, k in enumerate(R.PARAMS):                                   # each NULL or misaligned pointer, named
            for bad in (None, good[name][i] + 2):
                p = list(good[name])
                p[i] = bad
                rejected(f"{name}->{k.replace('.', '_')} is NULL or not 4-byte aligned", **{name: p})
    rejected("state", state=None)
    rejected("state", state=opt.state.data_ptr() + 4)
    rejected("beta1", beta1=1.0)
    rejected("beta1", beta1=-0.1)
    rejected("beta2", beta2=1.0)
    rejected("beta2", beta2=-0.1)
    rejected("eps", eps=-1.0)
    rejected("losses and loss_log", losses_p=losses.data_ptr())
    rejected("losses and loss_log", log_p=opt.loss_log.data_ptr(), rows=2)
    rejected("not 8-byte aligned", losses_p=losses.data_ptr() + 4, log_p=opt.loss_log.data_ptr(), rows=2)
    rejected("not 8-byte aligned", losses_p=losses.data_ptr(), log_p=opt.loss_log.data_ptr() + 4, rows=2)
    rejected("log_rows", losses_p=losses.data_ptr(), log_p=opt.loss_log.data_ptr(), rows=0)
    rejected("log_rows", losses_p=losses.data_ptr(), log_p=opt.loss_log.data_ptr(), rows=-1)
    assert L.be_cnn_adam(None, None, None, None, None, None, 0.9, 0.999, 1e-8, None, None, 0, None) == _abi.BE_E_INVALID
    assert b"cnn is NULL" in L.be_last_error(None)
    # a handle straight from be_cnn_create: the running statistics' rows were never written
    h = C.c_void_p()
    _abi.check(L.be_cnn_create(env._ctx, 9, C.byref(h)), env._ctx)
    rejected("be_cnn_adam before be_cnn_load", handle=h)
    _abi.check(L.be_cnn_destroy(h))

    # the Python surface: ValueError for the wrong dtype, shape, device, contiguity or module
    for bad_pol in (copy.deepcopy(pol).double(), PixelPolicy(4).to(gpu), copy.deepcopy(pol).cpu(),
                    torch.nn.Linear(3, 2).to(gpu)):
        with pytest.raises(ValueError):
            HipPixelAdam(hp, bad_pol)
    for kw in (dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(eps=-1.0), dict(lr=-1.0), dict(eps=0.0)):
        with pytest.raises(ValueError):
            HipPixelAdam(hp, pol, **kw)
    k1 = "conv2.weight"
    for k, bad in ((k1, g[k1].double()), (k1, g[k1].transpose(2, 3).contiguous().transpose(2, 3)),
                   ("bn1.bias", g["bn1.bias"][:-1]), ("head.bias", g["head.bias"].cpu())):
        with pytest.raises(ValueError):
            opt.step({**g, k: bad})
    with pytest.raises(ValueError):
        opt.step()                                                       # no .grad yet
    with pytest.raises(ValueError):
        opt.step(g, losses.float())
    torch.cuda.synchronize(gpu)
    for k, p in pol.named_parameters():
        assert bool((p == SENT).all()), f"{k} was written by a rejected call"
        assert bool((opt.exp_avg[k] == SENT).all()) and bool((opt.exp_avg_sq[k] == SENT).all()), k
    assert torch.equal(opt.state, before[0]) and torch.equal(opt.loss_log, before[1])
    assert env.status() == 0
    # .grad is the default source of the gradients
    for d in (opt.exp_avg, opt.exp_avg_sq):
        for x in d.values():
            x.zero_()
    for k, p in pol.named_parameters():
        p.grad = g[k].clone()
    opt.step()
    assert opt.step_count() == 1 and not bool((pol.conv1.weight == SENT).all())
    assert bool((pol.conv1.bias == SENT).all())                          # its gradient is zero
    opt.zero_grad()
    assert all(p.grad is None for p in pol.parameters())
    hp.close()
    env.close()


def _rule(w, w64, w32, w0, tag):
    for k in w64:
        moved = np.abs(w64[k] - w0[k].astype(np.float64)).max()
        err = np.abs(w[k].astype(np.float64) - w64[k]).max() / moved
        err32 = np.abs(w32[k].astype(np.float64) - w64[k]).max() / moved
        print(f"{tag} {k}: err={err:.3e} err_torch_f32={err32:.3e}")
        assert err <= 4 * err32 + 1e-6, (tag, k, err, err32)


def _torch_run(w0, grads, dtype):
    """`len(grads)` steps of torch.optim.Adam on copies of w0 in `dtype`, on the CPU."""
    ps = {k: torch.nn.Parameter(torch.from_numpy(w0[k].copy()).to(dtype)) for k in w0}
    opt = torch.optim.Adam(list(ps.values()), lr=LR, betas=BETAS, eps=EPS)
    for g in grads:
        for k, p in ps.items():
            p.grad = torch.from_numpy(g[k].copy()).to(dtype)
        opt.step()
    return {k: p.detach().numpy() for k, p in ps.items()}


def test_state_dict_interchange(gpu):
    """3 steps in HipPixelAdam, its state_dict() into torch.optim.Adam for 2 more: the 5 steps against torch's
    f64 run under the 4x + 1e-6 rule, next to 5 steps of the restatement.  Back from torch's state_dict a
    HipPixelAdam continues bit-equal to the restatement started from that state."""
    from gym_ballenv_amd import HipPixelAdam, HipPixelPolicy
    env = _env(gpu, N)
    env.reset()
    pol = random_policy(4).to(gpu)
    hp = HipPixelPolicy(env, pol)
    opt = HipPixelAdam(hp, pol, lr=LR, betas=BETAS, eps=EPS)
    assert opt.state_dict()["state"] == {}                               # as a fresh torch optimiser
    rng = np.random.default_rng(3)
    w0 = _np(_weights(pol))
    grads = [{k: rng.standard_normal(x.shape).astype(np.float32) for k, x in w0.items()} for _ in range(5)]
    dev = lambda g: {k: torch.from_numpy(x).to(gpu) for k, x in g.items()}     # noqa: E731
    for g in grads[:3]:
        opt.step(dev(g))
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(14)) and float(sd["state"][0]["step"]) == 3.0
    topt = torch.optim.Adam(list(pol.parameters()), lr=0.5)
    topt.load_state_dict(copy.deepcopy(sd))
    assert topt.param_groups[0]["lr"] == LR
    for g in grads[3:]:
        for k, p in pol.named_parameters():
            p.grad = torch.from_numpy(g[k]).to(gpu)
        topt.step()
    torch.cuda.synchronize(gpu)
    w64, w32 = _torch_run(w0, grads, torch.float64), _torch_run(w0, grads, torch.float32)
    w, state = {k: x.copy() for k, x in w0.items()}, fresh_state(LR)
    m, v = ({k: np.zeros_like(x) for k, x in w0.items()} for _ in range(2))
    for g in grads:
        adam_step_ref(w, g, m, v, state, *BETAS, EPS)
    _rule(w, w64, w32, w0, "restatement, 5 steps")
    _rule(_np(_weights(pol)), w64, w32, w0, "3 HIP + 2 torch steps")
    assert float(topt.state_dict()["state"][0]["step"]) == 5.0

    # the reverse direction: torch's state into a fresh HipPixelAdam; bit-equal to the restatement from there
    opt_b = HipPixelAdam(hp, pol, lr=0.5)
    opt_b.load_state_dict(topt.state_dict())
    assert opt_b.lr == LR and opt_b.step_count() == 5 and opt_b.betas == BETAS and opt_b.eps == EPS
    w = _np(_weights(pol))
    tsd = topt.state_dict()["state"]
    m = {k: tsd[i]["exp_avg"].cpu().numpy().copy() for i, k in enumerate(R.PARAMS)}
    v = {k: tsd[i]["exp_avg_sq"].cpu().numpy().copy() for i, k in enumerate(R.PARAMS)}
    state = fresh_state(LR)
    for _ in range(5):
        state[1:3] *= BETAS
    state[0] = 5
    assert opt_b.state.cpu().numpy().tobytes() == state.tobytes()
    hp.load(pol)                                                         # torch's two steps did not re-pack
    for s in range(2):
        g = _crafted_grads(gpu, pol, s)
        opt_b.step(g)
        adam_step_ref(w, _np(g), m, v, state, *BETAS, EPS)
    torch.cuda.synchronize(gpu)
    _same(_weights(pol), w, "after the load from torch")
    assert opt_b.state.cpu().numpy().tobytes() == state.tobytes()
    _same(opt_b.exp_avg, m, "exp_avg after the load from torch")
    _same(opt_b.exp_avg_sq, v, "exp_avg_sq after the load from torch")
    # a HipPixelAdam round trip
    opt_c = HipPixelAdam(hp, pol)
    opt_c.load_state_dict(copy.deepcopy(opt_b.state_dict()))
    assert opt_c.lr == LR and torch.equal(opt_c.state, opt_b.state)

    # hyperparameters outside the supported set
    base = topt.state_dict()
    for key, val in (("weight_decay", 0.1), ("maximize", True), ("amsgrad", True), ("eps", 0.0)):
        bad = copy.deepcopy(base)
        bad["param_groups"][0][key] = val
        with pytest.raises(ValueError):
            opt_c.load_state_dict(bad)
    with pytest.raises(ValueError):
        opt_c.load_state_dict(torch.optim.SGD(list(pol.parameters()), lr=LR).state_dict())
    hp.close()
    env.close()


def _trainer_env(gpu, n):
    """n envs just reset, the first 4 ten steps before the TimeLimit: their episodes end inside the horizon."""
    env = _env(gpu, n, seed=5)
    env.reset()
    env.ep_len[:4] = 990
    return env


@pytest.mark.parametrize("captured", [False, True])
def test_pixel_trainer_equals_hand_loop(gpu, captured):
    """PixelTrainer.train(3), eager and captured, against run_eager() -> a2c_targets -> PixelGrad -> the
    gradients to the host -> adam_step_ref -> the weights back -> HipPixelPolicy.load: the final weights, the
    moments, the state, the recorded rollout and the 3 loss-log rows equal bit for bit."""
    from gym_ballenv_amd import PixelGrad, PixelRollout, PixelTrainer, a2c_targets
    T, n = 12, 8
    pol_t = random_policy(2).to(gpu)
    pol_h = copy.deepcopy(pol_t)
    w_start = _weights(pol_t)
    env_t, env_h = _trainer_env(gpu, n), _trainer_env(gpu, n)
    tr = PixelTrainer(env_t, pol_t, horizon=T, gamma=0.99, lr=LR, betas=BETAS, eps=EPS, seed=6, log_rows=8, chunk=T)
    assert tr.rollout.images is not None and tr.rollout.hp.norm == "sample" and tr.GRAPH_CHUNK == T
    ro = PixelRollout(env_h, pol_h, horizon=T, record_images=True, seed=6)
    pg = PixelGrad(env_h, pol_h)
    w = _np(_weights(pol_h))
    m, v = ({k: np.zeros_like(x) for k, x in w.items()} for _ in range(2))
    state, hand_log, ended = fresh_state(LR), [], False
    for _ in range(3):
        ro.run_eager()
        tg = a2c_targets(env_h, ro.rewards, ro.dones, None, 0.99, with_returns=False)
        g = pg(ro.images, ro.quadrants, ro.actions, tg.returns_norm, tg.valid, scale=1.0)
        torch.cuda.synchronize(gpu)
        ended = ended or bool(ro.dones[:-1].any())
        hand_log.append(pg.losses.cpu().numpy().copy())
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
        now = dict(pol_t.named_parameters())
        for k, x in w_start.items():
            assert torch.equal(x, now[k].detach()) == (k in R.CONV_BIASES), k
        assert env_t.status() == 0
        tr.close()
    ro.close()
    env_t.close()
    env_h.close()


def test_pixel_reinforce_update_accepts_hip_pixel_adam(gpu):
    """pixel_reinforce_update(ro, HipPixelAdam, grads="hip") leaves the weights PixelTrainer.update() leaves on
    the same inputs, bit for bit, with no .grad copies."""
    from gym_ballenv_amd import HipPixelAdam, PixelRollout, PixelTrainer, pixel_reinforce_update
    T, n = 6, 4
    pol_t = random_policy(2).to(gpu)
    pol_u = copy.deepcopy(pol_t)
    env_t, env_u = _trainer_env(gpu, n), _trainer_env(gpu, n)
    tr = PixelTrainer(env_t, pol_t, horizon=T, lr=LR, seed=6, log_rows=2)
    ro = PixelRollout(env_u, pol_u, horizon=T, record_images=True, seed=6)
    opt = HipPixelAdam(ro.hp, pol_u, lr=LR)
    tr.rollout.run_eager()
    tr.update()
    ro.run_eager()
    loss = pixel_reinforce_update(ro, opt, gamma=0.99, targets="hip", grads="hip")
    torch.cuda.synchronize(gpu)
    _same(_weights(pol_u), _weights(pol_t), "pixel_reinforce_update")
    assert loss == float(tr.losses()[0, 0]) and opt.step_count() == 1
    assert all(p.grad is None for p in pol_u.parameters())
    img, quad = (x.to(gpu) for x in given_images(n, 3))
    for a, b in zip(_act(ro.hp, img, quad, "sample")[:2], _act(tr.rollout.hp, img, quad, "sample")[:2]):
        assert torch.equal(a, b)
    other = PixelRollout(env_u, pol_u, horizon=2, record_images=True)    # bound to another HipPixelPolicy
    try:
        with pytest.raises(ValueError):
            pixel_reinforce_update(other, opt, grads="hip")
    finally:
        other.close()
    with pytest.raises(ValueError):
        pixel_reinforce_update(ro, opt, targets="hip", grads="torch")
    assert opt.step_count() == 1
    tr.close()
    ro.close()
    env_t.close()
    env_u.close()


@pytest.mark.parametrize("seed", R.OVERFIT_SEEDS)
def test_overfits_the_fixed_rows(gpu, seed):
    """10 x (PixelGrad + HipPixelAdam.step) on the 8 fixed rows of tests/test_pixel_adam_host.py, where torch's
    own run is checked to descend: every logged loss is finite and the tenth is below the first."""
    from gym_ballenv_amd import HipPixelAdam, HipPixelPolicy, PixelGrad
    env = _env(gpu, N)
    env.reset()
    img, quad, act = (x.to(gpu) for x in R.overfit_rows())
    pol = random_policy(seed).float().to(gpu)
    hp = HipPixelPolicy(env, pol)
    pg, opt = PixelGrad(env, pol), HipPixelAdam(hp, pol, lr=1e-3, log_rows=10)
    for _ in range(10):
        opt.step(pg(img, quad, act), pg.losses)
    log = opt.losses().numpy()
    print(f"seed {seed}: " + " ".join(f"{x:.4f}" for x in log[:, 0]))
    assert log.shape == (10, 2) and np.isfinite(log).all() and (log[:, 1] == 8).all()
    assert log[9, 0] < log[0, 0], (log[0, 0], log[9, 0])
    hp.close()
    env.close()
