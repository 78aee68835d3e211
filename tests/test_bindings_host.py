"""The shared pieces of the Python bindings on the CPU (no GPU, no library): a cold import in a fresh interpreter
(``_bind`` loads lazily, the three handles and the three rollouts share their base's methods, no import cycle),
``want``, ``categorical_pick`` against the draw as the three ``torch_*_select_action`` had it written out, and the
return recursion / episode ids against plain Python loops and the recorded outputs of both target functions."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _fresh(code):
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1])\n" + code +
                        "print('cold import: OK')\n", ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "cold import: OK" in r.stdout, r.stdout + r.stderr


def test_cold_import_and_shared_methods():
    _fresh("import gym_ballenv_amd as gb\n"
           "assert 'gym_ballenv_amd._bind' not in sys.modules and 'torch' not in sys.modules\n"
           "handles = (gb.HipPolicy, gb.HipBlockPolicy, gb.HipPixelPolicy)\n"
           "rollouts = (gb.Rollout, gb.BlockRollout, gb.PixelRollout)\n"
           "from gym_ballenv_amd._bind import HipHandle\n"
           "from gym_ballenv_amd.rollout import StepRollout\n"
           "for c in handles:\n"
           "    assert c.__mro__[1] is HipHandle\n"
           "    assert c.close is HipHandle.close and c.__del__ is HipHandle.__del__\n"
           "    assert c.packed_bytes is HipHandle.packed_bytes\n"
           "assert [c.SEED for c in handles] == [0x5E1EC7, 0x5E1EC7, 0]\n"
           "assert [c.VALUE for c in handles] == [True, False, False]\n"
           "for c in rollouts:\n"
           "    assert c.__mro__[1] is StepRollout\n"
           "    for m in ('run', 'run_eager', 'capture', 'step', 'close', 'run_fused'):\n"
           "        assert getattr(c, m) is getattr(StepRollout, m), (c, m)\n"
           "from gym_ballenv_amd.optim import RowGrad\n"
           "assert gb.A2CGrad.assign is gb.BlockGrad.assign is RowGrad.assign\n")


@pytest.mark.parametrize("order", [("rollout", "block_policy"), ("block_policy", "rollout")])
def test_no_import_cycle(order):
    _fresh(f"import gym_ballenv_amd.{order[0]} as a, gym_ballenv_amd.{order[1]} as b\n"
           "import gym_ballenv_amd.pixel_policy as px, gym_ballenv_amd._bind as bind\n"
           "ro = a if a.__name__.endswith('rollout') else b\n"
           "assert px.StepRollout is ro.StepRollout and px.HipHandle is bind.HipHandle\n")


def test_want():
    from gym_ballenv_amd._bind import fits, want
    from gym_ballenv_amd.optim import is_f32
    x = torch.zeros(4, 6, dtype=torch.uint8)
    assert want(x, "obs", torch.uint8, (4, 6), CPU) is x
    assert want(x, "obs", torch.uint8, (None, 6), CPU) is x
    assert want(x, "obs", (torch.bool, torch.uint8), (4, None), CPU) is x
    assert want(x.bool(), "obs", (torch.bool, torch.uint8), (4, 6), CPU).dtype == torch.bool
    assert want(None, "obs", torch.uint8, (4, 6), CPU, optional=True) is None
    assert want(torch.zeros((), dtype=torch.float64), "s", torch.float64, (), CPU).dim() == 0
    bad = {"dtype": x.float(), "rank": x[0], "rank+": x[None], "extent": torch.zeros(4, 5, dtype=torch.uint8),
           "view": torch.zeros(6, 4, dtype=torch.uint8).t(), "step": torch.zeros(4, 12, dtype=torch.uint8)[:, ::2],
           "device": torch.zeros(4, 6, dtype=torch.uint8, device="meta"), "list": [[0] * 6] * 4,
           "numpy": np.zeros((4, 6), np.uint8), "none": None}
    for why, y in bad.items():
        assert not fits(y, torch.uint8, (4, 6), CPU), why
        with pytest.raises(ValueError, match=r"the_arg must be a contiguous u8 tensor of shape \(4, 6\) on the env's device"):
            want(y, "the_arg", torch.uint8, (4, 6), CPU)
    with pytest.raises(ValueError, match=r"v must be a contiguous bool / u8 tensor of shape \(\*, 6\)"):
        want(x.float(), "v", (torch.bool, torch.uint8), (None, 6), CPU, optional=True)
    w = torch.zeros(3, 2)
    assert is_f32(w, (3, 2), CPU) and is_f32(w, w.shape, CPU)
    assert not is_f32(w.double(), (3, 2), CPU) and not is_f32(w.t(), (2, 3), CPU) and not is_f32(None, (3, 2), CPU)


def _pick_as_written(probs, u):
    """The draw as torch_select_action wrote it out before categorical_pick: the oracle."""
    cdf = probs.cumsum(-1)
    a = (cdf <= u.unsqueeze(-1)).sum(-1)
    nz = torch.arange(probs.shape[-1], device=probs.device).expand_as(probs).masked_fill(probs <= 0, 0)
    a = torch.minimum(a, nz.max(-1).values)
    logp = torch.log(probs.gather(-1, a.unsqueeze(-1))).squeeze(-1)
    return a, logp


def _same(got, ref):
    assert got[0].dtype == torch.int64 and torch.equal(got[0], ref[0])
    assert got[1].dtype == ref[1].dtype and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


@pytest.mark.parametrize("A", [1, 9, 15])
def test_categorical_pick(A):
    from gym_ballenv_amd._bind import categorical_pick
    g = torch.Generator().manual_seed(A)
    base = torch.softmax(3 * torch.randn(64, A, generator=g), -1)
    tail = base.clone()                         # trailing zero probabilities, renormalised
    tail[:, A - A // 3:] = 0
    tail = tail / tail.sum(-1, keepdim=True)
    hole = base.clone()                         # a zero in the middle and one at the end
    hole[:, A // 2] = 0
    hole[:, -1] = 0 if A > 1 else 1
    probs = torch.cat([base, tail, hole])
    cdf = probs.cumsum(-1)
    j = torch.arange(probs.shape[0]) % A
    us = [torch.zeros(probs.shape[0]), cdf.gather(-1, j[:, None]).squeeze(-1), cdf[:, -1].clone(),
          torch.ones(probs.shape[0]), torch.full((probs.shape[0],), 1.5), torch.rand(probs.shape[0], generator=g)]
    clamped = 0
    for u in us:
        got, ref = categorical_pick(probs, u), _pick_as_written(probs, u)
        _same(got, ref)
        assert int(got[0].max()) < A and bool((probs.gather(-1, got[0][:, None]) > 0).all())
        clamped += int(((cdf <= u[:, None]).sum(-1) > got[0]).sum())
    assert clamped > 0                          # the clamp to the last p > 0 was taken


def test_select_actions_return_the_pick():
    from gym_ballenv_amd._bind import categorical_pick
    from gym_ballenv_amd.block_policy import BlockPolicy, torch_block_select_action
    from gym_ballenv_amd.pixel_policy import PixelPolicy, torch_pixel_select_action
    from gym_ballenv_amd.policy import Policy, torch_select_action
    torch.manual_seed(5)
    N = 33
    u = torch.rand(N)
    with torch.no_grad():
        obs = (torch.rand(N, 29) < 0.3).to(torch.uint8)
        a, lp, v, pr = torch_select_action(Policy(5), obs, u)
        assert v.shape == (N,) and pr.shape == (N, 9)
        _same((a, lp), categorical_pick(pr, u))
        a, lp, pr = torch_block_select_action(BlockPolicy(3, 32, num_actions=15), torch.randint(0, 20, (N, 29)).to(torch.uint8), u)
        assert pr.shape == (N, 15)
        _same((a, lp), categorical_pick(pr, u))
        for norm in ("sample", "running"):
            a, lp, pr = torch_pixel_select_action(PixelPolicy(), torch.randint(0, 256, (N, 3, 40, 40)).to(torch.uint8),
                                                  torch.randint(0, 4, (N,)), u, norm)
            assert pr.shape == (N, 9)
            _same((a, lp), categorical_pick(pr, u))


# (T, N) = (7, 3): dones in the first row (env 0), in the last row (env 1) and in two rows in a row (env 2)
REWARDS = [[0.25, -0.75, 0.0], [0.25, 1.5, 1.0], [-1.75, 0.25, -0.25], [-1.5, -1.0, -1.25], [0.25, 1.75, -0.5],
           [1.5, 1.75, 1.5], [-0.5, 2.0, 1.0]]
DONES = [[1, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 0, 0], [0, 1, 0]]
GAMMA = 0.99
VALID = [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1]
# the bits of the f32 R^ the two functions returned for this case before their loops were shared
TORCH_TARGETS = [0, 1057954034, 1058152652, -1087281260, 1066746049, 1058371593, -1084135373, 1033735593, -1080832918,
                 1049698960, -1113677684, 0, 1067786049, 1060526849, 1044828201, 1060439283, -1089336075, 1063485677,
                 -1087044365, -1074863342, -1081435526]
EPISODE_TARGETS = [0, 1057954034, 1058152651, -1087281260, 1066746049, 1058371593, -1084135372, 1033735593, -1080832918,
                   1049698958, -1113677684, 0, 1067786048, 1060526849, 1044828197, 1060439282, -1089336075, 1063485677,
                   -1087044366, -1074863343, -1081435525]


def test_return_recursion_and_episode_ids():
    from gym_ballenv_amd.rollout import discounted, episode_ids
    r, d = torch.tensor(REWARDS, dtype=torch.float64), torch.tensor(DONES, dtype=torch.bool)
    T, N = r.shape
    for boot in (None, [0.5, -2.0, 3.25]):
        want_R = [[0.0] * N for _ in range(T)]
        for n in range(N):
            acc = 0.0 if boot is None else boot[n]
            for t in reversed(range(T)):
                want_R[t][n] = acc = REWARDS[t][n] + GAMMA * acc * (1.0 - DONES[t][n])
        b = None if boot is None else torch.tensor(boot, dtype=torch.float64)
        for dd in (d, d.to(torch.uint8)):
            R = discounted(r, dd, GAMMA, b)
            assert R.dtype == torch.float64 and torch.equal(R, torch.tensor(want_R, dtype=torch.float64))
        assert b is None or b.tolist() == boot                  # the bootstrap is not written
    seg = [sum(DONES[s][n] for s in range(t)) * N + n for t in range(T) for n in range(N)]
    order = sorted(set(seg))
    sid, S = episode_ids(d)
    # an episode per env, one more after every done but a done in the last row
    assert S == len(order) == N + sum(map(sum, DONES[:-1])) and sid.tolist() == [order.index(v) for v in seg]


def test_targets_reproduce_their_recorded_bits():
    from gym_ballenv_amd.block_policy import _episode_targets
    from gym_ballenv_amd.rollout import _torch_targets
    r, d = torch.tensor(REWARDS, dtype=torch.float64), torch.tensor(DONES, dtype=torch.bool)
    assert TORCH_TARGETS != EPISODE_TARGETS                     # f32 against f64 statistics: different on purpose
    for fn, bits in ((lambda: _torch_targets(r, d, GAMMA), TORCH_TARGETS),
                     (lambda: _episode_targets(r, d, GAMMA, float(np.finfo(np.float32).eps)), EPISODE_TARGETS)):
        Rn, valid = fn()
        assert Rn.dtype == torch.float32 and Rn.view(torch.int32).tolist() == bits
        assert valid.dtype == torch.bool and valid.int().tolist() == VALID
