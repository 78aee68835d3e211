"""be_a2c_adam without a GPU: the pinned step (tests/a2c_adam_ref.py) against torch.optim.Adam, the
rebuilt beta^t of HipAdam.load_state_dict, the pack restatement's digits, and the entry's
declaration, export and NULL-policy error."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from a2c_adam_ref import QMAX, adam_step_ref, fresh_state, pack_rows_ref

from gym_ballenv_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"fc1": (208, 104), "head": (9, 208), "scalar": (1,)}
BETAS, EPS, LR = (0.9, 0.999), 1e-8, 1e-3


def _grads(rng, scale):
    out = {}
    for k, s in SHAPES.items():
        g = (rng.standard_normal(s) * scale).astype(np.float32)
        g[rng.random(s) < 0.05] = 0.0            # 5 % exact zeros
        out[k] = g
    return out


def _torch_adam(w0, grads, dtype):
    ps = [torch.nn.Parameter(torch.from_numpy(w0[k].copy()).to(dtype)) for k in SHAPES]
    opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS)
    for g in grads:
        for p, k in zip(ps, SHAPES):
            p.grad = torch.from_numpy(g[k].copy()).to(dtype)
        opt.step()
    return {k: p.detach().double().numpy() for p, k in zip(ps, SHAPES)}


@pytest.mark.parametrize("steps", [1, 5, 50])
@pytest.mark.parametrize("scale", [1e-4, 1.0, 100.0])
def test_restatement_against_torch_adam(steps, scale):
    """Per tensor err = max|w - w64| / max|w64 - w0| with w64 torch's Adam on f64 copies; the pinned
    arithmetic may be at most 4x torch's own f32 Adam + 1e-6 away (the rule of tests/test_gpu_policy.py)."""
    rng = np.random.default_rng(1000 * steps + int(np.log10(scale)) + 7)
    w0 = {k: (rng.standard_normal(s) * 0.1).astype(np.float32) for k, s in SHAPES.items()}
    grads = [_grads(rng, scale) for _ in range(steps)]
    w64 = _torch_adam(w0, grads, torch.float64)
    w32 = _torch_adam(w0, grads, torch.float32)
    w = {k: x.copy() for k, x in w0.items()}
    m = {k: np.zeros_like(x) for k, x in w0.items()}
    v = {k: np.zeros_like(x) for k, x in w0.items()}
    state = fresh_state(LR)
    for g in grads:
        adam_step_ref(w, g, m, v, state, *BETAS, EPS)
    assert state[0] == steps and state[3] == LR
    for k in SHAPES:
        moved = np.abs(w64[k] - w0[k].astype(np.float64)).max()
        assert moved > 0
        err_ref = np.abs(w[k].astype(np.float64) - w64[k]).max() / moved
        err_t32 = np.abs(w32[k] - w64[k]).max() / moved
        print(f"steps={steps} scale={scale:g} {k}: err_restatement={err_ref:.3e} err_torch_f32={err_t32:.3e}")
        assert err_ref <= 4 * err_t32 + 1e-6, (k, err_ref, err_t32)


@pytest.mark.parametrize("t", [0, 1, 2, 50, 1000])
def test_rebuilt_beta_powers_equal_running_product(t):
    from gym_ballenv_amd.rollout import _beta_powers
    w = {"x": np.zeros(1, np.float32)}
    g, m, v = ({"x": np.zeros(1, np.float32)} for _ in range(3))
    state = fresh_state(LR)
    for _ in range(t):
        adam_step_ref(w, g, m, v, state, *BETAS, EPS)
    p1, p2 = _beta_powers(t, BETAS)
    assert state[0] == t
    assert np.float64(p1).tobytes() == state[1].tobytes() and np.float64(p2).tobytes() == state[2].tobytes()
    if t == 1000:
        assert p2 != BETAS[1] ** t          # why the product is rebuilt, not beta ** t


def test_pack_restatement_digits():
    rng = np.random.default_rng(3)
    w1 = (rng.standard_normal((72, 53)) * 0.2).astype(np.float32)
    b1 = (rng.standard_normal(72) * 0.2).astype(np.float32)
    w1[5] = 0.0
    b1[5] = 0.0                              # an all-zero row: s = 1, every digit 0
    b1[6] = 100.0                            # the bias sets the row's step
    s, bq, (d2, d1, d0), q = pack_rows_ref(w1, b1)
    for d in (d2, d1, d0):
        assert d.min() >= -128 and d.max() <= 127
    assert np.array_equal(d2 * 65536 + d1 * 256 + d0, q)
    assert np.abs(q).max() <= QMAX and s[5] == 1.0 and not q[5].any() and bq[5] == 0
    assert abs(abs(int(bq[6])) - 64 * QMAX) <= 64       # |b1| / 64 was the row's maximum: bq = 64 * 127 * 2^16
    rows = (np.abs(w1).max(axis=1) >= np.abs(b1) / 64) & (np.abs(w1).max(axis=1) > 0)
    assert (np.abs(q[rows]).max(axis=1) >= QMAX - 1).all()      # the row's largest weight uses the 24 bits
    assert np.abs(q.astype(np.float64) * s[:, None] - w1).max() <= 0.5 * s.max() * (1 + 1e-6)


def test_library_declares_and_exports_the_entry():
    hdr = open(os.path.join(ROOT, "include", "ballenv.h")).read()
    assert re.search(r"\bint be_a2c_adam\(be_policy\* pol,", hdr)
    assert "typedef struct be_a2c_tensors" in hdr
    L = _abi.lib()
    assert hasattr(L, "be_a2c_adam") and L.be_a2c_adam.argtypes is not None
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT be_a2c_adam\b", out)
    assert L.be_abi_version() == 7
    import gym_ballenv_amd as gb
    assert gb.HipAdam.__name__ == "HipAdam" and gb.A2CTrainer.__name__ == "A2CTrainer"


def test_null_policy_is_invalid():
    L = _abi.lib()
    t = _abi.BeA2CTensors()
    rc = L.be_a2c_adam(None, C.byref(t), C.byref(t), C.byref(t), C.byref(t), None, 0.9, 0.999, 1e-8, None, None, 0,
                       None)
    assert rc == _abi.BE_E_INVALID
    assert b"policy is NULL" in L.be_last_error(None)
