"""CPU: be_cnn_grad's host side -- the float64 restatement of its contract (tests/cnn_grad_ref.py) against
float64 autograd, pixel_reinforce_losses against a per-episode loop written as the reference's finish_episode,
the declarations and exports, the rejection that needs no device, and csrc/cnn_grad_host.h (the workspace's
layout, the argument checks) in a stand-alone C++ program under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/cnn_grad_host_main.cpp).  No GPU and no HIP runtime."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cnn_grad_ref as R
from gym_ballenv_amd import _abi
from gym_ballenv_amd.pixel_policy import (GRAD_MAX_SLOTS, GRAD_TILE, GRAD_WAVES, PixelGrad, PixelPolicy,  # noqa: F401
                                          pixel_reinforce_losses, pixel_reinforce_update, torch_pixel_forward)
from pixel_policy_cases import random_policy, trained_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")


@pytest.mark.parametrize("which", ["random0", "random1", "trained"])
def test_restatement_equals_float64_autograd(which):
    pol = trained_policy() if which == "trained" else random_policy(int(which[-1]), 9)
    img, quad, act, coef, valid = R.inputs(pol, 13, 0 if which == "trained" else int(which[-1]))
    assert img.shape[0] == 13 and all(len(torch.unique(i)) > 1 for i in img)      # non-degenerate images
    act[3] = 9                                                                   # an out-of-range action: inactive
    mine = R.restatement(pol, img, quad, act, coef, valid)
    auto = R.torch_reference(pol, img, quad, act, coef, valid, torch.float64)
    assert mine.count == auto.count == int(((valid != 0) & (act < 9)).sum())
    assert abs(mine.loss - auto.loss) <= 1e-10 * mine.abs_loss
    assert (mine.probs - auto.probs).abs().max().item() <= 1e-12
    for k, e in R.errors(mine.grads, auto.grads).items():
        assert e <= 1e-10, (k, e)
    for i in (1, 2, 3):      # the per-map mean subtracts the bias: autograd leaves rounding noise there
        assert auto.grads[f"conv{i}.bias"].abs().max().item() <= 1e-9 * auto.grads[f"conv{i}.weight"].abs().max().item()
        assert torch.count_nonzero(mine.grads[f"conv{i}.bias"]) == 0


def test_restatement_scale_and_defaults():
    pol = random_policy(1, 9)
    img, quad, act, coef, valid = R.inputs(pol, 5, 1)
    ones = R.restatement(pol, img, quad, act, torch.ones(5), torch.ones(5, dtype=torch.uint8))
    none = R.restatement(pol, img, quad, act)
    half = R.restatement(pol, img, quad, act, scale=0.5)
    assert ones.loss == none.loss and half.loss == 0.5 * none.loss and half.count == none.count == 5
    for k in R.PARAMS:
        assert torch.equal(ones.grads[k], none.grads[k]) and torch.equal(half.grads[k], 0.5 * none.grads[k])


def test_pixel_reinforce_losses_is_finish_episode_per_episode():
    torch.manual_seed(0)
    pol = random_policy(0, 9).double()
    T, N, gamma = 7, 3, 0.9
    img, quad = R.drop_constant(*R.given_images(T * N + 4, 0))
    img, quad = img[:T * N].reshape(T, N, 3, 40, 40), quad[:T * N].reshape(T, N)
    actions = torch.randint(0, 9, (T, N), dtype=torch.uint8)
    rewards = torch.randn(T, N, dtype=torch.float64)
    dones = torch.zeros(T, N, dtype=torch.bool)
    dones[2, 0] = dones[3, 0] = dones[6, 1] = dones[0, 2] = True        # env 0: a one-step episode (step 3)
    got = pixel_reinforce_losses(pol, img, quad, actions, rewards, dones, gamma)
    eps = float(np.finfo(np.float32).eps)
    want = torch.zeros((), dtype=torch.float64)
    for n in range(N):
        start = 0
        for t in range(T):
            if dones[t, n] or t == T - 1:
                steps = list(range(start, t + 1))
                start = t + 1
                if len(steps) < 2:
                    continue                                             # std() of one element is NaN: left out
                Rr, rs = 0.0, []
                for s in steps[::-1]:                                    # ball_cnn_reinforce.py:102-104
                    Rr = float(rewards[s, n]) + gamma * Rr
                    rs.insert(0, Rr)
                rs = torch.tensor(rs)                                    # fp32, as the reference's
                rs = ((rs.double() - rs.double().mean()) / (rs.double().std() + eps)).float()
                for s, r in zip(steps, rs):
                    p = torch_pixel_forward(pol, img[s, n][None].double() / 255.0,
                                            torch.eye(4, dtype=torch.float64)[quad[s, n].long()][None], "sample")
                    lp = torch.distributions.Categorical(p).log_prob(actions[s, n].long()[None])
                    want = want + (-lp * r.double()).sum()
    got, want = float(got.detach()), float(want.detach())
    assert abs(got - want) <= 1e-9 * max(1.0, abs(want))
    with pytest.raises(ValueError):
        pixel_reinforce_losses(pol, img, quad, actions, rewards, dones, gamma, targets=(rewards[:2], dones[:2]))


def test_header_exports_and_signatures():
    txt = open(os.path.join(ROOT, "include", "ballenv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+be_cnn_grad\s*\(\s*be_ctx\*\s*ctx,\s*const uint8_t\*\s*images,\s*const uint8_t\*\s*quadrants,\s*"
                     r"const uint8_t\*\s*actions,\s*const float\*\s*coef,\s*const uint8_t\*\s*valid,\s*int64_t\s+rows,\s*"
                     r"double\s+scale,\s*const be_cnn_weights\*\s*weights,\s*int32_t\s+num_actions,\s*void\*\s*workspace,\s*"
                     r"int64_t\s+workspace_bytes,\s*const be_cnn_grads\*\s*grads,\s*void\*\s*stream\s*\)\s*;", code)
    assert re.search(r"int64_t\s+be_cnn_grad_workspace_bytes\s*\(\s*be_ctx\*\s*ctx,\s*int32_t\s+num_actions\s*\)\s*;", code)
    assert re.search(r"int\s+be_observe_quadrant\s*\(\s*be_ctx\*\s*ctx,\s*const be_state\*\s*st,\s*uint8_t\*\s*out,\s*"
                     r"void\*\s*stream\s*\)\s*;", code)
    body = re.search(r"typedef struct be_cnn_grads \{(.*?)\} be_cnn_grads;", code, flags=re.S).group(1)
    fields = re.findall(r"\*\s*([a-z0-9_]+)", body)
    assert fields == [f[0] for f in _abi.BeCnnGrads._fields_]
    assert fields[:14] == [k.replace(".", "_") for k in _abi.CNN_PARAMS] and fields[14:] == ["losses", "probs"]
    assert list(_abi.CNN_PARAMS) == [k for k, _ in PixelPolicy().named_parameters()] == list(R.PARAMS)
    assert "ball_cnn_reinforce.py:98-117" in txt
    L = _abi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("be_cnn_grad", "be_cnn_grad_workspace_bytes", "be_observe_quadrant"):
        assert name in _abi.EXPORTS and hasattr(L, name) and re.search(rf"\bT {name}\b", out)
    assert L.be_cnn_grad.restype is C.c_int and len(L.be_cnn_grad.argtypes) == 14
    import gym_ballenv_amd as gb
    for name in ("PixelGrad", "pixel_reinforce_losses", "pixel_reinforce_update"):
        assert name in gb.__all__ and getattr(gb, name) is not None
    assert L.be_abi_version() == _abi.ABI_VERSION == 7        # additive: no ABI bump


def test_null_context_is_rejected_before_any_device_work():
    L = _abi.lib()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    assert L.be_cnn_grad_workspace_bytes(None, 9) == _abi.BE_E_INVALID
    assert b"ctx is NULL" in L.be_last_error(None)
    w, g = _abi.BeCnnWeights(), _abi.BeCnnGrads()
    assert L.be_cnn_grad(None, p, p, p, None, None, 1, 1.0, C.byref(w), 9, p, 64, C.byref(g), None) == _abi.BE_E_INVALID
    assert b"ctx is NULL" in L.be_last_error(None)
    assert L.be_observe_quadrant(None, C.byref(_abi.BeState()), p, None) == _abi.BE_E_INVALID
    assert b"ctx is NULL" in L.be_last_error(None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_layout_and_argument_checks_asan_ubsan(tmp_path):
    exe = str(tmp_path / "cnn_grad_host_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gym-ballenv_amd", "csrc"),
           os.path.join(ROOT, "tests", "cnn_grad_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cnn_grad_host: OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    layout = dict(zip(*[iter(next(line for line in r.stdout.splitlines() if line.startswith("layout ")).split()[1:])] * 2))
    assert (int(layout["tile"]), int(layout["waves"]), int(layout["max_slots"])) == (GRAD_TILE, GRAD_WAVES, GRAD_MAX_SLOTS)
    assert int(layout["lds"]) <= 160 * 1024
    assert int(layout["outputs"]) == sum(p.numel() for p in PixelPolicy().parameters())
    # cnn_grad_host.h includes nothing of HIP: ballenv.h, its sibling cnn_host.h (the network's shape) and the
    # standard headers
    src = open(os.path.join(ROOT, "gym-ballenv_amd", "csrc", "cnn_grad_host.h")).read()
    assert set(re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)) == {"stdint.h", "ballenv.h", "cnn_host.h"}
