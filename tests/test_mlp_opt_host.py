"""be_mlp_opt without a GPU: the pinned SGD step (tests/mlp_opt_ref.py) against torch.optim.SGD, the
index inversion of the fused re-pack against mlp_pack_kernel's forward map, and the entry's declaration,
export and NULL-mlp error."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from a2c_adam_ref import fresh_state
from mlp_opt_ref import image_index, layout, names, pack_forward, sgd_step_ref, shapes

from gym_ballenv_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"affine1.weight": (128, 29), "affine3.weight": (9, 128), "scalar": (1,)}
LR = 1e-2


def _grads(rng, scale):
    out = {}
    for k, s in SHAPES.items():
        g = (rng.standard_normal(s) * scale).astype(np.float32)
        g[rng.random(s) < 0.05] = 0.0            # 5 % exact zeros
        out[k] = g
    return out


def _torch_sgd(w0, grads, dtype):
    ps = [torch.nn.Parameter(torch.from_numpy(w0[k].copy()).to(dtype)) for k in SHAPES]
    opt = torch.optim.SGD(ps, lr=LR)
    for g in grads:
        for p, k in zip(ps, SHAPES):
            p.grad = torch.from_numpy(g[k].copy()).to(dtype)
        opt.step()
    return {k: p.detach().double().numpy() for p, k in zip(ps, SHAPES)}


@pytest.mark.parametrize("steps", [1, 5, 50])
@pytest.mark.parametrize("scale", [1e-4, 1.0, 100.0])
def test_restatement_against_torch_sgd(steps, scale):
    """Per tensor err = max|w - w64| / max|w64 - w0| with w64 torch's SGD on f64 copies; the pinned
    arithmetic may be at most 4x torch's own f32 SGD + 1e-6 away (the rule of tests/test_a2c_adam_host.py).
    torch's f32 SGD is the yardstick of that rule, so it is first checked to be a usable one: finite, and
    within 5 % of the distance moved (at the 1e-4 scale a step of lr * g ~ 1e-6 is a few hundred f32 ulps of
    a weight ~ 0.1, so half an ulp of rounding per step is some 1e-3 of the move; it shrinks with the scale)."""
    rng = np.random.default_rng(1000 * steps + int(np.log10(scale)) + 7)
    w0 = {k: (rng.standard_normal(s) * 0.1).astype(np.float32) for k, s in SHAPES.items()}
    grads = [_grads(rng, scale) for _ in range(steps)]
    w64 = _torch_sgd(w0, grads, torch.float64)
    w32 = _torch_sgd(w0, grads, torch.float32)
    w = {k: x.copy() for k, x in w0.items()}
    state = fresh_state(LR)
    for g in grads:
        sgd_step_ref(w, g, state)
    assert state[0] == steps and state[1] == 1.0 and state[2] == 1.0 and state[3] == LR
    for k in SHAPES:
        moved = np.abs(w64[k] - w0[k].astype(np.float64)).max()
        assert moved > 0
        err_ref = np.abs(w[k].astype(np.float64) - w64[k]).max() / moved
        err_t32 = np.abs(w32[k] - w64[k]).max() / moved
        print(f"steps={steps} scale={scale:g} {k}: err_restatement={err_ref:.3e} err_torch_f32={err_t32:.3e}")
        assert np.isfinite(err_t32) and err_t32 < 0.05, (k, err_t32)    # torch's f32 run tracks its f64 run
        assert err_ref <= 4 * err_t32 + 1e-6, (k, err_ref, err_t32)


@pytest.mark.parametrize("layers,h1,h2,A", [(3, 128, 128, 9), (3, 100, 37, 5), (2, 128, 0, 9), (2, 16, 0, 1),
                                            (3, 1, 1, 15), (3, 17, 128, 15)])
def test_index_inversion_is_the_pack_kernels_map(layers, h1, h2, A):
    """Every non-pad image index is hit exactly once, by the element the pack kernel reads there, and no
    pad index is hit; the 16 hb entries are the kernel's last 16 threads'."""
    fwd = pack_forward(layers, h1, h2, A)
    L, inv, shp = layout(layers), image_index(layers, h1, h2, A), shapes(layers, h1, h2, A)
    assert len(fwd) == L["total"] and list(inv) == names(layers)
    hits = np.zeros(L["total"], dtype=np.int64)
    for k, dst in inv.items():
        assert dst.shape == (int(np.prod(shp[k])),)
        assert dst.min() >= 0 and dst.max() < L["hb"]
        np.add.at(hits, dst, 1)
        for j in (0, dst.size // 2, dst.size - 1):
            assert fwd[dst[j]] == (k, j)
        assert all(fwd[d] == (k, j) for j, d in enumerate(dst))
    nonpad = np.array([s is not None and s[0] != "hb" for s in fwd])
    assert np.array_equal(hits, nonpad.astype(np.int64))
    assert [fwd[L["hb"] + m] for m in range(16)] == [("hb", m) for m in range(16)]
    assert int(nonpad.sum()) == sum(int(np.prod(s)) for s in shp.values())


def test_library_declares_and_exports_the_entry():
    hdr = open(os.path.join(ROOT, "include", "ballenv.h")).read()
    assert re.search(r"\bint be_mlp_opt\(be_mlp\* mlp, int32_t kind,", hdr)
    assert "typedef struct be_mlp_tensors" in hdr
    assert re.search(r"#define BE_MLP_OPT_ADAM\s+0\b", hdr) and re.search(r"#define BE_MLP_OPT_SGD\s+1\b", hdr)
    assert (_abi.MLP_OPT_ADAM, _abi.MLP_OPT_SGD) == (0, 1)
    assert "be_mlp_opt" in _abi.EXPORTS
    assert C.sizeof(_abi.BeMlpTensors) == 6 * C.sizeof(C.c_void_p)
    L = _abi.lib()
    assert hasattr(L, "be_mlp_opt") and L.be_mlp_opt.argtypes is not None and len(L.be_mlp_opt.argtypes) == 14
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT be_mlp_opt\b", out)
    assert L.be_abi_version() == _abi.ABI_VERSION == 7


def test_package_exports_the_classes():
    import gym_ballenv_amd as gb
    for name in ("HipBlockOptim", "BlockTrainer", "SupervisedTrainer"):
        assert name in gb.__all__ and getattr(gb, name).__name__ == name


def test_null_mlp_is_invalid():
    L = _abi.lib()
    t = _abi.BeMlpTensors()
    for kind in (_abi.MLP_OPT_ADAM, _abi.MLP_OPT_SGD):
        rc = L.be_mlp_opt(None, kind, C.byref(t), C.byref(t), C.byref(t), C.byref(t), None, 0.9, 0.999, 1e-8, None,
                          None, 0, None)
        assert rc == _abi.BE_E_INVALID
        assert b"mlp is NULL" in L.be_last_error(None)
