"""CPU: the pixel policy's host side -- torch_pixel_forward's two BatchNorm modes against PixelPolicy
itself in float64, the reference's trained weights from the two committed fixtures, the declarations and
exports of be_cnn_*, the rejection that needs no device, and csrc/cnn_host.h (the packed image's index
function, the argument checks) in a stand-alone C++ program under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/cnn_host_main.cpp).  No GPU and no HIP runtime."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import helpers
from gym_ballenv_amd import _abi
from gym_ballenv_amd.pixel_policy import (TILE, WAVES, HipPixelPolicy, PixelPolicy, PixelRollout,  # noqa: F401
                                          reference_pixel_weights, torch_pixel_forward, torch_pixel_select_action)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")


def random_policy(seed, A=9):
    torch.manual_seed(seed)
    pol = PixelPolicy(A)
    with torch.no_grad():
        for bn in (pol.bn1, pol.bn2, pol.bn3):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.uniform_(-0.3, 0.3)
            bn.running_var.uniform_(0.2, 2.0)
    return pol


def test_sample_mode_is_the_train_mode_forward_of_one_image():
    pol = random_policy(0).double()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(5, 3, 40, 40, generator=g, dtype=torch.float64)
    y = torch.eye(4, dtype=torch.float64)[[0, 1, 2, 3, 1]]
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    with torch.no_grad():
        got = torch_pixel_forward(pol, x, y, "sample")
    for k, v in pol.state_dict().items():
        assert torch.equal(v, before[k]), k                       # no buffer is updated
    pol.train()
    with torch.no_grad():
        want = torch.cat([pol(x[i:i + 1], y[i:i + 1]) for i in range(5)])
    assert got.shape == (5, 9) and (got - want).abs().max().item() <= 1e-12
    with torch.no_grad():
        mixed = pol(x, y)                                          # batch statistics across the images: not the same
    assert (mixed - want).abs().max().item() > 1e-6


def test_running_mode_is_the_eval_mode_forward():
    pol = random_policy(2).double().eval()
    g = torch.Generator().manual_seed(3)
    x = torch.rand(5, 3, 40, 40, generator=g, dtype=torch.float64)
    y = torch.eye(4, dtype=torch.float64)[[3, 2, 1, 0, 0]]
    with torch.no_grad():
        got, want = torch_pixel_forward(pol, x, y, "running"), pol(x, y)
    assert (got - want).abs().max().item() <= 1e-12
    with pytest.raises(ValueError):
        torch_pixel_forward(pol, x, y, "batch")


def test_forward_is_differentiable():
    pol = random_policy(4)
    x = torch.rand(3, 3, 40, 40)
    y = torch.eye(4)[[0, 1, 2]]
    torch_pixel_forward(pol, x, y, "sample")[:, 0].log().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in pol.parameters())


def test_select_action_draws_by_inverse_cdf():
    pol = random_policy(5)
    img = torch.from_numpy(helpers.load("pixels")["images"])
    q = torch.arange(16) % 4
    u = torch.linspace(0.0, 0.999, 16)
    with torch.no_grad():
        a, lp, pr = torch_pixel_select_action(pol, img, q, u, "sample")
        want = torch_pixel_forward(pol, img.float() / 255.0, torch.eye(4)[q], "sample")
    assert torch.equal(pr, want) and a.dtype == torch.int64
    cdf = pr.cumsum(-1)
    for e in range(16):
        assert int(a[e]) == min(int((cdf[e] <= u[e]).sum()), 8)
        assert lp[e] == torch.log(pr[e, a[e]])


def test_reference_weights_load_strictly_and_give_probabilities_in_sample_mode():
    sd = reference_pixel_weights()
    pol = PixelPolicy()
    pol.load_state_dict(sd, strict=True)
    assert sum(v.numel() for k, v in sd.items() if v.dtype == torch.float32) == 1200 + 12800 + 25600 + 9 * 132 + 9 + 5 * 80
    sizes = [os.path.getsize(os.path.join(helpers.GOLDEN, n)) for n in ("pixel_policy_cnn.npz", "pixel_policy_cnn_conv3.npz")]
    largest_before = os.path.getsize(os.path.join(helpers.GOLDEN, "rollouts_default.npz"))
    assert max(sizes) < largest_before
    img = torch.from_numpy(helpers.load("pixels")["images"]).float() / 255.0
    y = torch.eye(4)[torch.arange(16) % 4]
    with torch.no_grad():
        pr = torch_pixel_forward(pol, img, y, "sample")
    assert torch.isfinite(pr).all() and pr.max().item() < 1.0 and pr.min().item() > 0.0
    assert torch.allclose(pr.sum(1), torch.ones(16), atol=1e-6)


def test_header_exports_and_signatures():
    txt = open(os.path.join(ROOT, "include", "ballenv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+be_cnn_act\s*\(\s*be_cnn\*\s*cnn,\s*const be_state\*\s*st,\s*const uint8_t\*\s*image,\s*"
                     r"const uint8_t\*\s*quadrant_in,\s*int32_t\s+norm,\s*const be_act_out\*\s*out,\s*uint64_t\s+seed,\s*"
                     r"void\*\s*stream\s*\)\s*;", code)
    assert re.search(r"int\s+be_cnn_load\s*\(\s*be_cnn\*\s*cnn,\s*const be_cnn_weights\*\s*w,\s*void\*\s*stream\s*\)\s*;", code)
    assert re.search(r"#define\s+BE_CNN_NORM_SAMPLE\s+0\b", txt) and re.search(r"#define\s+BE_CNN_NORM_RUNNING\s+1\b", txt)
    assert (_abi.CNN_NORM_SAMPLE, _abi.CNN_NORM_RUNNING) == (0, 1)
    body = re.search(r"typedef struct be_cnn_weights \{(.*?)\} be_cnn_weights;", code, flags=re.S).group(1)
    fields = re.findall(r"\*\s*([a-z0-9_]+)", body)
    assert fields == [k.replace(".", "_") for k in _abi.CNN_TENSORS] == [f[0] for f in _abi.BeCnnWeights._fields_]
    assert len(fields) == 20 and C.sizeof(_abi.BeCnnWeights) == 20 * C.sizeof(C.c_void_p)
    assert "ball_cnn_reinforce.py:60-83" in txt
    L = _abi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("be_cnn_create", "be_cnn_destroy", "be_cnn_load", "be_cnn_act", "be_cnn_bytes"):
        assert name in _abi.EXPORTS and hasattr(L, name) and re.search(rf"\bT {name}\b", out)
    f = L.be_cnn_act
    assert f.restype is C.c_int and len(f.argtypes) == 8 and f.argtypes[1]._type_ is _abi.BeState
    import gym_ballenv_amd as gb
    for name in ("HipPixelPolicy", "PixelRollout", "torch_pixel_forward", "torch_pixel_select_action",
                 "reference_pixel_weights"):
        assert name in gb.__all__ and getattr(gb, name) is not None
    assert L.be_cnn_bytes(None) == 0


def test_null_handles_are_rejected_before_any_device_work():
    L = _abi.lib()
    st = _abi.BeState()
    buf = (C.c_uint8 * 64)()
    out = _abi.BeActOut(C.addressof(buf), None, None, None)
    assert L.be_cnn_act(None, C.byref(st), C.addressof(buf), None, 0, C.byref(out), 0, None) == _abi.BE_E_INVALID
    assert b"cnn is NULL" in L.be_last_error(None)
    assert L.be_cnn_load(None, C.byref(_abi.BeCnnWeights()), None) == _abi.BE_E_INVALID
    assert b"cnn is NULL" in L.be_last_error(None)
    h = C.c_void_p()
    assert L.be_cnn_create(None, 9, C.byref(h)) == _abi.BE_E_INVALID and not h.value
    assert L.be_cnn_destroy(None) == _abi.BE_OK


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_pack_index_and_argument_checks_asan_ubsan(tmp_path):
    exe = str(tmp_path / "cnn_host_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gym-ballenv_amd", "csrc"),
           os.path.join(ROOT, "tests", "cnn_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cnn_host: OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    layout = dict(zip(*[iter(next(line for line in r.stdout.splitlines() if line.startswith("layout ")).split()[1:])] * 2))
    assert (int(layout["tile"]), int(layout["waves"])) == (TILE, WAVES)      # the Python side's mirror
    assert int(layout["total"]) * 4 == 168640 and int(layout["lds"]) <= 160 * 1024
