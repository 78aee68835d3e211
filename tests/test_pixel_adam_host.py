"""be_cnn_adam without a GPU: the index inversion of the fused re-pack (tests/cnn_adam_ref.py's numpy
image_index against a Python walk of the pack kernel's rule; csrc/cnn_host.h's cnn_pack_dest in a stand-alone
C++ program under AddressSanitizer + UndefinedBehaviorSanitizer, tests/cnn_adam_host_main.cpp), the entry's
declaration, export and NULL-cnn error, the package's exports, the constructor errors that need no device,
and the yardstick of the GPU overfit test: torch's own training run on its rows."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import cnn_adam_ref as R
from gym_ballenv_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")


@pytest.mark.parametrize("A", [1, 9, 15])
def test_index_inversion_is_the_pack_kernels_map(A):
    """Every image index that holds a parameter is hit exactly once, by the element the pack kernel reads there;
    no pad, -inf or running-statistics index is hit."""
    fwd, inv, shp = R.pack_forward(A), R.image_index(A), R.shapes(A)
    assert len(fwd) == R.TOTAL == 42160 and list(inv) == list(R.PARAMS) == list(_abi.CNN_PARAMS)
    hits = np.zeros(R.TOTAL, dtype=np.int64)
    for k, dst in inv.items():
        assert dst.shape == shp[k]
        flat = dst.reshape(-1)
        assert flat.min() >= 0 and flat.max() < R.TOTAL
        np.add.at(hits, flat, 1)
        assert all(fwd[d] == (k, j) for j, d in enumerate(flat)), k
    param = np.array([isinstance(s, tuple) and "running" not in s[0] for s in fwd])
    assert np.array_equal(hits, param.astype(np.int64))
    running = R.running_index()
    assert running.size == 2 * 80 and all("running" in fwd[i][0] for i in running) and not hits[running].any()
    assert int(param.sum()) == sum(int(np.prod(s)) for s in shp.values())
    assert sum(s == "neginf" for s in fwd) == 15 - A


def test_shapes_are_the_modules():
    from gym_ballenv_amd.pixel_policy import PixelPolicy
    for A in (1, 9, 15):
        assert {k: tuple(p.shape) for k, p in PixelPolicy(A).named_parameters()} == R.shapes(A)
        assert list(dict(PixelPolicy(A).named_parameters())) == list(_abi.CNN_PARAMS)      # torch.optim's order


def test_library_declares_and_exports_the_entry():
    hdr = open(os.path.join(ROOT, "include", "ballenv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint be_cnn_adam\(be_cnn\* cnn, const be_cnn_tensors\* params, const be_cnn_tensors\* grads,\s*"
                     r"const be_cnn_tensors\* exp_avg, const be_cnn_tensors\* exp_avg_sq, double\* state,\s*"
                     r"double beta1, double beta2, double eps,\s*"
                     r"const double\* losses, double\* loss_log, int32_t log_rows, void\* stream\);", code)
    body = re.search(r"typedef struct be_cnn_tensors \{(.*?)\} be_cnn_tensors;", code, flags=re.S).group(1)
    fields = re.findall(r"\*\s*([a-z0-9_]+)", body)
    assert fields == [k.replace(".", "_") for k in _abi.CNN_PARAMS] == [f[0] for f in _abi.BeCnnTensors._fields_]
    assert len(fields) == 14 and C.sizeof(_abi.BeCnnTensors) == 14 * C.sizeof(C.c_void_p)
    assert "be_cnn_adam before be_cnn_load" in hdr and "ball_cnn_reinforce.py:115" in hdr
    assert "be_cnn_adam" in _abi.EXPORTS
    L = _abi.lib()
    f = L.be_cnn_adam
    assert f.restype is C.c_int and len(f.argtypes) == 13
    assert all(f.argtypes[i]._type_ is _abi.BeCnnTensors for i in (1, 2, 3, 4))
    assert [f.argtypes[i] for i in (6, 7, 8)] == [C.c_double] * 3 and f.argtypes[11] is C.c_int32
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT be_cnn_adam\b", out)
    assert L.be_abi_version() == _abi.ABI_VERSION == 7


def test_null_cnn_is_invalid():
    L = _abi.lib()
    t = _abi.BeCnnTensors()
    rc = L.be_cnn_adam(None, C.byref(t), C.byref(t), C.byref(t), C.byref(t), None, 0.9, 0.999, 1e-8, None, None, 0, None)
    assert rc == _abi.BE_E_INVALID
    assert b"be_cnn_adam: cnn is NULL" in L.be_last_error(None)


def test_package_exports_the_classes():
    import gym_ballenv_amd as gb
    from gym_ballenv_amd.optim import HipOptim
    from gym_ballenv_amd.rollout import RolloutTrainer
    for name in ("HipPixelAdam", "PixelTrainer"):
        assert name in gb.__all__ and getattr(gb, name).__name__ == name
    opt = gb.HipPixelAdam
    assert issubclass(opt, HipOptim) and issubclass(gb.PixelTrainer, RolloutTrainer)
    assert (opt.KINDS, opt.LOSS_WIDTH, opt.SLOTS, opt.STRUCT) == ({"adam": ()}, 2, 14, _abi.BeCnnTensors)
    assert HipOptim.SLOTS == 6 and gb.HipAdam.SLOTS == 6 and gb.HipBlockOptim.SLOTS == 6
    for k in ("capture", "train", "losses", "close", "update"):           # inherited, not restated
        assert k not in vars(gb.PixelTrainer)


def test_constructor_errors_that_need_no_device():
    """A stand-in for the HipPixelPolicy on the CPU: these are raised before anything touches a device."""
    from gym_ballenv_amd.pixel_policy import HipPixelAdam, PixelPolicy
    hp = types.SimpleNamespace(env=types.SimpleNamespace(device=torch.device("cpu")), num_actions=9)
    pol = PixelPolicy(9)
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(lr=-1.0)):
        with pytest.raises(ValueError):
            HipPixelAdam(hp, pol, **kw)
    with pytest.raises(ValueError, match="eps > 0"):
        HipPixelAdam(hp, pol, eps=0.0)
    for bad in (PixelPolicy(4), PixelPolicy(9).double(), torch.nn.Linear(3, 2)):
        with pytest.raises(ValueError):
            HipPixelAdam(hp, bad)
    opt = HipPixelAdam(hp, pol, log_rows=3)                                # the defaults are the reference's
    assert (opt.lr, opt.betas, opt.eps) == (1e-3, (0.9, 0.999), 1e-8)
    assert list(opt.exp_avg) == list(_abi.CNN_PARAMS) and tuple(opt.loss_log.shape) == (3, 2)
    assert opt.state.tolist() == [0.0, 1.0, 1.0, 1e-3] and opt._pad == ()
    with pytest.raises(ValueError):
        opt.step()                                                         # no .grad yet
    sd = torch.optim.Adam(pol.parameters(), lr=1e-3, eps=0.0).state_dict()
    with pytest.raises(ValueError, match="eps > 0"):
        opt.load_state_dict(sd)


@pytest.mark.parametrize("seed", R.OVERFIT_SEEDS)
def test_torch_itself_overfits_the_fixed_rows(seed):
    """The yardstick of tests/test_gpu_pixel_adam.py's overfit test: on the same 8 rows, from the same policy,
    torch's own forward + Categorical.log_prob + optim.Adam(lr=1e-3) has a lower loss at step 10 than at step 1."""
    losses = R.torch_overfit_losses(seed)
    print(f"seed {seed}: " + " ".join(f"{x:.4f}" for x in losses))
    assert len(losses) == 10 and np.isfinite(losses).all() and losses[9] < losses[0]


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_pack_dest_and_argument_checks_asan_ubsan(tmp_path):
    exe = str(tmp_path / "cnn_adam_host_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gym-ballenv_amd", "csrc"),
           os.path.join(ROOT, "tests", "cnn_adam_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cnn_adam_host: OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    elems = {int(a): int(n) for a, n in (line.split()[1:] for line in r.stdout.splitlines() if line.startswith("elems "))}
    assert elems == {A: sum(int(np.prod(s)) for s in R.shapes(A).values()) for A in (1, 9, 15)}    # the kernel's threads
