"""CPU: be_mlp_rollout's host side -- the declarations and ctypes signatures, the rejection that needs no
device, the instance rule and the argument checks of csrc/host_logic.h (a stand-alone C++ program under
AddressSanitizer + UndefinedBehaviorSanitizer, tests/mlp_rollout_host_main.cpp), and the index arithmetic of
mlp_rollout_kernel's wave slice restated in numpy.  No GPU and no HIP runtime."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gym_ballenv_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")


def test_header_exports_and_signatures():
    txt = open(os.path.join(ROOT, "include", "ballenv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+be_mlp_rollout\s*\(\s*be_mlp\*\s*mlp,\s*const be_state\*\s*st,\s*uint8_t\*\s*obs_last,\s*"
                     r"uint8_t\*\s*blocks_out,\s*int32_t\s+steps,\s*const be_out\*\s*out,\s*const be_act_out\*\s*act,\s*"
                     r"uint64_t\s+seed,\s*void\*\s*stream\s*\)\s*;", code)
    assert re.search(r"const char\*\s*be_mlp_rollout_kernel\s*\(\s*const be_mlp\*\s*mlp\s*\)\s*;", code)
    assert re.search(r"#define\s+BE_ABI_VERSION\s+7\b", txt)
    assert "ball_env_reinforce.py:309-336" in txt          # the entry's comment cites the episode loop
    L = _abi.lib()
    assert L.be_abi_version() == 7 == _abi.ABI_VERSION
    for name in ("be_mlp_rollout", "be_mlp_rollout_kernel"):
        assert name in _abi.EXPORTS and hasattr(L, name)
    f = L.be_mlp_rollout
    assert f.restype is C.c_int and len(f.argtypes) == 9
    assert f.argtypes[4] is C.c_int32 and f.argtypes[7] is C.c_uint64
    assert f.argtypes[1]._type_ is _abi.BeState and f.argtypes[5]._type_ is _abi.BeOut and f.argtypes[6]._type_ is _abi.BeActOut
    assert L.be_mlp_rollout_kernel.restype is C.c_char_p and len(L.be_mlp_rollout_kernel.argtypes) == 1


def test_null_handle_is_rejected_before_any_device_work():
    L = _abi.lib()
    st, out, act = _abi.BeState(), _abi.BeOut(), _abi.BeActOut()
    assert L.be_mlp_rollout(None, C.byref(st), None, None, 4, C.byref(out), C.byref(act), 1, None) == _abi.BE_E_INVALID
    assert b"be_mlp_rollout: mlp is NULL" in L.be_last_error(None)
    assert L.be_mlp_rollout_kernel(None) is None


# (N, compute units, layers) -> waves per workgroup.  The rule: the largest NW of 8, 4, 2 with
# N >= 32 NW CUs (every compute unit gets a full workgroup), else 1; nothing to run: 0.
WAVES = [
    (0, 256, 3, 0), (1, 256, 3, 1), (1, 256, 2, 1), (31, 256, 3, 1), (32, 1, 3, 1), (63, 1, 3, 1),
    (512, 256, 3, 1), (4096, 256, 3, 1), (32 * 256, 256, 3, 1), (32 * 256, 256, 2, 1),             # N <= 32 CUs: 1
    (64 * 256 - 1, 256, 3, 1), (64 * 256, 256, 3, 2), (16384, 256, 2, 2), (128 * 256 - 1, 256, 3, 2),
    (128 * 256, 256, 3, 4), (256 * 256 - 1, 256, 3, 4),
    (256 * 256, 256, 3, 8), (65536, 256, 2, 8), (1 << 20, 256, 3, 8), (1 << 29, 256, 3, 8),         # 32 * 8 * CUs up: 8
    (64, 1, 3, 2), (128, 1, 3, 4), (255, 1, 3, 4), (256, 1, 3, 8),
    (65536, 304, 3, 4), (32 * 8 * 304, 304, 3, 8), (32 * 8 * 304 - 1, 304, 2, 4), (4096, 64, 3, 2),
    (4096, 0, 3, 0), (4096, 256, 4, 0), (-5, 256, 3, 0),
]


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_instance_rule_and_argument_checks_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mlp_rollout_host_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gym-ballenv_amd", "csrc"),
           os.path.join(ROOT, "tests", "mlp_rollout_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    args = [f"{n}:{cus}:{layers}" for n, cus, layers, _ in WAVES]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "mlp_rollout_host: OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = [tuple(int(v) for v in m.groups()) for m in re.finditer(r"waves (-?\d+) (\d+) (\d+) -> (\d+)", r.stdout)]
    assert got == WAVES
    for n, cus, layers, nw in WAVES:        # what the rule promises, checked on the table itself
        if nw > 1:
            assert n // (32 * nw) >= cus            # every compute unit gets a (full) workgroup
        if nw in (1, 2, 4):
            assert n < 32 * 2 * nw * cus            # and no larger instance would


def test_wave_slice_index_arithmetic():
    """mlp_rollout_kernel's slice: env r of the wave keeps its 29 counts in 8 packed words at a 32-byte
    stride (blocks_core.h: byte b of the row in byte b & 3 of word b >> 2).  The copy to blocks_out reads
    byte b of the wave's run from slice byte (b // 29) * 32 + b % 29; lane (l15, l4) of tile tt takes
    x[k] = byte l4 of word k of row 16 tt + l15, which is input 4 k + l4 of that env (inputs 29..31: zero)."""
    rng = np.random.default_rng(5)
    for nrows in (1, 15, 16, 17, 32):
        rows = rng.integers(0, 20, (32, 29)).astype(np.uint8)
        words = np.zeros((32, 8), np.uint32)
        for b in range(29):
            words[:, b >> 2] |= rows[:, b].astype(np.uint32) << (8 * (b & 3))
        slice_bytes = words.view(np.uint8).reshape(-1)           # little endian, as the GPU's
        assert slice_bytes.size == 32 * 32
        nbytes = nrows * 29
        out = np.array([slice_bytes[(b // 29) * 32 + b % 29] for b in range(nbytes)], np.uint8)
        assert np.array_equal(out, rows[:nrows].reshape(-1))
        for tt in range(2):
            for lane in range(64):
                l15, l4 = lane & 15, lane >> 4
                x = [(int(words[16 * tt + l15, k]) >> (8 * l4)) & 0xFF for k in range(8)]
                want = [int(rows[16 * tt + l15, 4 * k + l4]) if 4 * k + l4 < 29 else 0 for k in range(8)]
                assert x == want
    # the slice's words: counts, logits at a 17-float stride, wave_resets' scratch (3 envs per pass, 4 rows + 8),
    # a pass's new obstacles -- and the launch's bytes with the 3- and 2-layer images
    slice_words = 32 * 8 + 32 * 17 + 3 * (4 + 8) + 64
    assert slice_words % 4 == 0 and slice_words * 4 == 3600
    assert 91264 + 8 * slice_words * 4 <= 160 * 1024 and 25216 + 8 * slice_words * 4 <= 160 * 1024
