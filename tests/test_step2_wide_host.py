"""be_step's rule for step2_kernel's wide-row-load instance (behost::step2_wide in csrc/host_logic.h:
whole waves, 16-byte aligned obstacle arrays, the BALLENV_STEP2_WIDE override) -- compiled by the host
C++ compiler alone into the stand-alone tests/step2_wide_host_main.cpp, under AddressSanitizer +
UndefinedBehaviorSanitizer, and run.  No GPU and no HIP runtime."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_step2_wide_rule_asan_ubsan_clean(tmp_path):
    exe = str(tmp_path / "step2_wide_host_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gym-ballenv_amd", "csrc"),
           os.path.join(ROOT, "tests", "step2_wide_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "step2_wide_host: OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_accessor_is_declared_bound_and_null_safe():
    from gym_ballenv_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "ballenv.h")).read()
    assert re.search(r"\bint32_t be_step_instance\(const be_ctx\* ctx\);", hdr)
    assert "be_step_instance" in _abi.EXPORTS
    L = _abi.lib()
    assert len(L.be_step_instance.argtypes) == 1
    assert L.be_step_instance(None) == 0
    assert L.be_abi_version() == _abi.ABI_VERSION == 7        # additive: no ABI bump
