"""csrc/host_logic.h -- the host logic of libballenv.so that has no HIP in it (the autoreset pool's
bookkeeping, the checkpoint blob's layout, be_pool_entry's word order, be_out_at) -- compiled by the
host C++ compiler alone into the stand-alone tests/host_logic_main.cpp, under AddressSanitizer +
UndefinedBehaviorSanitizer (abort on the first report), and run.  No GPU and no HIP runtime."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_host_logic_asan_ubsan_clean(tmp_path):
    exe = str(tmp_path / "host_logic_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gym-ballenv_amd", "csrc"),
           os.path.join(ROOT, "tests", "host_logic_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host_logic: OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
