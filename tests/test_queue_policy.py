"""The hardware-queue policy (bbs_sign_amd/csrc/queue_policy.hpp: which stream gets a hardware queue of its own, which one
comes from the runtime's pool, which one is refused) is a HIP-free header: tests/cpp/queue_policy.cpp walks it on the CPU
-- pools {1, 4, 8, 14, 20, 32} x budgets {1, 8, 25, 64} x settings {automatic, 0, 1, 12, 16} x streams already made -- and
asserts that dedicated + min(pool, pooled) never exceeds the budget, that explicit settings give what they gave before,
that the automatic setting is off from pool 20 and never wishes for more than 16.  Built as a plain executable, once as it
is and once with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_queue_policy(sanitize, tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "queue_policy.cpp")
    exe = str(tmp_path / "queue_policy")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:]
