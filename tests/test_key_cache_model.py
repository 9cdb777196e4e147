"""The bookkeeping of the job-local key cache (bbs_sign_amd/csrc/key_cache.hpp: string -> slot, free list, least-recently-used
order, pins, counters, rollback of a failed upload) is a HIP-free header: tests/cpp/key_cache_model.cpp drives it alone with
a few thousand random operations against a naive model inside the same program.  Built as a plain executable with the
address and undefined-behaviour sanitizers; needs no GPU and no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_cache_model_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "key_cache_model.cpp")
    exe = str(tmp_path / "key_cache_model")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           src, "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:]
