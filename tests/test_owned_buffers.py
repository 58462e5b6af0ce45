"""The engine's scoped owners of device memory, pinned memory, events and streams (csrc/dev_owned.h) and the pool's
buffer set (csrc/pool.h), run against a fake HIP runtime: tests/owned_fake_hip.cpp is built with the host compiler
alone, without the HIP runtime library, so this needs no GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_owners_and_pool_against_a_fake_runtime(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    rocm = os.environ.get("ROCM", "/opt/rocm")
    if shutil.which(cxx) is None:
        pytest.fail(f"no host compiler ({cxx})")
    exe = str(tmp_path / "owned_fake_hip")
    cmd = [cxx, "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include",
           os.path.join(HERE, "owned_fake_hip.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-4000:]
    assert "owned buffers ok" in ran.stdout
