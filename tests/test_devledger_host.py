"""CPU test of the device-resource ledger (csrc/devledger.h; DESIGN.md: "Device resources balance"): the header holds
nothing of the HIP runtime, so tests/native/devledger_check.cpp builds with g++ alone and drives it with made-up pointers:
note and forget, a free of null or of an unknown pointer, a pointer released by its scope stays live, the one-shot refusal
(arm, fire once, disarm, what `still armed` reports), and eight threads that note and forget 10 000 pointers each and end
at zero live with exactly one refusal between them.  The GPU side is tests/test_gpu_devmem.py."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "devledger_check.cpp")
HEADER = os.path.join(HERE, os.pardir, "bayesian-inference_amd", "csrc", "devledger.h")


def _gxx():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    return gxx


def test_ledger_header_is_hip_free():
    """the bookkeeping must build and be tested without a GPU toolchain: no HIP header, type or call in it"""
    code = "\n".join(ln.split("//")[0] for ln in open(HEADER).read().splitlines())
    assert not re.search(r"\bhip[A-Z_]\w*|hip_runtime|__global__|__device__", code)
    assert "#include <mutex>" in code


def test_ledger_check(tmp_path):
    exe = tmp_path / "devledger_check"
    subprocess.run([_gxx(), "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", SRC, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    m = re.search(r"checks (\d+) failures (\d+)", run.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) >= 50
