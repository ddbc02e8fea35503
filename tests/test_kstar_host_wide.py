"""CPU test of the cross-kernel's host-built operands (csrc/kstar_host.h) for 9 to 16 parameters: the number of MFMA
k-steps is ceil((d + 1) / 4) and the augmented product still recovers the squared scaled distance of sklearn's ARD
kernels (ref: emulation.py:497 -> skl kernels.py:1553-1582, 1708-1781).  The harness is the one of test_kstar_host.py,
built here with AddressSanitizer as well, so that a centre array or augmented row too short for d is an error."""
import math
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / ("kstar_host_check_asan" if sanitize else "kstar_host_check")
    flags = ["-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([gxx, *flags, "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "native", "kstar_host_check.cpp"),
                    "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan"])
@pytest.mark.parametrize("N,d,k", [(203, 9, 3), (130, 12, 2), (64, 15, 2), (150, 16, 3)])
def test_wide_augmented_product_recovers_the_scaled_distance(tmp_path, N, d, k, sanitize):
    exe = _build(tmp_path, sanitize)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([str(exe), str(N), str(d), str(k)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("kind")]
    assert len(lines) == 2
    for ln in lines:
        m = re.match(r"kind (\d) ksteps (\d) worst_rel_r2 (\S+) at_training_point (\S+) layout (\w+)", ln)
        assert m, ln
        assert int(m.group(2)) == math.ceil((d + 1) / 4)
        assert m.group(5) == "ok", ln
        # error model of test_kstar_host.py: ~ d (range / 2 ls)^2 eps, so its 1e-11 (stated for d <= 8) widened by d / 8
        bound = 1e-11 * d / 8
        assert float(m.group(3)) < bound, ln
        assert float(m.group(4)) < bound, ln
