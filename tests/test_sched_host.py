"""CPU test of the host-built tables of the triangular GEMM and the compacted half-step (csrc/sched_host.h; DESIGN.md
4.37): tests/native/sched_host_check.cpp builds the tables of every live block count of a sweep of shapes and forms and
checks that each row's items cover every (PC, row block, 64-column cell) exactly once, that each row of the cross-kernel's
map holds every (PC, row chunk, column block) exactly once, that the full row is the whole batch's own schedule, and that
the shapes beyond the map's limits are declined.  A dropped item (a stale partial sum) and a doubled one (time only, the
same bits) both fail here."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sched_host_check.cpp")


def _counts(out):
    vals = {}
    for ln in out.splitlines():
        if ln.startswith(("shapes ", "rows_form0 ", "failures ")):
            vals.update({k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)", ln)})
    return vals


def _gxx():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    return gxx


def test_every_table_of_the_sweep(tmp_path):
    exe = tmp_path / "sched_host_check"
    subprocess.run([_gxx(), "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    v = _counts(run.stdout)
    assert v["failures"] == 0
    assert v["accepted"] > 1500 and v["declined"] > 0 and v["rows"] > 50000
    # every form and both guarded fall-backs were taken by some row of the sweep
    for key in ("rows_form0", "rows_form1", "rows_form2", "fell_2_to_1", "fell_to_0"):
        assert v[key] > 0, (key, v)


def test_reduced_sweep_under_the_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan (a stand-alone binary: nothing preloaded) on every 12th shape:
    the form-2 map is written through a computed index, the tables through computed strides."""
    exe = tmp_path / "sched_host_check_san"
    cc = subprocess.run([_gxx(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         SRC, "-o", str(exe)], capture_output=True, text=True)
    if cc.returncode != 0:
        if re.search(r"cannot find|libasan|libubsan|unrecognized.*sanitize", cc.stderr):
            pytest.skip("no sanitizer runtime for g++ here")
        raise AssertionError(cc.stderr[-4000:])
    run = subprocess.run([str(exe), "12"], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    v = _counts(run.stdout)
    assert v["failures"] == 0 and v["shapes"] >= 150
