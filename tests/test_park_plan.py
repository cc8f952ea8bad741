"""k_encode_prune's parked completion, on the host.

In tiles of CWQ_PARK_MIN_ROWS rows or more the screening loop has no completion
test: a row that passes its last visit position walks on to a sentinel record
and waits there until the iteration that shares tau finds it
(csrc/cwq_kernels.hip, "Parked rows").  tests/native/park_sim.cpp replays that
control flow together with the descending hand-out of
tests/native/refill_desc_sim.cpp, with rows that drop at a random unit and rows
that reach the end, for G in {2, 4, 8, 16} and shares of 0, 1, 2, 63 .. 16,384
rows, with none, a few, half and all of the rows reaching the end:

  * every row is started exactly once;
  * every row that reaches the end is seen by the keep step exactly once, with
    all its units and nothing else summed; no other row is;
  * no lane is left parked when the loop ends, and none waits longer than 7
    iterations;
  * every drop is taken at the unit drawn for the row.

It is run once as built for speed and once built with the address and
undefined-behaviour sanitizers, as a program of its own.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the host checks need a C++ compiler"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, "-o", exe,
                           os.path.join(REPO, "tests", "native", name.split("-")[0] + ".cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout.split("\n")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("park_plan")


def test_parked_rows_are_kept_once(tmp):
    out = _build_and_run(tmp, "park_sim", ["-O2"])
    assert out[-2:] == ["ok", ""], out[-5:]
    assert not [ln for ln in out if ln.startswith("FAIL")]


def test_parked_rows_under_sanitizers(tmp):
    out = _build_and_run(tmp, "park_sim-san",
                         ["-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined"])
    assert out[-2:] == ["ok", ""], out[-5:]
