"""k_encode_prune's unrolled screening loop, on the host.

The screening pass runs trips of CWQ_SHARE_UNROLL copies of its body with no
exit inside a trip, while every lane is active and the pool holds the rows that
a trip's refills can take at most, and hands out the rest in a one-copy loop
that tests the active mask at its end; a lane turns inactive in a pool refill
only (csrc/cwq_kernels.hip; cwq_refill.h unroll_due, unroll_trip_rows).
tests/native/unroll_sim.cpp replays that control flow together with the
descending hand-out and the parked completion, with rows that drop at a random
unit and rows that reach the end, for unrolls of 1, 2, 4 and 8 copies, looks
for parked rows every 4th and every 8th iteration, with and without parking,
G in {2, 8, 16} and shares of 0, 1, 16, 63, 64, 65, 128, 256, 1,024, 4,096,
4,097, 5,000 and 16,384 rows, half of them ending at Philox block 2^32:

  * every row is started exactly once, on a block below 2^32;
  * every row that reaches the end is seen by the keep step exactly once, with
    all its units and nothing else summed, before the wave leaves; no parked
    row waits longer than the look mask;
  * inside an unrolled trip every refill's rows are in range and every lane
    stays active;
  * no copy runs without an active lane: the wave leaves behind the refill in
    which its last lane turns inactive, and a wave without a row runs no copy;
  * the share falls on every 8th iteration and the look on every 4th or 8th,
    counted over both loops.

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
    return tmp_path_factory.mktemp("unroll_plan")


def test_unrolled_loop_hands_out_and_keeps_once(tmp):
    out = _build_and_run(tmp, "unroll_sim", ["-O2"])
    assert out[-2:] == ["ok", ""], out[-5:]
    assert not [ln for ln in out if ln.startswith("FAIL")]


def test_unrolled_loop_under_sanitizers(tmp):
    out = _build_and_run(tmp, "unroll_sim-san",
                         ["-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined"])
    assert out[-2:] == ["ok", ""], out[-5:]
