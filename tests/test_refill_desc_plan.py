"""k_encode_prune's downward static rows and the folded Philox add, on the host.

tests/native/refill_desc_sim.cpp replays, in the kernel's 32-bit arithmetic and
with random finishing lanes, the hand-out in which a lane walks its static
rows from the last one down and the subtract's borrow tells that they are used
up (csrc/cwq_kernels.hip, CWQ_BORROW_REFILL), for the shares of
tests/test_refill_plan.py, R in {0, 1, 63, 64, 65, 127, 128, 129, 192, 255, 256,
1000, 16384}, with the wave at row 0 and at the end of a stream of 2^32 Philox
blocks.  It is run once as built for speed and once built with the address and
undefined-behaviour sanitizers, as a program of its own.

tests/native/philox_fold_check.cpp holds csrc/cwq_philox_lo.h to cwq_math.h's
philox10: M0 X + M0 g == M0 (X + g), and the Philox entry that takes round 0's
product, on 10^6 random triples and the edges.
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
    return tmp_path_factory.mktemp("refill_desc")


def test_every_row_started_once_going_down(tmp):
    out = _build_and_run(tmp, "refill_desc_sim", ["-O2"])
    assert out[-2:] == ["ok", ""], out[-5:]
    assert not [ln for ln in out if ln.startswith("FAIL")]


def test_hand_out_under_sanitizers(tmp):
    out = _build_and_run(tmp, "refill_desc_sim-san",
                         ["-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined"])
    assert out[-2:] == ["ok", ""], out[-5:]


def test_round0_product_and_entry(tmp):
    out = _build_and_run(tmp, "philox_fold_check", ["-O2"])
    assert out[-2:] == ["ok", ""], out[-5:]
