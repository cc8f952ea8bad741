"""How k_encode_prune hands a wave's rows to its lanes, on the host.

csrc/cwq_refill.h defines the static region S(R) of a share of R rows and where
the dynamic pool starts; tests/native/refill_sim.cpp replays the loop's
hand-out with random finishing lanes for R in {0, 1, 63, 64, 65, 127, 128, 129,
192, 255, 256, 1000, 16384} (and one share of 2^24 Philox blocks) and checks
that every row is started exactly once, by its own lane while it is a static
row, that ng stays within its bound and that no lane is out of range on the
path that skips the range test.  Here it is compiled and run once, and the S(R)
it prints is compared with the rule written out in Python.

The shapes of tests/test_prune_refill_gpu.py are checked too: which instance of
the kernel each runs and the share R of its waves.
"""
import os
import shutil
import subprocess

import pytest

import prune_refill_shapes as R
from test_encode_plan import EVAL, UNIFORM_PRUNED, mc, plan  # noqa: F401  (mc: a fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARES = (0, 1, 63, 64, 65, 127, 128, 129, 192, 255, 256, 1000, 16384)


def static_rows(r):
    """S(R): the largest multiple of 64 not above 7 R / 8; 0 below 128 rows."""
    return 0 if r < 128 else (7 * r // 8) // 64 * 64


@pytest.fixture(scope="module")
def sim_output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the refill simulation needs a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("refill") / "refill_sim")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-o", exe,
                           os.path.join(REPO, "tests", "native", "refill_sim.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout.split("\n")


def test_every_row_started_once(sim_output):
    assert sim_output[-2:] == ["ok", ""], sim_output[-5:]
    assert not [ln for ln in sim_output if ln.startswith("FAIL")]


def test_static_rows(sim_output):
    rows = [tuple(int(x) for x in ln.split()) for ln in sim_output[:len(SHARES)]]
    assert tuple(r for r, _, _ in rows) == SHARES
    for r, s, pool in rows:
        assert s == static_rows(r), (r, s)
        assert pool == max(s, 64), (r, s, pool)
    assert [static_rows(r) for r in (64, 128, 256, 1024, 16384)] == [0, 64, 192, 896, 14336]


@pytest.mark.parametrize("shape", sorted(set(R.ALL)))
def test_shape_takes_uniform_pruned(mc, shape):
    d, bits, nb, n_steps = shape
    for prune in (1, 2):
        assert plan(mc, csr=False, ud=d, bits=bits, prune=prune, nb=nb, n_steps=n_steps) == \
            (UNIFORM_PRUNED, False, False, 1)
    assert plan(mc, csr=False, ud=d, bits=bits, prune=0, nb=nb, n_steps=n_steps)[0] == EVAL


def test_shares():
    """The wave shares the GPU shapes are chosen for: a quarter of a tile."""
    got = {bits: R.wave_share(R.MANY, bits) for bits in (8, 9, 10, 12)}
    assert got == {8: [64], 9: [128], 10: [256], 12: [1024]}
    assert [static_rows(r[0]) for r in got.values()] == [0, 64, 192, 896]
    # INTER: tiles of 256 candidates (S = 0) ...
    for d, bits, nb, _ in R.INTER[:2]:
        assert R.P.tiling(nb, 1 << bits) == ((1 << bits) // 256, 256)
        assert R.wave_share(nb, bits) == [64]
    # ... and 64 blocks at 18 bits: 256 tiles of 1,024 per block, the last ones
    # cut in four (launch_prune_t's tail tiles): shares of 256 and of 64 rows
    d, bits, nb, _ = R.INTER[2]
    assert R.P.tiling(nb, 1 << bits) == (256, 1024)
    assert R.wave_share(nb, bits) == [256, 64]
