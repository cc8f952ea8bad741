"""CPU: backfitting's C ABI (0.12) is exported and bound, its host-side
validation answers before any launch, and its dispatch rules hold a table."""
import ctypes
import os
import subprocess

import pytest

from compression_without_quantization_amd import _lib
from encode_shapes import SMALL_PATH_SIZES

NAMES = ("cwq_greedy_backfit_workspace_size", "cwq_greedy_backfit")


def test_abi_version_and_symbols(cwqlib):
    assert _lib.ABI_VERSION >= 12 and cwqlib.cwq_version() == _lib.ABI_VERSION
    for name in NAMES:
        assert hasattr(cwqlib, name) and name in _lib.SIGNATURES, name
    import compression_without_quantization_amd as C
    for name in ("backfit_blocks", "encode_blocks_backfit", "code_grouped_greedy_sample_backfit"):
        assert callable(getattr(C, name)) and name in C.__all__, name
    assert C.backfit.MAX_SWEEPS == 16


def test_workspace_size(cwqlib):
    """The encoder's layout for ragged blocks, then n_steps rows of floats per
    dim and two words per block, each array rounded up to 256 bytes; monotone
    in every argument."""
    size = cwqlib.cwq_greedy_backfit_workspace_size
    up = lambda v: (v + 255) // 256 * 256
    for nb, D, longest, steps in [(18, 8711, 4095, 3), (300, 9600, 32, 4), (1, 4095, 4095, 30),
                                  (5000, 25000, 5, 2), (7, 100, 64, 1)]:
        enc = cwqlib.cwq_greedy_encode_workspace_size(nb, D, longest)
        assert size(nb, D, longest, steps) == up(enc) + up(4 * steps * D) + 2 * up(4 * nb)
        assert size(nb + 1, D, longest, steps) >= size(nb, D, longest, steps)
        assert size(nb, D + 1, longest, steps) >= size(nb, D, longest, steps)
        assert size(nb, D, longest + 1, steps) >= size(nb, D, longest, steps)
        assert size(nb, D, 2 * longest + 1024, steps) >= size(nb, D, longest, steps)
        assert size(nb, D, longest, steps + 1) > size(nb, D, longest, steps)
    assert size(0, 0, 0, 1) == cwqlib.cwq_greedy_encode_workspace_size(0, 0, 0)
    for bad in [(-1, 0, 0, 1), (1, -4, 4, 1), (1, 4, -4, 1), (1, 4, 4, 0)]:
        assert size(*bad) == 0


def _call(cwqlib, nb=2, d=4, n_bits=3, n_steps=2, sweeps=1, ws=None, off=None, total=None,
          opts=None):
    """Non-null dummy pointers: validation must answer before anything is read."""
    total = nb * d if total is None else total
    need = cwqlib.cwq_greedy_backfit_workspace_size(nb, nb * d, d, max(n_steps, 1))
    return cwqlib.cwq_greedy_backfit(1, 1, 1, 1, off, nb, total, d, n_bits, n_steps, sweeps, 42,
                                     1.0, 0, 1, 1, None, None, 1, need if ws is None else ws,
                                     opts, None)


def test_invalid_arguments_rejected_before_launch(cwqlib):
    for sweeps in (-1, 17, 1000):
        assert _call(cwqlib, sweeps=sweeps) == -1 and b"sweeps" in cwqlib.cwq_last_error()
    assert _call(cwqlib, n_bits=31) == -1 and b"n_bits_per_step" in cwqlib.cwq_last_error()
    assert _call(cwqlib, n_steps=0) == -1 and b"n_steps" in cwqlib.cwq_last_error()
    assert _call(cwqlib, total=9) == -1 and b"uniform" in cwqlib.cwq_last_error()
    need = cwqlib.cwq_greedy_backfit_workspace_size(2, 8, 4, 2)
    assert need > 0
    assert _call(cwqlib, ws=need - 1) == -3 and b"workspace" in cwqlib.cwq_last_error()
    assert _call(cwqlib, opts=_lib.options(prune_mode=3)) == -1
    assert b"cwq_options" in cwqlib.cwq_last_error()
    # an empty call succeeds without touching the device and clears the message
    assert cwqlib.cwq_greedy_backfit(None, None, None, None, None, 0, 0, 0, 3, 2, 1, 42, 1.0, 0,
                                     None, None, None, None, None, 0, None, None) == 0
    assert cwqlib.cwq_last_error() == b""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    from conftest import REPO
    so = tmp_path_factory.mktemp("backfit_plan") / "libbackfit_plan.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(REPO, "tests", "native", "backfit_plan.cpp")])
    L = ctypes.CDLL(str(so))
    i64 = ctypes.c_int64
    L.bf_path.argtypes, L.bf_path.restype = [i64, i64], ctypes.c_int
    L.bf_lane_min_blocks.restype = i64
    L.bf_encode_path.argtypes = [ctypes.c_int, i64, i64, i64, i64, ctypes.c_int, ctypes.c_int]
    L.bf_encode_path.restype = ctypes.c_int
    return L


def test_backfit_plan_table(plan):
    """csrc/cwq_dispatch.h backfit_plan: a lane per block only when no block
    exceeds 64 dims and there are 16,384 blocks or more; a wave per block
    otherwise and for an unknown length."""
    m = plan.bf_lane_min_blocks()
    assert m == 16384
    table = [((0, m), 1), ((1, m), 1), ((32, 65536), 1), ((64, m), 1), ((64, m - 1), 0),
             ((65, m), 0), ((65, 1 << 20), 0), ((4095, 18), 0), ((-1, 1 << 20), 0), ((32, 300), 0),
             ((8, 0), 0), ((13, 1), 0)]
    for args, want in table:
        assert plan.bf_path(*args) == want, args


def test_scoring_never_takes_the_self_finalizing_pipeline(plan):
    """EncodeShape::keys_only: the shapes of the small pipeline (every block at
    most 64 dims, 64 to 4,095 candidates, prune_mode 2) take the three-kernel
    path; every other shape keeps its path, and without the field nothing
    changes."""
    RowsWave, UniformPruned, CsrPruned, SmallPipe, SmallThree, Eval = range(6)
    longest = max(SMALL_PATH_SIZES["pipeline"])
    nb = len(SMALL_PATH_SIZES["pipeline"])
    assert longest == 64
    for n_cand in (64, 256, 2048):
        assert plan.bf_encode_path(1, 0, longest, nb, n_cand, 2, 0) == 2 * SmallPipe + 1
        assert plan.bf_encode_path(1, 0, longest, nb, n_cand, 2, 1) == 2 * SmallThree
        assert plan.bf_encode_path(0, 13, 13, 300, n_cand, 2, 0) == 2 * SmallPipe + 1
        assert plan.bf_encode_path(0, 13, 13, 300, n_cand, 2, 1) == 2 * SmallThree
    same = [(1, 0, 130, 8, 256, 2), (1, 0, 64, 13, 32, 2), (1, 0, 64, 13, 4096, 2),
            (1, 0, 4095, 18, 1 << 14, 2), (0, 16, 16, 16, 4096, 1), (0, 16, 16, 16, 4096, 0),
            (0, 32, 32, 65536, 256, 2), (0, 5, 5, 7, 8192, 2), (1, 0, 64, 13, 256, 1),
            (1, 0, -1, 13, 256, 2)]
    for shape in same:
        a, b = plan.bf_encode_path(*shape, 0), plan.bf_encode_path(*shape, 1)
        assert a == b and a % 2 == 0, shape
