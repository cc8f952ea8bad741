"""GPU: k_encode_prune's folded Philox add and downward static rows.

The screening loop forms a visit's Philox block inside round 0's multiply-add,
from per-wave records that hold M0 (w0 G + g_k) (csrc/cwq_philox_lo.h), and a
lane walks its static rows from the last one down, the subtract's borrow
telling when they are used up (csrc/cwq_kernels.hip; the hand-out is replayed
on the host by tests/test_refill_desc_plan.py).  Neither may change a result:

  * every shape of tests/prune_refill_shapes.py (wave shares of 64, 128, 256
    and 1,024 rows in one-tile blocks, INTER tiles with tails, three steps):
    prune_mode 0, 1 and 2 agree bit for bit, and mode 2 with the CPU oracle on
    that file's sample of blocks (computed once, shared with
    tests/test_prune_refill_gpu.py through its cache);
  * a flat target (every row completes) and locations outside the screening
    gate (the exact pass, which forms its blocks with a plain add);
  * every screened tile retried (the pass runs twice from the same start);
  * one block at the index limit, d = 64 at 28 bits: 2^28 rows of 16 Philox
    blocks, the last wave's share ending at block 2^32.  Mode 2 against mode 0;
    the oracle is too slow for this shape.
"""
import numpy as np
import pytest
import torch

import prune_refill_shapes as R
from test_prune_refill_gpu import _check, _encode, _inputs, _same
from test_tau_guess_gpu import _encode as _encode_guess

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    return C


@pytest.mark.parametrize("shape", R.ALL, ids=lambda s: "d%d_b%d_nb%d_s%d" % s)
def test_modes_agree_and_match_oracle(cwq, oracle, shape):
    _check(cwq, oracle, shape)


@pytest.mark.parametrize("kind", ["flat_target", "huge_locs"])
def test_all_rows_complete_and_exact_pass(cwq, oracle, kind):
    """(32, 10, MANY, 1).  A flat target: every row completes, so every lane
    walks all its static rows to the borrow.  Locations outside the screening
    gate: the exact pass runs the same hand-out."""
    _check(cwq, oracle, (32, 10, R.MANY, 1), kind)


@pytest.mark.parametrize("shape", [(32, 12, R.MANY, 1), (8, 9, R.MANY, 1)],
                         ids=lambda s: "d%d_b%d" % s[:2])
def test_every_tile_retried(cwq, cwqlib, shape):
    """The forced retry: the screening pass starts over, lanes, pool counter
    and the mask of lanes past their static rows included."""
    host = _inputs(shape)
    want = _encode(cwq, shape, host, 0)
    _same(_encode_guess(cwqlib, shape, host, 2), want, f"{shape}: every tile retried against mode 0")


def test_index_limit(cwq):
    """d = 64 at 28 bits, one block: n G reaches 2^32 - 16."""
    shape = (64, 28, 1, 1)
    assert (1 << shape[1]) * (shape[0] // 4) == 1 << 32
    host = _inputs(shape)
    want = _encode(cwq, shape, host, 0)
    got = _encode(cwq, shape, host, 2)
    _same(got, want, "d = 64, 28 bits: mode 2 against mode 0")
    assert 0 <= int(got[0][0, 0]) < 1 << 28
