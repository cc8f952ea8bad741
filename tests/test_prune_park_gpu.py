"""GPU: k_encode_prune's completed rows that park.

In tiles of 2^16 Philox blocks or more (CWQ_PARK_MIN_ROWS = 8,192 rows at d = 32,
twice as many at d = 16) of blocks of at least 16 dims the screening loop has no
completion test: a row that passes its last visit position walks on to a
sentinel record and waits there for the iteration that shares tau, which finds
it (csrc/cwq_kernels.hip, "Parked rows"; tests/test_park_plan.py replays the
control flow on the host).  Smaller tiles and d = 8 keep the loop with the test
(_parks below restates the rule).  Neither side may change a result.  Everything
here goes through cwq_selftest_encode_uniform_tau_guess and is
compared, indices and sample words, with prune_mode 0 of the same call:

  * every shape of tests/prune_refill_shapes.py and (nb, d, bits) = (3, 8, 13),
    (3, 32, 13), (2, 64, 13), (3, 32, 12), under tau-guess modes 0, 1 and 2.
    Few blocks are cut into tiles of 256 rows, and the one-tile blocks of
    prune_refill_shapes.py have at most 4,096, so these take the loop with the
    completion test, all but d = 64 at 12 bits (4,096 rows of 16 Philox blocks),
    which parks; so do d = 8 and d = 16 at 2^13 candidates in 16,384 blocks;
  * PARKED: 16,384 blocks, one tile each, of 2^14 candidates at d = 16 and 2^13
    at d = 32 and 64, which take the loop without it, under the same modes (mode
    2 runs every pass twice);
  * the near-tie blocks of tests/encode_shapes.py that run k_encode_prune
    (tests/near_ties.py's inputs), against the oracle's declared indices too;
  * target = proposal at d = 32 and 13 bits, one block (tiles of 256 rows) and
    16,384 blocks (parked), and a flat target at d = 32 and 13 bits in 16,384
    blocks: every row completes, 8,192 rows pass the survivor list's 1,024
    slots, so the list-full branch scores rows from the parked path.
"""
import functools

import numpy as np
import pytest
import torch

import encode_shapes as S
import near_ties as NT
import prune_refill_shapes as R
from test_prune_refill_gpu import BASE, SEED, _inputs, _same

pytestmark = pytest.mark.gpu

GUESS_MODES = (0, 1, 2)
ISSUE_SHAPES = [(8, 13, 3, 1), (32, 13, 3, 1), (64, 13, 2, 1), (32, 12, 3, 1)]  # (d, bits, nb, steps)
PARKED = [(16, 14, R.MANY, 1), (32, 13, R.MANY, 1), (64, 13, R.MANY, 1)]
SMALL_D = [(8, 13, R.MANY, 1), (16, 13, R.MANY, 1)]   # 8,192 rows of two and four units


def _parks(shape):
    """launch_prune_t's rule (csrc/cwq_kernels.hip), on choose_tiling's tiles."""
    import prune_tau_shapes as P
    d, bits, nb, _ = shape
    rows = min(P.tiling(nb, 1 << bits)[1], 1 << bits)
    return d >= 16 and rows * d >= 8192 * 32
NEAR_TIES = ["prune_d8", "prune_d16", "prune_d32", "prune_d64", "tau_guess", "tile_queue"]


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    return C


def _selftest(cwqlib, shape, host, prune, guess, seed=SEED, rho=1.0, base=BASE):
    """cwq_selftest_encode_uniform_tau_guess: (indices, sample words)."""
    from compression_without_quantization_amd import _lib
    d, bits, nb, n_steps = shape
    tl, ts, pl, ps = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in host)
    idx = torch.full((nb, n_steps), -77, dtype=torch.int32, device="cuda")
    sample = torch.full((nb * d,), float("nan"), dtype=torch.float32, device="cuda")
    need = int(cwqlib.cwq_greedy_encode_uniform_workspace_size(nb, d))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    rc = cwqlib.cwq_selftest_encode_uniform_tau_guess(
        tl.data_ptr(), ts.data_ptr(), pl.data_ptr(), ps.data_ptr(), nb, d, bits, n_steps, seed,
        rho, base, idx.data_ptr(), sample.data_ptr(), ws.data_ptr(), ws.numel(),
        _lib.options(prune, None), torch.cuda.current_stream().cuda_stream, guess)
    _lib.check(rc, "cwq_selftest_encode_uniform_tau_guess")
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.int64), sample.cpu().numpy().view(np.uint32).copy()


def _modes_against_exact(cwqlib, shape, kind="normal", modes=GUESS_MODES):
    host = _inputs(shape, kind)
    want = _selftest(cwqlib, shape, host, 0, 0)
    assert (want[0] >= 0).all() and (want[0] < 1 << shape[1]).all()
    for g in modes:
        _same(_selftest(cwqlib, shape, host, 2, g), want,
              f"{shape} {kind}: guess mode {g} against prune_mode 0")
    return want


def test_shapes_are_on_both_sides_of_the_parking_threshold():
    """What the docstring says of the tiles."""
    assert [s for s in R.ALL + ISSUE_SHAPES + SMALL_D if _parks(s)] == [(64, 12, R.MANY, 1)]
    assert all(_parks(s) for s in PARKED)
    assert _parks((32, 16, 1000000, 1)) and _parks((16, 24, 1024, 1))  # the benchmark's C4, C5


@pytest.mark.parametrize("shape", R.ALL + ISSUE_SHAPES + SMALL_D, ids=lambda s: "d%d_b%d_nb%d_s%d" % s)
def test_refill_and_small_shapes(cwq, cwqlib, shape):
    _modes_against_exact(cwqlib, shape)


@pytest.mark.parametrize("shape", PARKED, ids=lambda s: "d%d_b%d_nb%d_s%d" % s)
def test_parked_tiles(cwq, cwqlib, shape):
    _modes_against_exact(cwqlib, shape)


@functools.lru_cache(maxsize=None)
def _near_tie_case(name):
    c = dict(S.NEAR_TIE_CASES[name])
    assert c["d"] is not None and c["path"] == "uniform_pruned"
    c["nb"] = len(c["sizes"])
    c["off"] = NT.offsets(c["sizes"])
    c["rho"] = 0.8 if c["n_steps"] > 1 else 1.0
    c["host"] = NT.inputs(c["off"], c["input_seed"], c["level"])
    return c


@pytest.mark.parametrize("name", NEAR_TIES)
def test_near_ties(cwq, cwqlib, oracle, name):
    """Rows a rounding apart or tied: a drop that is not a subset of upper <
    tau's, or a tied row not pushed from where it parks, changes an index."""
    c = _near_tie_case(name)
    shape = (c["d"], c["bits"], c["nb"], c["n_steps"])
    kw = dict(seed=NT.SEED, rho=c["rho"], base=NT.BASE)
    want = _selftest(cwqlib, shape, c["host"], 0, 0, **kw)
    for g in GUESS_MODES:
        _same(_selftest(cwqlib, shape, c["host"], 2, g, **kw), want,
              f"{name}: guess mode {g} against prune_mode 0")
    blocks = np.arange(min(c["nb"], NT.certified_blocks(c["off"])))
    idx, _ = NT.declared(c["host"], c["off"], c["bits"], c["n_steps"], NT.SEED, c["rho"], NT.BASE,
                         blocks)
    assert np.array_equal(want[0][blocks], idx[blocks].astype(np.int64)), f"{name}: the oracle"


@pytest.mark.parametrize("shape,kind", [((32, 13, 1, 1), "posterior_is_prior"),
                                        ((32, 13, R.MANY, 1), "posterior_is_prior"),
                                        ((32, 13, R.MANY, 1), "flat_target")],
                         ids=["one_block", "parked", "parked_list_full"])
def test_every_row_in_reach(cwq, cwqlib, shape, kind):
    _modes_against_exact(cwqlib, shape, kind, modes=(0, 1) if shape[2] > 1 else GUESS_MODES)
