"""GPU: k_encode_prune's screening loop, unrolled.

The screening pass of a tile that parks runs trips of CWQ_SHARE_UNROLL = 8 copies of its body, with
no exit and no test of the active mask inside a trip, while every lane of the
wave is active and its pool holds the 512 rows that eight refills can take at
most; the rest is handed out by the one-copy loop behind it
(csrc/cwq_kernels.hip; tests/test_unroll_plan.py replays the control
flow on the host).  A wave's share R is a quarter of its tile and its pool the
rows behind S(R) (csrc/cwq_refill.h), so the unrolled loop runs from R = 4,096
on (_unrolls below restates the rule) and every smaller tile takes the one-copy
loop alone.  Neither may change a result.  Everything here goes through
cwq_selftest_encode_uniform_tau_guess and is compared, indices and sample
words, with prune_mode 0 of the same call, under tau-guess modes 0, 1 and 2:

  * tiles that leave waves empty or part-filled: (d, bits, nb) = (8, 4, MANY),
    (32, 4, MANY), (32, 6, MANY), (32, 7, 3), (64, 5, 2): 16 to 128 candidates
    per tile, so three, two or no empty waves, and a wave with 16 active lanes;
    a wave that starts with no row must run no copy;
  * shares that are no multiple of the unroll: every shape of
    tests/prune_refill_shapes.py (R = 64, 128, 256, 1,024, INTER tiles and a
    multi-step case);
  * both sides of the parking rule: (32, 13, MANY), (64, 13, MANY) and
    (16, 14, MANY) park, (32, 12, 3) and (32, 13, 3) do not;
  * tiles whose waves run unrolled trips: R = 4,096 at d = 16 and 64, where the
    pool is exactly one trip's rows, 8,192 at d = 16, and the benchmark's own
    tile of 2^16 candidates at d = 32 (R = 16,384);
  * rows found by the look of an unrolled trip and of the loop behind it:
    target = proposal at (64, 14, MANY) and (32, 13, 1), and the flat target at
    (32, 13, MANY), where every row completes and the survivor list overflows
    from the parked path;
  * the near-tie blocks of tests/encode_shapes.py that run k_encode_prune,
    against the oracle's declared indices too.
"""
import numpy as np
import pytest

import prune_refill_shapes as R
import prune_tau_shapes as P
from test_prune_park_gpu import (GUESS_MODES, NEAR_TIES, NT, _modes_against_exact, _near_tie_case,
                                 _parks, _same, _selftest, cwq)  # noqa: F401 (cwq: a fixture)

pytestmark = pytest.mark.gpu

EMPTY_WAVES = [(8, 4, R.MANY, 1), (32, 4, R.MANY, 1), (32, 6, R.MANY, 1), (32, 7, 3, 1), (64, 5, 2, 1)]
PARKING = [(32, 13, R.MANY, 1), (64, 13, R.MANY, 1), (16, 14, R.MANY, 1), (32, 12, 3, 1), (32, 13, 3, 1)]
UNROLLED = [(64, 14, R.MANY, 1), (16, 15, R.MANY, 1), P.WORKLOAD_TILE]
UNROLL = 8        # CWQ_SHARE_UNROLL


def _ids(s):
    return "d%d_b%d_nb%d_s%d" % s


def _static_rows(r):
    """csrc/cwq_refill.h refill_static_rows."""
    return 0 if r < 128 else (r * 7 // 8) & ~63


def _unrolls(shape):
    """Whether a wave of the shape's full tiles runs an unrolled trip: the tile
    parks, every lane has a row and the pool holds 64 rows per copy
    (k_encode_prune)."""
    _, bits, nb, _ = shape
    rows = min(P.tiling(nb, 1 << bits)[1], 1 << bits)
    r = -(-rows // 4)
    return _parks(shape) and r >= 128 and r - max(_static_rows(r), 64) >= 64 * UNROLL


def test_shapes_are_on_both_sides_of_the_rules():
    """What the docstring says of the tiles."""
    assert all(_unrolls(s) for s in UNROLLED)
    assert not any(_unrolls(s) for s in EMPTY_WAVES + R.ALL + [s for s in PARKING if s[0] != 16])
    assert _unrolls((16, 14, R.MANY, 1))       # R = 4,096: the pool is one trip's rows
    assert [_parks(s) for s in PARKING] == [True, True, True, False, False]
    assert all(_parks(s) for s in UNROLLED)
    assert _unrolls((32, 16, 1000000, 1)) and _unrolls((16, 24, 1024, 1))  # the benchmark's C4, C5
    assert not _unrolls((8, 16, R.MANY, 1))    # d = 8 never parks
    # waves without a row, and one with 16 active lanes
    rows = [min(P.tiling(nb, 1 << bits)[1], 1 << bits) for _, bits, nb, _ in EMPTY_WAVES]
    assert rows == [16, 16, 64, 128, 32]


@pytest.mark.parametrize("shape", EMPTY_WAVES, ids=_ids)
def test_empty_and_part_filled_waves(cwq, cwqlib, shape):
    _modes_against_exact(cwqlib, shape)


@pytest.mark.parametrize("shape", R.ALL, ids=_ids)
def test_shares_that_are_no_multiple_of_the_unroll(cwq, cwqlib, shape):
    _modes_against_exact(cwqlib, shape)


@pytest.mark.parametrize("shape", PARKING, ids=_ids)
def test_both_sides_of_the_parking_rule(cwq, cwqlib, shape):
    _modes_against_exact(cwqlib, shape)


@pytest.mark.parametrize("shape", UNROLLED, ids=_ids)
def test_unrolled_trips(cwq, cwqlib, shape):
    _modes_against_exact(cwqlib, shape)


@pytest.mark.parametrize("shape,kind", [((32, 13, 1, 1), "posterior_is_prior"),
                                        ((64, 14, R.MANY, 1), "posterior_is_prior"),
                                        ((32, 13, R.MANY, 1), "flat_target")],
                         ids=["one_block", "unrolled", "parked_list_full"])
def test_rows_found_by_a_look(cwq, cwqlib, shape, kind):
    _modes_against_exact(cwqlib, shape, kind, modes=(0, 1) if shape[2] > 1 else GUESS_MODES)


@pytest.mark.parametrize("name", NEAR_TIES)
def test_near_ties(cwq, cwqlib, oracle, name):
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
