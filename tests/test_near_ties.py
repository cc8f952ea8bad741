"""CPU: the near-tie cases of tests/encode_shapes.py (NEAR_TIE_CASES) really
separate the declared arithmetic from its neighbours.

tests/test_near_ties_gpu.py holds every greedy-family scoring path to the
oracle on these inputs.  That says something about summation order, the d % 8
tail, log sigma and the tie rule only if another choice of any of them would
have produced other indices.  Here the oracle itself says so
(tests/near_ties.py, certificate()): with the coder's seed, block_id_base and
rho that the GPU test uses, for every case

* each row-sum order that can differ from the declared one at the case's block
  lengths (sse4, avx8x2, avx512, seq, tree) and log sigma one ulp up or down
  changes the index row of at least 4 blocks -- so swapping the reference for
  any applicable variant's index table makes the GPU comparison fail;
* at least 4 (block, step) pairs are exact ties between the two best rows that
  an index other than 0 wins (the lowest-index rule, across tiles and waves);
* the declared indices are spread out: their distinct values number at least
  half the non-empty (block, step) pairs, or half of 2^bits if that is smaller.

These are conditions on the inputs, not measurements: the cases' input seeds
and levels are chosen so that they hold, from the oracle alone.
"""
import numpy as np
import pytest

import encode_shapes as S
import near_ties as NT

MIN_FLIPS = 4
MIN_TIES = 4


def case_values(name):
    c = S.NEAR_TIE_CASES[name]
    off = NT.offsets(c["sizes"])
    return off, NT.inputs(off, c["input_seed"], c["level"])


def case_rho(c):
    return 0.8 if c["n_steps"] > 1 else 1.0


def test_inputs_are_the_declared_family():
    off = NT.offsets([3, 0, 20])
    a = NT.inputs(off, 7)
    b = NT.inputs(off, 7)
    rng = np.random.Generator(np.random.PCG64(7))
    ts = (rng.uniform(0.5, 2.0, 23) * 300.0).astype(np.float32)
    assert all(x.dtype == np.float32 and x.shape == (23,) for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[1], ts)
    assert a[1].min() >= 150.0 and a[1].max() <= 600.0
    assert np.abs(a[2]).max() > 0 and a[3].min() >= 0.8 and a[3].max() <= 1.25
    assert NT.inputs(off, 7, 1000.0)[1].min() >= 500.0
    assert not np.array_equal(NT.inputs(off, 8)[0], a[0])


def test_applicable_is_the_row_sum_orders_reach():
    """A tail alone is the sequential sum; one packet has no second accumulator
    and two Packet4f fold like one Packet8f; avx8x2 needs a third packet."""
    assert not any(NT.applicable(o, [1]) for o in NT.ORDERS)
    assert [o for o in NT.ORDERS if NT.applicable(o, [5])] == ["sse4", "tree"]
    assert [o for o in NT.ORDERS if NT.applicable(o, [8])] == ["avx512", "seq", "tree"]
    assert not NT.applicable("avx8x2", [15, 3, 0, 8]) and not NT.applicable("avx8x2", [16])
    assert NT.applicable("avx8x2", [24]) and NT.applicable("avx8x2", [3, 45])
    assert all(NT.applicable(o, [4095]) for o in NT.VARIANTS)
    assert NT.applicable("ls_up", [1]) and NT.applicable("ls_dn", [])


def test_certificate_keeps_each_blocks_seed(oracle):
    """The certificate of a prefix, and of blocks at mixed budgets, is the
    oracle's own encoding block by block."""
    name = "var_short"
    c = S.NEAR_TIE_CASES[name]
    off, values = case_values(name)
    r = NT.certificate(values, off, c["bits"], c["n_steps"], NT.SEED, 0.8, NT.BASE, max_blocks=9)
    nb = NT.certified_blocks(off, 9)
    assert r["blocks"] == 9 and r["declared"].shape == (nb, c["n_steps"]) and nb > 9
    for g in range(nb):
        sl = slice(int(off[g]), int(off[g + 1]))
        want, _ = oracle.greedy_encode(*(a[sl] for a in values), [0, sl.stop - sl.start],
                                       c["bits"][g], c["n_steps"], NT.SEED, 0.8, NT.BASE + g)
        assert np.array_equal(r["declared"][g], want[0]), g


@pytest.mark.parametrize("name", list(S.NEAR_TIE_CASES))
def test_case_is_certified(oracle, name):
    c = S.NEAR_TIE_CASES[name]
    off, values = case_values(name)
    lens = np.diff(off)
    assert (lens > 0).sum() >= S.NEAR_TIE_MIN_BLOCKS
    r = NT.certificate(values, off, c["bits"], c["n_steps"], NT.SEED, case_rho(c), NT.BASE)
    covered = lens[:r["declared"].shape[0]]
    apply = [v for v in NT.VARIANTS if NT.applicable(v, covered)]
    counts = (f"{name}: {r['blocks']} blocks, flips {r['flips']} (applicable: {apply}), "
              f"{r['ties']} non-zero ties, {r['distinct']} distinct indices in {r['pairs']} pairs")
    print(counts)
    assert {"ls_up", "ls_dn", "tree"} <= set(apply), counts
    for v in apply:
        assert r["flips"][v] >= MIN_FLIPS, counts
    for v in set(NT.VARIANTS) - set(apply):
        assert r["flips"][v] == 0, counts  # applicable() misses nothing the oracle sees
    assert r["ties"] >= MIN_TIES, counts
    assert r["distinct"] >= min((r["pairs"] + 1) // 2, (1 << int(np.max(c["bits"]))) // 2), counts
    # the oracle's encoder is the declared variant
    sub = off[:r["declared"].shape[0] + 1]
    if np.ndim(c["bits"]) == 0:
        want, _ = oracle.greedy_encode(*(a[:int(sub[-1])] for a in values), sub, c["bits"],
                                       c["n_steps"], NT.SEED, case_rho(c), NT.BASE)
        assert np.array_equal(r["declared"], want), counts
