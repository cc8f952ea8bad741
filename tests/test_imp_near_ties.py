"""CPU: the near-tie cases of tests/importance_shapes.py (NEAR_TIE_CASES) really
separate the importance coder's declared arithmetic from its neighbours.

tests/test_imp_near_ties_gpu.py holds every scoring path of the importance
coder to the oracle on these inputs.  That says something about the fma in
x = pl + ps z, the round trip of log p through x, the log-prob form, the
normalisers and the tie rule only if another choice of any of them would have
produced other indices.  Here the oracle itself says so
(tests/imp_near_ties.py, certificate()): with the coder's seed and
block_id_base that the GPU test uses, on the first 64 non-empty groups of each
case (nt_overflow: its ten ladder groups)

* each required variant (the TFP >= 0.8 form, x as one fma, log p without the
  round trip, the term as a float quadratic, ct and cp one ulp up and down)
  changes the emitted index of at least 4 groups -- so swapping the reference
  for that variant's index table makes the GPU comparison fail;
* at least 4 groups are exact ties between the two best rows that an index
  other than 0 wins (the lowest-index rule, across lanes, waves and tiles);
* the winners take at least half as many distinct values as there are groups.

The other row-sum orders (sse4, avx8x2, avx512, seq, tree) cannot be required
on the six cases of the plain family: there they give every candidate row the
declared score (test_row_sum_orders_cannot_differ, and the reason in
imp_near_ties.py).  The seventh case, nt_sum, lifts the scores above 2 with one
informative dim per group; on it all thirteen variants are required.

These are conditions on the inputs, not measurements: each case's input seed
and eps (importance_shapes.NT_LEVELS) are chosen so that they hold, from the
oracle alone.
"""
import numpy as np
import pytest

import imp_near_ties as NT
import importance_shapes as S

_CERT = {}


def cert(name):
    if name not in _CERT:
        case = S.near_tie_case(name)
        _CERT[name] = (case, NT.certificate(case))
    return _CERT[name]


def test_inputs_are_the_declared_family():
    off = np.array([0, 3, 3, 23], np.int64)
    tl, ts, pl, ps = NT.inputs(off, 7)
    again = NT.inputs(off, 7)
    assert all(a.dtype == np.float32 and a.shape == (23,) for a in (tl, ts, pl, ps))
    assert all(np.array_equal(a, b) for a, b in zip((tl, ts, pl, ps), again))
    rng = np.random.Generator(np.random.PCG64(7))
    assert np.array_equal(pl, (0.1 * rng.standard_normal(23)).astype(np.float32))
    assert np.array_equal(ps, rng.uniform(0.8, 1.25, 23).astype(np.float32))
    assert ps.min() >= 0.8 and ps.max() <= 1.25 and np.abs(pl).max() > 0
    # the target lies within a few ulps of the proposal, and not on it everywhere
    assert np.abs(ts / ps - 1).max() <= 2.0 ** -22 and np.abs(tl - pl).max() <= 2.0 ** -21
    assert (ts != ps).any() and (tl != pl).any()
    wide = NT.inputs(off, 7, 2.0 ** -12)
    assert 2.0 ** -16 < np.abs(wide[1] / wide[3] - 1).max() <= 2.0 ** -12 + 2.0 ** -23
    assert not np.array_equal(NT.inputs(off, 8)[2], pl)


def test_applicable_is_the_row_sum_orders_reach():
    assert not any(NT.applicable(o, [1]) for o in NT.ORDERS)
    assert [o for o in NT.ORDERS if NT.applicable(o, [5])] == ["sse4", "tree"]
    assert NT.reach("avx512", [7, 3, 16, 1, 5, 9, 2, 12, 6, 4]) == 2   # 9 and 12 dims
    assert all(NT.applicable(v, [1]) for v in NT.VARIANTS if v not in NT.ORDERS)
    assert len(NT.VARIANTS) == 13 and set(NT.ORDERS) < set(NT.VARIANTS)


@pytest.mark.parametrize("name", S.NEAR_TIE_CASES)
def test_variant_0_is_the_declared_encoder(oracle, name):
    """Group by group (each with its own seed), the certificate's declared
    column is oracle.importance_encode."""
    case, r = cert(name)
    tl, ts, pl, ps = case.inputs()
    groups = r["groups"]
    if name == "nt_overflow":   # ten groups of a large launch: one at a time
        for k, g in enumerate(groups):
            sl = slice(int(case.off[g]), int(case.off[g + 1]))
            want, _ = oracle.importance_encode(tl[sl], ts[sl], pl[sl], ps[sl], [0, sl.stop - sl.start],
                                               [case.oracle_counts[g]], case.seed, case.base + int(g))
            assert want[0] == r["declared"][k], (name, g)
    else:
        want, _ = oracle.importance_encode(tl, ts, pl, ps, case.off, case.oracle_counts,
                                           case.seed, case.base)
        assert np.array_equal(want[groups], r["declared"]), name


@pytest.mark.parametrize("name", S.NEAR_TIE_CASES)
def test_case_is_certified(oracle, name):
    case, r = cert(name)
    groups = r["groups"]
    assert groups.size == min(64, int((case.sizes > 0).sum()) if case.certify is None
                              else len(case.certify))
    req = NT.required(case, r)
    counts = (f"{name}: {groups.size} groups, eps 2^{int(np.log2(case.eps))}, flips {r['flips']} "
              f"(required: {req}), {r['ties']} non-zero ties, {r['distinct']} distinct indices, "
              f"median gap {np.median(r['gap']) * 2.0 ** 24:.1f} x 2^-24")
    print(counts)
    assert set(req) >= set(NT.VARIANTS) - set(NT.ORDERS), counts
    for v in req:
        assert r["flips"][v] >= NT.MIN_FLIPS, counts
    for v in set(NT.VARIANTS) - set(req):   # an order left out really cannot reach the count
        assert r["flips"][v] <= r["differs"][v] < NT.MIN_FLIPS, counts
    assert r["ties"] >= NT.MIN_TIES, counts
    assert 2 * r["distinct"] >= groups.size, counts
    # the group seeds wrap int32 inside the certified range
    assert case.seed < 2 ** 31 <= case.seed + case.base + int(groups[-1])


@pytest.mark.parametrize("name", [n for n in S.NEAR_TIE_CASES if n != "nt_sum"])
def test_row_sum_orders_cannot_differ(oracle, name):
    """Every term is a small multiple of 2^-24 and every partial sum stays
    below 1, so the six row-sum orders agree on every candidate row: no level
    of the plain family can certify the order of the sum."""
    case, r = cert(name)
    assert case.lead is None
    assert all(r["differs"][o] == 0 and r["flips"][o] == 0 for o in NT.ORDERS), r["differs"]
    assert all(r["differs"][v] >= NT.MIN_FLIPS for v in NT.VARIANTS if v not in NT.ORDERS)


def test_nt_sum_certifies_the_row_sum_orders(oracle):
    case, r = cert("nt_sum")
    assert case.lead > np.e ** 2 and NT.required(case, r) == list(NT.VARIANTS)
    tl, ts, pl, ps = case.inputs()
    first = case.off[:-1]
    assert np.array_equal(tl[first], pl[first])
    assert np.array_equal(ts[first], ps[first] / np.float32(case.lead))
    rest = np.ones(tl.size, bool)
    rest[first] = False
    assert np.abs(ts[rest] / ps[rest] - 1).max() <= 2.0 ** -22
