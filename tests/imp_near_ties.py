"""Near-tie inputs for the importance coder's scoring paths, and the CPU
oracle's certificate that they tell the declared arithmetic from its
neighbours.  A helper of tests/test_imp_near_ties.py (CPU) and
tests/test_imp_near_ties_gpu.py; not a test, and nothing in the product
imports it.  The greedy family's counterpart is tests/near_ties.py.

An index is an argmax over float32 scores sum_j (log q(x_j) - log p(x_j)).  On
informative targets the two best rows of a group lie many roundings apart, and
with the standard proposal x = RN(0 + RN(1 z)) is z itself, so a kernel that
sums a row in another order, contracts pl + ps z into an fma, scores log p
without the round trip through x or merges tiles with another tie rule still
emits the oracle's index.  The family here takes a proposal that is not the
standard one and a target within a relative eps = 2^-24 .. 2^-27 of it: every
term is then rounding noise around 0, the best rows of a group differ by a
rounding or not at all, and the winner is spread over the whole index range.

One neighbour stays out of reach of that family, and provably so: the order of
the row sum.
Both log-probs of a dim are at least 0.5 in magnitude here (their normalisers
are: 0.919 + log 0.8 = 0.70), so every term lt - lq is a multiple of 2^-24, and
a row's terms are a few such units each.  Sums of multiples of 2^-24 below 1
in magnitude are exact in float32 in any order, so all six orders give every
candidate row the same score (certificate()["differs"] counts the groups where
they do not: none).  A sum rounds only once it reaches 1, and scores that large
lie many units apart at the top.  Rounding-sized gaps and order-dependent sums
exclude each other in this family, whatever eps.  The case nt_sum therefore
adds one informative dim per group and many more rows (inputs(), ``lead``).

certificate() asks the oracle alone what each neighbouring arithmetic would
emit on these inputs (oracle.importance_encode_semvar) and counts the groups
whose index differs from the declared one, the exact ties a non-zero index
wins, and the distinct declared indices.
"""
import numpy as np

from near_ties import _probe
from oracle import oracle as O

F32 = np.float32
EPS = 2.0 ** -24
# the neighbouring arithmetics, as oracle.IMP_VARIANTS numbers them (0: declared)
VARIANTS = O.IMP_VARIANTS[1:]
ORDERS = {name: O.SEM_ORDERS.index(name) for name in O.SEM_ORDERS[1:]}
MIN_FLIPS = 4
MIN_TIES = 4


def inputs(off, rng_seed, eps=EPS, lead=None):
    """(t_loc, t_scale, p_loc, p_scale), float32 [off[-1]]: p_loc = 0.1 N(0, 1),
    p_scale = U(0.8, 1.25), t_scale = p_scale (1 + eps U(-1, 1)), t_loc = p_loc +
    p_scale eps N(0, 1), computed in float64 and rounded once.

    lead (a ratio > e, or None): the first dim of every group gets the target
    N(p_loc, p_scale / lead) instead.  Its term log(lead) - (lead^2 - 1) z^2 / 2
    is at most log(lead) > 1 and reaches it where z is near 0: the best rows of
    a group of N rows pile up within about (lead / N)^2 of that value, so with
    some 10^4 rows they share the lead term to within a rounding and the other
    dims' few units of 2^-24 decide -- now at a score above 1 (above 2 from
    lead = e^2), where adding those units rounds, in an order-dependent way.
    This is what lets the row-sum orders be certified (case nt_sum)."""
    rng = np.random.Generator(np.random.PCG64(rng_seed))
    off = np.asarray(off, np.int64)
    D = int(off[-1])
    pl = 0.1 * rng.standard_normal(D)
    ps = rng.uniform(0.8, 1.25, D)
    ts = ps * (1.0 + eps * rng.uniform(-1.0, 1.0, D))
    tl = pl + ps * eps * rng.standard_normal(D)
    tl, ts, pl, ps = (np.ascontiguousarray(v, dtype=F32) for v in (tl, ts, pl, ps))
    if lead is not None:
        first = off[:-1][np.diff(off) > 0]
        ts[first] = ps[first] / F32(lead)
        tl[first] = pl[first]
    return tl, ts, pl, ps


def certified_groups(sizes, only=None, max_groups=64):
    """The groups a certificate covers: the first max_groups non-empty ones
    (of ``only``, when given)."""
    full = np.flatnonzero(np.asarray(sizes, np.int64) > 0)
    if only is not None:
        full = full[np.isin(full, np.asarray(only, np.int64))]
    return full[:max_groups]


def applicable(variant, lengths):
    """Can this variant differ from the declared arithmetic at these group
    lengths?  Decided by the oracle alone: a row-sum order is applicable when
    its sum of some fixed pseudo-random row of one of the lengths is not the
    declared order's; the form, fma, quadratic and ulp variants always are."""
    if variant not in ORDERS:
        return True
    o = ORDERS[variant]
    return any(O.sem_rowsum(x, o) != O.sem_rowsum(x, 0)
               for d in sorted(set(int(n) for n in lengths if n > 0)) for x in _probe(d))


def reach(variant, lengths):
    """The number of groups at whose length the variant can differ at all."""
    return sum(1 for d in lengths if applicable(variant, [d]))


def certificate(case, max_groups=64):
    """``case``: a near-tie Blocks of tests/importance_shapes.py.  On its
    certified groups (case.certify, default all; the first max_groups non-empty
    ones), from the oracle alone, each group keeping its number, hence its seed:

      groups    their numbers
      declared  the declared indices [len(groups)]
      tables    {variant: its indices, same shape}
      flips     {variant: groups whose index differs from the declared one}
      ties      groups with best == second best and a declared index > 0
      distinct  distinct declared indices
      gap       declared best - second best [len(groups)], float64
      differs   {variant: groups in which it scores any candidate row differently}
    """
    groups = certified_groups(case.sizes, getattr(case, "certify", None), max_groups)
    keep = np.zeros(case.sizes.size, bool)
    keep[groups] = True
    sub = np.concatenate([[0], np.cumsum(np.where(keep, case.sizes, 0))]).astype(np.int64)
    dims = np.concatenate([np.arange(case.off[g], case.off[g + 1]) for g in groups] +
                          [np.zeros(0, np.int64)]).astype(np.int64)
    tl, ts, pl, ps = (np.ascontiguousarray(a[dims]) for a in case.inputs())
    counts = np.where(keep, case.oracle_counts, 1)   # the emptied groups: one row of no dims
    vidx, gap, _, nd = O.importance_encode_semvar(tl, ts, pl, ps, sub, counts, case.seed,
                                                  case.base)
    vidx, gap, nd = vidx[groups], gap[groups], nd[groups]
    declared = vidx[:, 0]
    tables = {name: vidx[:, 1 + i] for i, name in enumerate(VARIANTS)}
    return dict(groups=groups, declared=declared, tables=tables, gap=gap,
                differs={name: int((nd[:, 1 + i] > 0).sum()) for i, name in enumerate(VARIANTS)},
                flips={name: int((t != declared).sum()) for name, t in tables.items()},
                ties=int(((gap == 0) & (declared > 0)).sum()),
                distinct=int(np.unique(declared).size))


def required(case, cert):
    """The variants whose table must differ from the declared indices on at
    least MIN_FLIPS groups.  The form, fma, quadratic and ulp variants always;
    a row-sum order when it can differ at the lengths of at least MIN_FLIPS
    certified groups and scores some candidate row of at least MIN_FLIPS of
    them differently (otherwise it cannot reach the count: "-" in DESIGN.md's
    table)."""
    lengths = case.sizes[cert["groups"]]
    return [v for v in VARIANTS
            if v not in ORDERS or (reach(v, lengths) >= MIN_FLIPS and
                                   cert["differs"][v] >= MIN_FLIPS)]
