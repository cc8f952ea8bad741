"""Near-tie inputs for the greedy coder's scoring paths, and the CPU oracle's
certificate that they tell the declared arithmetic from its neighbours.  A
helper of tests/test_near_ties.py (CPU) and tests/test_near_ties_gpu.py; not a
test, and nothing in the product imports it.

An index is an argmax over float32 row values.  On random targets the best two
rows of a block lie many roundings apart, so a kernel that sums a row in
another order, folds the d % 8 tail elsewhere, takes log sigma one ulp off or
merges tiles with another tie rule still emits the oracle's index.  The family
here makes the target so wide (t_scale = U(0.5, 2) * level) that every row's
value is the sum of nearly equal terms: the best rows differ by a rounding or
not at all, and the winner is spread over the whole index range.

certificate() asks the oracle alone what each neighbouring arithmetic would
emit on these inputs (oracle.greedy_encode_semvar: the row-sum orders;
oracle.greedy_encode_lsig: log sigma one ulp up and down) and counts the blocks
whose indices differ from the declared ones, the exact ties a non-zero index
wins, and the distinct declared indices.
"""
import functools

import numpy as np

from oracle import oracle as O

F32 = np.float32
SEED = 2147483647 - 3  # seed + base + g wraps past 2^31 - 1 in every case
BASE = 5               # block_id_base
# the row-sum orders of the declared (TFP <= 0.7) form other than the declared
# one, as oracle.SEM_ORDERS numbers them, and the two shifted normalisers
ORDERS = {"sse4": 1, "avx8x2": 2, "avx512": 3, "seq": 4, "tree": 5}
VARIANTS = tuple(ORDERS) + ("ls_up", "ls_dn")


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def inputs(off, seed, level=300.0):
    """(t_loc, t_scale, p_loc, p_scale), float32 [off[-1]].  The prior is not
    the standard one, so the shard constants and rho matter."""
    rng = np.random.Generator(np.random.PCG64(seed))
    D = int(np.asarray(off)[-1])
    t_scale = (rng.uniform(0.5, 2.0, D) * level).astype(F32)
    t_loc = rng.standard_normal(D).astype(F32)
    p_loc = (0.1 * rng.standard_normal(D)).astype(F32)
    p_scale = rng.uniform(0.8, 1.25, D).astype(F32)
    return t_loc, t_scale, p_loc, p_scale


def certified_blocks(off, max_blocks=64):
    """The blocks a certificate covers: up to the max_blocks-th non-empty one."""
    full = np.flatnonzero(np.diff(np.asarray(off, np.int64)) > 0)
    return int(full[:max_blocks][-1]) + 1 if full.size else 0


def _gather(values, off, keep):
    """The blocks in ``keep`` as a layout of their own: the other blocks are
    emptied, so each block keeps its number, hence its seed.  Returns (offsets,
    the kept dims, the values on them)."""
    off = np.asarray(off, np.int64)
    sub = offsets(np.where(keep, np.diff(off), 0))
    dims = np.concatenate([np.arange(off[g], off[g + 1]) for g in np.flatnonzero(keep)] +
                          [np.zeros(0, np.int64)]).astype(np.int64)
    return sub, dims, tuple(np.ascontiguousarray(np.asarray(a, F32)[dims]) for a in values)


def declared(values, off, bits, n_steps, seed, rho, base, blocks=None):
    """oracle.greedy_encode on the blocks asked for (default: all), block g at
    ``bits[g]`` bits (``bits``: one count, or one per block) with seed ``seed +
    base + g``.  Returns (idx int32 [nb, n_steps], sample f32 [D]); rows and
    dims of blocks not asked for, and of empty ones, stay 0."""
    off = np.asarray(off, np.int64)
    nb = off.size - 1
    bits = np.full(nb, int(bits)) if np.ndim(bits) == 0 else np.asarray(bits, np.int64)
    want = np.diff(off) > 0
    if blocks is not None:
        only = np.zeros(nb, bool)
        only[np.asarray(blocks, np.int64)] = True
        want &= only
    idx = np.zeros((nb, n_steps), np.int32)
    sample = np.zeros(int(off[-1]), F32)
    for b in sorted(set(bits[want].tolist())):
        keep = want & (bits == b)
        sub, dims, (tl, ts, pl, ps) = _gather(values, off, keep)
        i, s = O.greedy_encode(tl, ts, pl, ps, sub, int(b), n_steps, seed, rho, base)
        idx[keep], sample[dims] = i[keep], s
    return idx, sample


def _variant_tables(values, off, keep, bits, n_steps, seed, rho, base):
    """The blocks in ``keep`` (all at ``bits`` bits) under every variant.
    Returns (vidx [nb, n_steps, V], gap [nb, n_steps], ls_up idx, ls_dn idx)."""
    sub, _, (tl, ts, pl, ps) = _gather(values, off, keep)
    vidx, _, gap, _ = O.greedy_encode_semvar(tl, ts, pl, ps, sub, bits, n_steps, seed, rho, base)
    lf = O.logf_table(ts)
    out = [vidx, gap]
    for to in (np.inf, -np.inf):
        ls = np.nextafter(lf, F32(to))
        out.append(O.greedy_encode_lsig(tl, ts, pl, ps, sub, bits, n_steps, seed, ls, rho, base)[0])
    return out


def certificate(values, off, bits, n_steps, seed, rho, base, max_blocks=64):
    """``values`` = inputs(off, ...); ``bits``: one count, or one per block.
    On the first max_blocks non-empty blocks (and the empty ones in between),
    from the oracle alone:

      flips     {variant: blocks whose index row differs from the declared one}
      ties      (block, step) pairs with best == second best and a declared index > 0
      distinct  distinct declared indices
      pairs     non-empty (block, step) pairs
      blocks    non-empty blocks
      declared  the declared indices [blocks covered, n_steps]
      tables    {variant: its indices, same shape}
    """
    off = np.asarray(off, np.int64)
    nb = certified_blocks(off, max_blocks)
    off = off[:nb + 1]
    values = tuple(np.asarray(a, F32)[:int(off[-1])] for a in values)
    full = np.diff(off) > 0
    bits = (np.full(nb, int(bits)) if np.ndim(bits) == 0 else np.asarray(bits, np.int64))[:nb]
    nv = len(O.sem_variant_names())
    vidx = np.zeros((nb, n_steps, nv), np.int32)
    gap = np.ones((nb, n_steps), np.float64)
    up = np.zeros((nb, n_steps), np.int32)
    dn = np.zeros((nb, n_steps), np.int32)
    for b in sorted(set(bits[full].tolist())):
        keep = full & (bits == b)
        for dst, src in zip((vidx, gap, up, dn),
                            _variant_tables(values, off, keep, int(b), n_steps, seed, rho, base)):
            dst[keep] = src[keep]
    base_idx = vidx[..., 0]
    tables = {name: vidx[..., v] for name, v in ORDERS.items()}
    tables["ls_up"], tables["ls_dn"] = up, dn
    return dict(
        flips={name: int((t != base_idx).any(axis=1).sum()) for name, t in tables.items()},
        ties=int(((gap == 0) & (base_idx > 0) & full[:, None]).sum()),
        distinct=int(np.unique(base_idx[full]).size),
        pairs=int(full.sum()) * n_steps, blocks=int(full.sum()),
        declared=base_idx, tables=tables)


@functools.lru_cache(maxsize=None)
def _probe(d):
    """Fixed pseudo-random rows of d dims: log-density-sized terms, and terms
    spread over six decades.  Two orders that differ at all differ on about
    one such row in four; 128 rows leave no doubt."""
    rng = np.random.Generator(np.random.PCG64(1000003 + d))
    rows = [(-6.0 - rng.uniform(0.0, 1.0, d)).astype(F32) for _ in range(64)]
    rows += [(rng.standard_normal(d) * 10.0 ** rng.uniform(-3, 3, d)).astype(F32)
             for _ in range(64)]
    return rows


def applicable(order, lengths):
    """Can this variant differ from the declared arithmetic at these block
    lengths?  Decided by the oracle alone: a row-sum order is applicable when
    its sum of some fixed pseudo-random row of one of the lengths is not the
    declared order's; the shifted normalisers always are."""
    if order in ("ls_up", "ls_dn"):
        return True
    o = ORDERS[order]
    return any(O.sem_rowsum(x, o) != O.sem_rowsum(x, 0)
               for d in sorted(set(int(n) for n in lengths if n > 0)) for x in _probe(d))
