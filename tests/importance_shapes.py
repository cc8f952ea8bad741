"""Shapes of tests/test_importance_paths_gpu.py, shared with
tests/test_importance_plan.py, which checks on the CPU that each shape takes
the paths its case names (csrc/cwq_imp_plan.h, DESIGN.md "Importance coder
paths").

A "blocks" case is one cwq_importance_encode launch (importance_encode_blocks:
counts passed directly, tile size and tile count found on the device).  A
"grouped" case is a latent for code_grouped_importance_sample, a "batch" case
a list of latents for code_grouped_importance_sample_batch; their counts follow
from the latents (grouped_plan), and the host knows the launch's totals.

Inputs come from one numpy generator per case, a standard-normal proposal,
target locs 0.7 N(0, 1) and target scales in [0.3, 0.95] unless the kind says
otherwise."""
import numpy as np

CPT_MIN, CPT_MAX = 1024, 16384
SMALL_N = 128


class Blocks:
    """One cwq_importance_encode launch: group lengths, counts, seed, base."""

    def __init__(self, name, sizes, counts, seed, base=0, kind="normal", rng_seed=0,
                 eps=2.0 ** -24, certify=None, lead=None):
        self.name, self.kind = name, kind
        # of the "near" kind (NEAR_TIE_CASES)
        self.eps, self.certify, self.lead = eps, certify, lead
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.counts = np.asarray(counts, dtype=np.int64)
        assert self.sizes.size == self.counts.size
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.seed, self.base, self.rng_seed = seed, base, rng_seed

    @property
    def oracle_counts(self):
        return np.maximum(self.counts, 1)

    def inputs(self):
        """(t_loc, t_scale, p_loc, p_scale) float32 [D]."""
        if self.kind == "near":      # rounding-sized gaps under a non-standard proposal
            import imp_near_ties
            return imp_near_ties.inputs(self.off, self.rng_seed, self.eps, self.lead)
        rng = np.random.default_rng(self.rng_seed)
        D = int(self.off[-1])
        tl = (rng.standard_normal(D) * 0.7).astype(np.float32)
        ts = rng.uniform(0.3, 0.95, D).astype(np.float32)
        pl = np.zeros(D, np.float32)
        ps = np.ones(D, np.float32)
        if self.kind == "ties":      # target == proposal: every score 0, index 0 wins
            tl[:], ts[:] = 0.0, 1.0
        elif self.kind == "flat":    # near-ties: the survivor list fills, rows go exact in line
            tl[:], ts[:] = 0.0, np.float32(1.0 - 2.0 ** -12)
        elif self.kind == "wide":    # sigma_q > sigma_p: the log ratio is convex in z
            ts = rng.uniform(1.0, 3.0, D).astype(np.float32)
        elif self.kind == "gate":    # one dim per group outside the value gate's range
            first = self.off[:-1][self.sizes > 0]
            ps[first] = np.float32(2.0 ** 70)
            ts[first] = np.float32(2.0 ** 69)
            tl[first] = (tl[first] * np.float32(2.0 ** 68)).astype(np.float32)
        else:
            assert self.kind == "normal", self.kind
        return tl, ts, pl, ps


# ---------------------------------------------------------------------------
# dyn_groups: dynamic, permuted hand-out by group count (4,096), static below
# ---------------------------------------------------------------------------
DYN_GROUPS_SEED, DYN_GROUPS_BASE = 2 ** 31 - 3, 5   # seed + base + g wraps int32
DYN_GROUPS_LONG = [3 * 1024 + 1, 3 * 1024 + 2, 4 * 1024, 5000, 2 * 1024 + 1, 2 * 1024]


def dyn_groups(nb):
    rng = np.random.default_rng(4096)
    sizes = rng.integers(1, 17, nb)
    counts = rng.integers(1, SMALL_N + 1, nb)
    big = rng.choice(nb, 64, replace=False)
    counts[big] = rng.integers(SMALL_N + 1, 5001, 64)
    counts[big[:len(DYN_GROUPS_LONG)]] = DYN_GROUPS_LONG
    return Blocks(f"dyn_groups_{nb}", sizes, counts, DYN_GROUPS_SEED, DYN_GROUPS_BASE,
                  rng_seed=40960 + nb)


DYN_GROUPS_NB = [4096, 4095]

# ---------------------------------------------------------------------------
# tiles_scan: k_imp_tiles' prefix, in registers (<= 16,384 groups) and streamed
# ---------------------------------------------------------------------------
TILES_SCAN_NB = [16384, 16385, 17409]


def tiles_scan_big_indices(nb):
    """Groups above 128 candidates: the first and last group of the launch, both
    sides of the first round's and of the register form's boundary, and one
    inside every round of 1,024, so every carry of the prefix lies under a tile."""
    idx = {0, 1023, 1024, 16383, nb - 1}
    if nb > 16384:
        idx.add(16384)
    for r in range((nb + 1023) // 1024):
        g = r * 1024 + 300 + 37 * r
        if g < nb:
            idx.add(g)
    return sorted(idx)


def tiles_scan(nb):
    rng = np.random.default_rng(nb)
    sizes = rng.integers(1, 9, nb)
    counts = rng.integers(1, 65, nb)
    big = tiles_scan_big_indices(nb)
    counts[big] = rng.integers(SMALL_N + 1, 3001, len(big))
    counts[0], counts[nb - 1] = 2 * 1024 + 5, 1024 + 1   # more than one tile at both ends
    return Blocks(f"tiles_scan_{nb}", sizes, counts, 77, 0, rng_seed=nb + 1)


# ---------------------------------------------------------------------------
# cpt_ladder: every tile size, chosen on the device
# ---------------------------------------------------------------------------
# (name, T, tile size)
CPT_LADDER = [("t21", 1 << 21, 1024), ("t21p", (1 << 21) + 1, 2048),
              ("t22p", (1 << 22) + 1, 4096), ("t23p", (1 << 23) + 1, 8192),
              ("t24p", (1 << 24) + 1, 16384)]
CPT_LADDER_DIMS = [7, 3, 16, 1, 5, 9, 2, 12, 6, 4]
CPT_LADDER_FILLERS = 16


def cpt_ladder_counts(c):
    """Around the tile size c: the last tile of c + 1 .. c + 3 holds one to three
    rows (some waves get none); 128 and 129 are the small-group threshold."""
    return [c - 1, c, c + 1, c + 2, c + 3, 2 * c, 2 * c + 1, 3 * c - 1, 128, 129]


# near-ties at tiles above the survivor list's 1,024 rows: the list overflows
# and rows are scored exactly in line (a 1,024-row tile can only fill it)
CPT_LADDER_NEAR_TIES = [("t21p", "flat"), ("t22p", "ties"), ("t24p", "flat")]


def cpt_ladder(name, kind="normal"):
    T, c = next((t, c) for n, t, c in CPT_LADDER if n == name)
    rng = np.random.default_rng(T % 1000 + c)
    head = cpt_ladder_counts(c)
    rest = T - sum(head)
    per = rest // CPT_LADDER_FILLERS
    fill = [per] * (CPT_LADDER_FILLERS - 1) + [rest - per * (CPT_LADDER_FILLERS - 1)]
    fdims = list(rng.integers(1, 5, CPT_LADDER_FILLERS))
    # fillers between the ladder's groups, not after them
    sizes, counts = [], []
    for i in range(max(len(head), len(fill))):
        if i < len(fill):
            sizes.append(fdims[i]); counts.append(fill[i])
        if i < len(head):
            sizes.append(CPT_LADDER_DIMS[i]); counts.append(head[i])
    assert sum(counts) == T
    return Blocks(f"cpt_ladder_{name}_{kind}", sizes, counts, 2024, 1, kind=kind, rng_seed=c)


# ---------------------------------------------------------------------------
# near ties: one case per scoring path, certified by tests/test_imp_near_ties.py
# ---------------------------------------------------------------------------
NT_SEED, NT_BASE = 2 ** 31 - 4, 5       # seed + base + g wraps int32 in every case
# (input rng seed, eps) of each case: chosen on the CPU so that the oracle alone
# meets the certificate's conditions (tests/test_imp_near_ties.py)
NT_LEVELS = {"nt_small": (1, 2.0 ** -24), "nt_short": (1, 2.0 ** -24),
             "nt_pruned": (1, 2.0 ** -25), "nt_tiles": (1, 2.0 ** -24),
             "nt_exact": (3, 2.0 ** -27), "nt_overflow": (1, 2.0 ** -26),
             "nt_sum": (7, 2.0 ** -24)}
# nt_sum: every group's first dim has the target N(p_loc, p_scale / 7.5): scores
# of log 7.5 = 2.01 and rounding-sized gaps at 60,000 rows (imp_near_ties.inputs)
NT_SUM_LEAD, NT_SUM_ROWS = 7.5, 60000
NT_OVERFLOW_LADDER = [2 * i + 1 for i in range(len(CPT_LADDER_DIMS))]  # cpt_ladder's head groups


def _nt_draw(name, nb, dims, counts, always=()):
    """nb groups with lengths and counts drawn from the given values; the
    counts in ``always`` (and every length) occur at least once."""
    rng = np.random.default_rng(sum(map(ord, name)))
    sizes = rng.choice(dims, nb)
    sizes[:len(dims)] = dims
    ns = rng.choice(counts, nb) if not isinstance(counts, range) else \
        rng.integers(counts.start, counts.stop, nb)
    ns[nb - len(always):] = always
    perm = rng.permutation(nb)
    return sizes[perm], ns[perm]


def near_tie_case(name):
    rng_seed, eps = NT_LEVELS[name]
    kw = dict(kind="near", rng_seed=rng_seed, eps=eps)
    if name == "nt_overflow":
        c = cpt_ladder("t21p", "near")
        return Blocks(name, c.sizes, c.counts, NT_SEED, NT_BASE, certify=NT_OVERFLOW_LADDER, **kw)
    if name == "nt_sum":        # scores above 1 (a lead dim): the order of the row sum shows
        sizes, counts = _nt_draw(name, 64, [9, 33, 100], [NT_SUM_ROWS])
        return Blocks(name, sizes, counts, NT_SEED, NT_BASE, lead=NT_SUM_LEAD, **kw)
    if name == "nt_small":      # k_imp_small; a few groups of one and two candidates
        sizes, counts = _nt_draw(name, 64, list(range(1, 17)), [63, 64, 65, 127, 128],
                                 always=[1, 1, 2, 2, 63, 64, 65, 127, 128])
    elif name == "nt_short":    # short screened form
        sizes, counts = _nt_draw(name, 48, [1, 2, 3, 4], range(129, 1025), always=[129, 1024])
    elif name == "nt_pruned":   # pruned screened form
        sizes, counts = _nt_draw(name, 48, [5, 8, 9, 32, 100, 256], range(129, 1025),
                                 always=[129, 1024])
    elif name == "nt_tiles":    # two to four 1,024-row tiles per group
        sizes, counts = _nt_draw(name, 32, [3, 8, 33], [1025, 2085, 3072, 3073],
                                 always=[1025, 2085, 3072, 3073])
    else:                       # exact rows by length
        assert name == "nt_exact", name
        sizes, counts = _nt_draw(name, 16, [257, 300], [129, 1500], always=[129, 1500])
    return Blocks(name, sizes, counts, NT_SEED, NT_BASE, **kw)


NEAR_TIE_CASES = ["nt_small", "nt_short", "nt_pruned", "nt_tiles", "nt_exact", "nt_overflow",
                  "nt_sum"]


# ---------------------------------------------------------------------------
# row_lengths: every row form at each side of its length thresholds
# ---------------------------------------------------------------------------
ROW_LENGTHS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 255, 256, 257, 300, 1025]
ROW_COUNTS = [129, 1500, 2 * 1024 + 37]
ROW_KINDS = ["normal", "ties", "flat", "wide", "gate"]


def row_lengths(kind):
    # the non-empty lengths in a fixed shuffled order; the three empty groups
    # (length 0, one per count) land between non-empty ones
    mixed = [int(x) for x in np.random.default_rng(5).permutation(ROW_LENGTHS[1:])]
    sizes, counts = [], []
    for i, L in enumerate(mixed):
        for n in ROW_COUNTS:
            sizes.append(L); counts.append(n)
        if i in (2, 8, 13):
            sizes.append(0); counts.append(ROW_COUNTS[(2, 8, 13).index(i)])
    return Blocks(f"row_lengths_{kind}", sizes, counts, 31337, 2, kind=kind,
                  rng_seed=sum(map(ord, kind)))


# ---------------------------------------------------------------------------
# counts_edge: counts below 1 are coded as one candidate
# ---------------------------------------------------------------------------
def counts_edge():
    counts = [50, 0, 129, -1, 700, -2 ** 31, 3000, 1, 2, 128, 0, 2049]
    sizes = [3, 5, 7, 2, 9, 4, 1, 6, 8, 16, 0, 5]
    return Blocks("counts_edge", sizes, counts, -7, 0, rng_seed=99)


# ---------------------------------------------------------------------------
# hi_counters: Philox block indices at and past 2^32
# ---------------------------------------------------------------------------
HI_DECODE_D = [255, 256]


def hi_first_row(d):
    """First row of a d-dim group with a Philox block index of 2^32 or more."""
    return -((-(1 << 34)) // d)


def hi_decode_rows(d):
    n = hi_first_row(d)
    rows = [n - 1, n, n + 1, (1 << 34) // d, (1 << 30) - 1]
    return rows


HI_ENCODE_D = 256
HI_ENCODE_N = (1 << 26) + (1 << 24)      # N d = 1.25 * 2^34: the screening loop's 64-bit form
# the first seed from 1 whose exact-mode winner lies past row 2^26 (asserted on the GPU)
HI_ENCODE_SEED = 18
HI_ENCODE_WINNER = 77557693


def hi_encode():
    return Blocks("hi_encode", [HI_ENCODE_D], [HI_ENCODE_N], HI_ENCODE_SEED, 0, rng_seed=2 ** 26)


# ---------------------------------------------------------------------------
# grouped and batch calls: counts follow from the latents
# ---------------------------------------------------------------------------
def _latent(rng, spec, t_scale=0.8):
    """Latent (q_loc, q_scale, p_loc, p_scale) whose standardised target has the
    per-dim KL (nats) against N(0, 1) drawn uniformly from each (n_dims, lo, hi)
    of spec: KL = (ts^2 + tl^2 - 1) / 2 - ln ts."""
    kl = np.concatenate([rng.uniform(lo, hi, n) for n, lo, hi in spec])
    c = 0.5 * (t_scale ** 2 - 1.0) - np.log(t_scale)
    tl = np.sqrt(2.0 * (kl - c)) * rng.choice([-1.0, 1.0], kl.size)
    p_loc = (0.5 * rng.standard_normal(kl.size)).astype(np.float32)
    p_scale = rng.choice([0.5, 1.0, 2.0], kl.size).astype(np.float32)   # exact rescale
    q_loc = (p_loc + p_scale * tl.astype(np.float32)).astype(np.float32)
    q_scale = (p_scale * np.float32(t_scale)).astype(np.float32)
    return q_loc, q_scale, p_loc, p_scale


# dyn_tiles: 9 bits per group close a group at 5.238 nats; four dims of 1.25 to
# 1.30 nats (or eight of 0.62 to 0.65) reach 4.96 to 5.2 and a further dim
# would pass the limit, so every group draws 143 to 182 candidates: one tile
# each, just above the 128 of k_imp_small.
DYN_TILES_BITS = 9
DYN_TILES_SINGLE = (4200, 4100, 8192)      # (4-dim groups, 8-dim groups, rng seed)
DYN_TILES_BATCH = [(1500, 1400, 1), (1300, 1500, 2), (0, 1, 3), (1400, 1300, 4)]
DYN_TILES_BATCH_SEEDS = [11, 2 ** 31 - 2, -3, 12]


def dyn_tiles_latent(n4, n8, seed):
    rng = np.random.default_rng(seed)
    return _latent(rng, [(4 * n4, 1.25, 1.30), (8 * n8, 0.62, 0.65)])


# cpt_grouped: 21 bits per group close a group at 13.556 nats; four dims of 3.25
# to 3.35 (eight of 1.63 to 1.67) make groups of 4.4e5 to 6.6e5 candidates, and
# 40 of them more than 2^24: the host picks the 16,384 tile (CPT_MAX).
CPT_GROUPED_BITS = 21
CPT_GROUPED_SEED = 4242


def cpt_grouped_latent():
    rng = np.random.default_rng(21)
    return _latent(rng, [(4 * 20, 3.25, 3.35), (8 * 20, 1.63, 1.67)])


def grouped_plan(oracle, latent, n_bits_per_group, max_group_size_bits=4, dim_kl_bit_limit=12):
    """(group starts with D appended, counts) of one item, as
    oracle.code_grouped_importance_sample plans it."""
    ql, qs, pl, ps = latent
    tl, ts = oracle.standardise(ql, qs, pl, ps)
    kl_bits = oracle.kl_normal_normal(ql, qs, pl, ps) / np.float32(np.log(2))
    keep = kl_bits <= dim_kl_bit_limit
    tl = np.where(keep, tl, np.float32(0)).astype(np.float32)
    ts = np.where(keep, ts, np.float32(1)).astype(np.float32)
    D = tl.size
    kl = oracle.kl_normal_normal(tl, ts, np.zeros(D, np.float32), np.ones(D, np.float32))
    starts = oracle.importance_group_starts(kl, n_bits_per_group, max_group_size_bits)
    return np.asarray(starts, np.int64), oracle.importance_plan(kl, starts)
