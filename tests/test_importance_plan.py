"""The importance coder's launch plan (csrc/cwq_imp_plan.h, DESIGN.md
"Importance coder paths") on the host: which of its paths a launch of a given
shape takes.

Every path is bit-exact by design, so the GPU tests, which compare outputs with
the oracle, cannot see a shape being rerouted.  These tests can: the thresholds
from both sides, and for every case of tests/importance_shapes.py the paths the
case is there to reach (tests/test_importance_paths_gpu.py runs them)."""
import ctypes

import numpy as np
import pytest

import importance_shapes as S

SMALL, PRUNED, SHORT, EXACT = range(4)
HI0 = 0x80
I64 = ctypes.c_int64
P64 = ctypes.POINTER(I64)


@pytest.fixture(scope="module")
def mc(mathcheck):
    mathcheck.mc_importance_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, I64, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, P64, ctypes.c_void_p]
    mathcheck.mc_importance_plan.restype = None
    mathcheck.mc_importance_tile_count.argtypes = [ctypes.c_void_p, I64, I64]
    mathcheck.mc_importance_tile_count.restype = I64
    mathcheck.mc_importance_cand_per_tile.argtypes = [I64]
    mathcheck.mc_importance_cand_per_tile.restype = I64
    mathcheck.mc_importance_consts.argtypes = [P64]
    mathcheck.mc_importance_consts.restype = None
    return mathcheck


FIELDS = ("T", "cpt", "tiles", "small", "dynamic", "permuted", "multiplier", "per_block",
          "cpt_max", "in_regs")


def plan(mc, counts, off=None, *, known=False, per_block=False, screen=1):
    """The plan of one launch as a dict, plus "forms" (per group) when the
    group offsets are given.  known: the grouped and batch calls, which pass the
    launch's totals; else cwq_importance_encode."""
    ns = np.ascontiguousarray(np.asarray(counts, dtype=np.int64))
    nb = ns.size
    out = (I64 * 10)()
    forms = np.zeros(max(nb, 1), np.uint8)
    o = None if off is None else np.ascontiguousarray(np.asarray(off, dtype=np.int64))
    assert o is None or o.size == nb + 1
    mc.mc_importance_plan(ns.ctypes.data, None if o is None else o.ctypes.data, nb, int(known),
                          int(per_block), screen, out, None if o is None else forms.ctypes.data)
    p = dict(zip(FIELDS, out))
    for k in ("dynamic", "permuted", "per_block", "cpt_max", "in_regs"):
        p[k] = bool(p[k])
    if o is not None:
        p["forms"] = forms[:nb]
    # importance_tile_count (the launcher's hand-out argument) is the same count
    assert mc.mc_importance_tile_count(ns.ctypes.data, nb, p["T"]) == p["tiles"]
    assert p["permuted"] == (p["multiplier"] != 1)
    return p


def form(mc, count, d, screen=1):
    return int(plan(mc, [count], [0, d], screen=screen)["forms"][0])


def want_forms(case, screen=1):
    """Each group's row form and HI0 flag from the issue's wording, not from
    the header: small up to 128 candidates; else pruned for 5 to 256 dims,
    short for 1 to 4, exact for 0 or more than 256 (or with screening off)."""
    out = []
    for n, d in zip(case.oracle_counts, case.sizes):
        n, d = int(n), int(d)
        if n <= 128:
            f = SMALL
        elif not screen or d == 0 or d > 256:
            f = EXACT
        else:
            f = PRUNED if d >= 5 else SHORT
        out.append(f | (HI0 if n * d <= 2 ** 34 else 0))
    return np.array(out, np.uint8)


def check_blocks(mc, case, *, cpt, dynamic, in_regs=True):
    """A cwq_importance_encode launch: totals unknown to the host, so seeds are
    seed + base + g and CPT_MAX is off."""
    for screen in (1, 0):
        p = plan(mc, case.counts, case.off, screen=screen)
        assert p["T"] == int(case.oracle_counts.sum())
        assert (p["cpt"], p["dynamic"], p["permuted"], p["in_regs"]) == \
            (cpt, dynamic, dynamic, in_regs), (case.name, p)
        assert (p["per_block"], p["cpt_max"]) == (False, False)
        assert p["small"] == int((case.oracle_counts <= 128).sum())
        assert p["tiles"] == sum(-(-int(n) // cpt) for n in case.oracle_counts if n > 128)
        assert np.array_equal(p["forms"], want_forms(case, screen)), case.name
    return plan(mc, case.counts, case.off)


# ---------------------------------------------------------------------------
# constants and thresholds, both sides
# ---------------------------------------------------------------------------
def test_constants(mc):
    c = (I64 * 10)()
    mc.mc_importance_consts(c)
    assert list(c) == [128, 1024, 16384, 2048, 4096, 8192, 16384, 5, 256, 1024]
    assert (S.SMALL_N, S.CPT_MIN, S.CPT_MAX) == (c[0], c[1], c[2])


def test_small_group_threshold(mc):
    for d in (1, 7, 300):
        assert form(mc, 128, d) & 3 == SMALL and form(mc, 129, d) & 3 != SMALL
    p = plan(mc, [128, 129, 0, -5, 1], [0, 3, 6, 9, 12, 15])
    assert (p["small"], p["tiles"], p["T"]) == (4, 1, 128 + 129 + 3)


def test_handout_thresholds(mc):
    one_tile = [129]
    # by group count when the host does not know the tile count
    for counts in ([1], one_tile):
        assert not plan(mc, counts * 4095)["dynamic"]
        assert plan(mc, counts * 4096)["dynamic"]
    # ... by tile count when it does, whatever the group count
    assert not plan(mc, one_tile * 8191, known=True)["dynamic"]
    assert plan(mc, one_tile * 8192, known=True)["dynamic"]
    assert plan(mc, [8192 * 16384], known=True)["dynamic"]         # one group, 8,192 tiles
    assert not plan(mc, [8191 * 16384], known=True)["dynamic"]
    assert not plan(mc, [1] * 20000, known=True)["dynamic"]          # no tile at all
    # the permutation: dynamic launches of more than one tile
    assert plan(mc, one_tile * 8192, known=True)["multiplier"] == (2 ** 31 - 1) % 8192
    assert plan(mc, [1] * 4095 + [129])["multiplier"] == 1         # dynamic, one tile
    assert plan(mc, [1] * 4096)["multiplier"] == 1                  # dynamic, no tile
    assert plan(mc, one_tile * 4095)["multiplier"] == 1             # static
    p = plan(mc, [1] * 4094 + [129, 1025])
    assert p["dynamic"] and p["tiles"] == 3 and p["multiplier"] == (2 ** 31 - 1) % 3


def test_prefix_kernel_threshold(mc):
    assert plan(mc, [1] * 16384)["in_regs"] and not plan(mc, [1] * 16385)["in_regs"]
    assert plan(mc, [1])["in_regs"] and not plan(mc, [1] * 17409)["in_regs"]


def test_row_form_thresholds(mc):
    n = 5000
    assert [form(mc, n, d) & 3 for d in (0, 1, 4, 5, 256, 257, 1025)] == \
        [EXACT, SHORT, SHORT, PRUNED, PRUNED, EXACT, EXACT]
    assert [form(mc, n, d, screen=0) & 3 for d in (0, 1, 4, 5, 256, 257)] == [EXACT] * 6
    assert form(mc, 100, 5, screen=0) & 3 == SMALL


def test_counter_width_threshold(mc):
    """HI0 (32-bit Philox block index in the screening Box-Muller) while
    N d <= 2^34."""
    assert form(mc, 2 ** 26, 256) == PRUNED | HI0
    assert form(mc, 2 ** 26 + 1, 256) == PRUNED
    assert form(mc, 2 ** 32, 4) == SHORT | HI0 and form(mc, 2 ** 32 + 1, 4) == SHORT
    assert 2 ** 34 % 255 == 4
    assert form(mc, 2 ** 34 // 255, 255) == PRUNED | HI0   # N d = 2^34 - 4
    assert form(mc, 2 ** 34 // 255 + 1, 255) == PRUNED     # N d = 2^34 + 251
    assert form(mc, 2 ** 34, 1) == SHORT | HI0 and form(mc, 2 ** 34 + 1, 1) == SHORT


def test_tile_size_at_each_power_of_two(mc):
    for lg, cpt in ((21, 1024), (22, 2048), (23, 4096), (24, 8192)):
        T = 1 << lg
        assert mc.mc_importance_cand_per_tile(T) == cpt
        assert mc.mc_importance_cand_per_tile(T + 1) == 2 * cpt
        # as a launch, with the host knowing T and not
        for known in (False, True):
            at, above = plan(mc, [T], known=known), plan(mc, [T, 1], known=known)
            assert (at["cpt"], at["tiles"]) == (cpt, 2048)
            assert (above["cpt"], above["tiles"]) == (2 * cpt, 1024)
            assert not at["cpt_max"] and above["cpt_max"] == (known and lg == 24)
    for T in (0, 1, 1 << 20, (1 << 21) - 1):
        assert mc.mc_importance_cand_per_tile(T) == 1024
    for T in ((1 << 25), (1 << 40)):
        assert mc.mc_importance_cand_per_tile(T) == 16384
    assert plan(mc, [1 << 25], known=True, per_block=True)["per_block"]


# ---------------------------------------------------------------------------
# the cases of importance_shapes.py
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nb", S.DYN_GROUPS_NB)
def test_dyn_groups_shapes(mc, nb):
    case = S.dyn_groups(nb)
    p = check_blocks(mc, case, cpt=1024, dynamic=(nb == 4096))
    assert (p["multiplier"] != 1) == (nb == 4096)
    n, d = case.counts, case.sizes
    assert d.min() == 1 and d.max() == 16 and n.min() >= 1
    big = n > 128
    assert int(big.sum()) == 64 and n.max() <= 5000
    assert int((n > 2 * 1024).sum()) >= 4           # three tiles or more
    assert set(S.DYN_GROUPS_LONG) <= set(n.tolist())
    # both screened row forms lie under tiles
    kinds = set((p["forms"][big] & 3).tolist())
    assert kinds == {PRUNED, SHORT}
    # seed + base + g wraps int32 inside the launch
    assert case.seed < 2 ** 31 <= case.seed + case.base + nb - 1


@pytest.mark.parametrize("nb", S.TILES_SCAN_NB)
def test_tiles_scan_shapes(mc, nb):
    case = S.tiles_scan(nb)
    p = check_blocks(mc, case, cpt=1024, dynamic=True, in_regs=(nb <= 16384))
    big = np.nonzero(case.counts > 128)[0]
    assert big.tolist() == S.tiles_scan_big_indices(nb)
    for g in (0, 1023, 1024, 16383, nb - 1):
        assert g in big
    assert (16384 in big) == (nb > 16384)
    rounds = (nb + 1023) // 1024
    assert rounds == {16384: 16, 16385: 17, 17409: 18}[nb]
    # every round's total is non-zero (a tile lies above every carry), except a
    # last round of one group, whose group is the launch's last
    assert set((big // 1024).tolist()) == set(range(rounds))
    assert case.counts[case.counts <= 128].max() <= 64
    assert p["tiles"] > len(big)


@pytest.mark.parametrize("name,T,cpt", S.CPT_LADDER)
def test_cpt_ladder_shapes(mc, name, T, cpt):
    case = S.cpt_ladder(name)
    p = check_blocks(mc, case, cpt=cpt, dynamic=False)
    assert p["T"] == T
    counts = case.counts.tolist()
    for n in S.cpt_ladder_counts(cpt):
        assert n in counts
    fill = [(n, d) for n, d in zip(counts, case.sizes) if n not in S.cpt_ladder_counts(cpt)]
    assert len(fill) >= 16 and all(1 <= d <= 4 for _, d in fill)
    if name == "t21":    # exactly 2^21: one candidate more doubles the tile
        assert mc.mc_importance_cand_per_tile(T + 1) == 2 * cpt
    else:                # a little above a power of two: that power takes half the tile
        assert T - 1 == 1 << (T - 1).bit_length() - 1
        assert mc.mc_importance_cand_per_tile(T - 1) == cpt // 2


@pytest.mark.parametrize("name,kind", S.CPT_LADDER_NEAR_TIES)
def test_cpt_ladder_near_ties_shapes(mc, name, kind):
    """The same launches with every score (nearly) equal: each tile holds more
    rows than the survivor list, so the list overflows."""
    case = S.cpt_ladder(name, kind)
    cpt = dict((n, c) for n, _, c in S.CPT_LADDER)[name]
    p = check_blocks(mc, case, cpt=cpt, dynamic=False)
    c = (I64 * 10)()
    mc.mc_importance_consts(c)
    assert cpt > c[9] and int((case.counts > c[9]).sum()) >= 16
    assert {PRUNED | HI0, SHORT | HI0} <= set(p["forms"].tolist())
    tl, ts, pl, ps = case.inputs()
    assert np.unique(tl).size == 1 and np.unique(ts).size == 1


def test_cpt_grouped_shape(mc, oracle):
    """The grouped call on a latent of more than 2^24 candidates: the host
    knows T and picks k_imp_eval<false, true>."""
    starts, ns = S.grouped_plan(oracle, S.cpt_grouped_latent(), S.CPT_GROUPED_BITS)
    p = plan(mc, ns, starts, known=True)
    assert p["T"] > 1 << 24 and p["cpt"] == 16384
    assert (p["per_block"], p["cpt_max"], p["dynamic"]) == (False, True, False)
    assert {PRUNED | HI0, SHORT | HI0} <= set(p["forms"].tolist())
    assert int((ns > 16384).sum()) >= 38             # multi-tile groups
    # the step-by-step path runs the same groups with the tile chosen on the device
    q = plan(mc, ns, starts)
    assert (q["cpt"], q["cpt_max"], q["tiles"]) == (16384, False, p["tiles"])


def test_dyn_tiles_shapes(mc, oracle):
    """Host-known tile counts of at least 8,192, in one item and in a batch."""
    starts, ns = S.grouped_plan(oracle, S.dyn_tiles_latent(*S.DYN_TILES_SINGLE), S.DYN_TILES_BITS)
    p = plan(mc, ns, starts, known=True)
    assert p["tiles"] >= 8192 and p["dynamic"] and p["multiplier"] != 1
    assert (p["cpt"], p["per_block"], p["cpt_max"]) == (1024, False, False)
    assert int((ns > 1024).sum()) == 0               # one tile each
    assert {PRUNED | HI0, SHORT | HI0} <= set(p["forms"].tolist())
    # the batch: every item below the threshold on its own, the launch above it
    assert len(S.DYN_TILES_BATCH) >= 3
    all_ns, all_sizes, each = [], [], []
    for item in S.DYN_TILES_BATCH:
        st, n = S.grouped_plan(oracle, S.dyn_tiles_latent(*item), S.DYN_TILES_BITS)
        each.append(plan(mc, n, st, known=True)["tiles"])
        all_ns += n.tolist()
        all_sizes += np.diff(st).tolist()
    assert max(each) < 8192
    off = np.concatenate([[0], np.cumsum(all_sizes)])
    b = plan(mc, all_ns, off, known=True, per_block=True)
    assert b["tiles"] == sum(each) >= 8192 and b["dynamic"] and b["multiplier"] != 1
    assert (b["cpt"], b["per_block"], b["cpt_max"]) == (1024, True, False)


@pytest.mark.parametrize("kind", S.ROW_KINDS)
def test_row_lengths_shapes(mc, kind):
    case = S.row_lengths(kind)
    p = check_blocks(mc, case, cpt=1024, dynamic=False)
    assert sorted(set(case.sizes.tolist())) == S.ROW_LENGTHS
    for L in S.ROW_LENGTHS:
        assert sorted(case.counts[case.sizes == L].tolist()) == S.ROW_COUNTS, L
    assert case.counts.min() > 128 and p["small"] == 0
    # one, two and three tiles per length
    assert [-(-n // 1024) for n in S.ROW_COUNTS] == [1, 2, 3]
    # empty groups between non-empty ones
    empty = np.nonzero(case.sizes == 0)[0]
    assert all(0 < g < case.sizes.size - 1 and case.sizes[g - 1] > 0 and case.sizes[g + 1] > 0
               for g in empty)
    by_len = {int(d): int(f) & 3 for d, f in zip(case.sizes, p["forms"])}
    assert by_len == {0: EXACT, 1: SHORT, 2: SHORT, 3: SHORT, 4: SHORT, 5: PRUNED, 6: PRUNED,
                      7: PRUNED, 8: PRUNED, 9: PRUNED, 63: PRUNED, 64: PRUNED, 65: PRUNED,
                      255: PRUNED, 256: PRUNED, 257: EXACT, 300: EXACT, 1025: EXACT}
    if kind == "gate":   # one dim per non-empty group outside [2^-60, 2^60]
        tl, ts, pl, ps = case.inputs()
        for a, b in zip(case.off[:-1], case.off[1:]):
            assert b == a or int((ps[a:b] > 2.0 ** 60).sum()) == 1


def test_counts_edge_shapes(mc):
    case = S.counts_edge()
    p = check_blocks(mc, case, cpt=1024, dynamic=False)
    for n in (0, -1, -2 ** 31, 1, 2):
        assert n in case.counts.tolist()
    assert case.oracle_counts.min() == 1 and p["small"] >= 5 and p["tiles"] >= 4


def test_hi_counters_shapes(mc):
    for d in S.HI_DECODE_D:
        n = S.hi_first_row(d)
        assert n * d >= 2 ** 34 > (n - 1) * d
        rows = S.hi_decode_rows(d)
        assert {n - 1, n, n + 1, 2 ** 30 - 1} <= set(rows)
        if d == 255:   # a row whose blocks lie on both sides of index 2^32
            r = rows[3]
            assert r * d < 2 ** 34 < r * d + d - 1
    case = S.hi_encode()
    p = check_blocks(mc, case, cpt=16384, dynamic=False)
    assert int(p["forms"][0]) == PRUNED                # HI0 off
    assert int(case.counts[0]) * S.HI_ENCODE_D > 2 ** 34
    assert p["tiles"] == S.HI_ENCODE_N // 16384


# ---------------------------------------------------------------------------
# the near-tie cases (tests/test_imp_near_ties.py certifies their inputs,
# tests/test_imp_near_ties_gpu.py runs them): each takes the path it names
# ---------------------------------------------------------------------------
def _nt(mc, name, cpt=1024):
    case = S.near_tie_case(name)
    assert case.kind == "near" and (case.seed, case.base) == (2 ** 31 - 4, 5)
    return case, check_blocks(mc, case, cpt=cpt, dynamic=False)


def test_near_tie_cases_are_listed():
    assert S.NEAR_TIE_CASES == ["nt_small", "nt_short", "nt_pruned", "nt_tiles", "nt_exact",
                                "nt_overflow", "nt_sum"]
    assert set(S.NT_LEVELS) == set(S.NEAR_TIE_CASES)


def test_nt_small_shape(mc):
    case, p = _nt(mc, "nt_small")
    assert case.sizes.size == 64 and sorted(set(case.sizes.tolist())) == list(range(1, 17))
    assert sorted(set(case.counts.tolist())) == [1, 2, 63, 64, 65, 127, 128]
    assert (p["small"], p["tiles"]) == (64, 0)                # k_imp_small codes every group
    assert set((p["forms"] & 3).tolist()) == {SMALL}
    assert int((case.counts <= 2).sum()) <= 4                 # the rest can spread their winners


def test_nt_short_shape(mc):
    case, p = _nt(mc, "nt_short")
    assert case.sizes.size == 48 and sorted(set(case.sizes.tolist())) == [1, 2, 3, 4]
    assert case.counts.min() == 129 and case.counts.max() == 1024
    assert set(p["forms"].tolist()) == {SHORT | HI0}
    c = (I64 * 10)()
    mc.mc_importance_consts(c)
    # one tile per group and no more rows than the survivor list holds: every
    # survivor is re-scored from the list
    assert (p["small"], p["tiles"]) == (0, 48) and case.counts.max() <= c[9]


def test_nt_pruned_shape(mc):
    case, p = _nt(mc, "nt_pruned")
    assert case.sizes.size == 48 and sorted(set(case.sizes.tolist())) == [5, 8, 9, 32, 100, 256]
    assert case.counts.min() == 129 and case.counts.max() == 1024
    assert set(p["forms"].tolist()) == {PRUNED | HI0} and (p["small"], p["tiles"]) == (0, 48)


def test_nt_tiles_shape(mc):
    case, p = _nt(mc, "nt_tiles")
    assert case.sizes.size == 32 and sorted(set(case.sizes.tolist())) == [3, 8, 33]
    assert sorted(set(case.counts.tolist())) == [1025, 2085, 3072, 3073]
    assert set(p["forms"].tolist()) == {SHORT | HI0, PRUNED | HI0}
    tiles = [-(-int(n) // 1024) for n in case.counts]
    assert set(tiles) == {2, 3, 4} and p["tiles"] == sum(tiles)
    # both screened forms under two, three and four tiles
    for f in (SHORT, PRUNED):
        assert {t for t, g in zip(tiles, p["forms"]) if g & 3 == f} == {2, 3, 4}


def test_nt_exact_shape(mc):
    case, p = _nt(mc, "nt_exact")
    assert case.sizes.size == 16 and sorted(set(case.sizes.tolist())) == [257, 300]
    assert sorted(set(case.counts.tolist())) == [129, 1500]
    assert set(p["forms"].tolist()) == {EXACT | HI0}          # with screening on: by length
    assert case.sizes.min() > 256 and p["small"] == 0
    for d in (257, 300):
        assert set(case.counts[case.sizes == d].tolist()) == {129, 1500}


def test_nt_overflow_shape(mc):
    case, p = _nt(mc, "nt_overflow", cpt=2048)
    ladder = S.cpt_ladder("t21p")
    assert np.array_equal(case.sizes, ladder.sizes) and np.array_equal(case.counts, ladder.counts)
    assert p["T"] == 2 ** 21 + 1
    c = (I64 * 10)()
    mc.mc_importance_consts(c)
    assert p["cpt"] > c[9]                                    # a tile outgrows the survivor list
    assert case.sizes[case.certify].tolist() == S.CPT_LADDER_DIMS
    assert case.counts[case.certify].tolist() == S.cpt_ladder_counts(2048)
    assert int((case.counts[case.certify] > c[9]).sum()) >= 8
    assert {PRUNED | HI0, SHORT | HI0} <= set(p["forms"][case.certify].tolist())


def test_nt_sum_shape(mc):
    case, p = _nt(mc, "nt_sum", cpt=2048)
    assert case.sizes.size == 64 and sorted(set(case.sizes.tolist())) == [9, 33, 100]
    assert set(case.counts.tolist()) == {S.NT_SUM_ROWS} and case.lead == S.NT_SUM_LEAD
    assert set(p["forms"].tolist()) == {PRUNED | HI0}
    assert p["tiles"] == 64 * -(-S.NT_SUM_ROWS // 2048) and p["small"] == 0   # 30 tiles a group
