"""Every path a launch of the importance coder can take (csrc/cwq_imp_plan.h,
DESIGN.md "Importance coder paths"), each on a small shape that provably takes
it (tests/test_importance_plan.py checks that on the CPU) and compared bit for
bit with the CPU oracle, in prune_mode 0 (every row exact) and 2 (screened)."""
import numpy as np
import pytest
import torch

import importance_shapes as S

pytestmark = pytest.mark.gpu
MODES = [0, 2]


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    import compression_without_quantization_amd.coded_importance_sampler as I
    I.VERBOSE = False
    return C


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _assert_bits_equal(got, want, what):
    g, w = _u32(got), _u32(want)
    assert g.size == w.size, what
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {w.size} differ, first at {bad[:8]}"


_REF = {}


def _oracle_blocks(oracle, case):
    """The oracle's (indices, samples) of a blocks case, computed once."""
    if case.name not in _REF:
        tl, ts, pl, ps = case.inputs()
        wi, ws = oracle.importance_encode(tl, ts, pl, ps, case.off, case.oracle_counts,
                                          case.seed, case.base)
        wi.setflags(write=False)
        ws.setflags(write=False)
        _REF[case.name] = (wi, ws)
    return _REF[case.name]


def _encode(cwq, case, mode):
    tl, ts, pl, ps = case.inputs()
    gi, gs = cwq.importance_encode_blocks(tl, ts, pl, ps, case.off, case.counts, case.seed,
                                          block_id_base=case.base, prune_mode=mode)
    return gi.cpu().numpy(), gs.cpu().numpy()


def _check_blocks(cwq, oracle, case, mode, decode=False):
    wi, ws = _oracle_blocks(oracle, case)
    gi, gs = _encode(cwq, case, mode)
    bad = np.nonzero(gi != wi)[0]
    assert bad.size == 0, (f"{case.name}, prune_mode {mode}: {bad.size} of {wi.size} indices "
                           f"differ, first groups {bad[:8]} (counts {case.counts[bad[:8]]}, "
                           f"dims {case.sizes[bad[:8]]})")
    _assert_bits_equal(gs, ws, f"{case.name}, prune_mode {mode}: samples")
    if decode:
        _, _, pl, ps = case.inputs()
        dec = cwq.importance_decode_blocks(wi.copy(), pl, ps, case.off, case.seed,
                                           block_id_base=case.base)
        _assert_bits_equal(dec.cpu().numpy(), ws, f"{case.name}: decode")
    return gi, gs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nb", S.DYN_GROUPS_NB)
def test_dyn_groups(cwq, oracle, nb, mode):
    """4,096 groups: tiles handed out through the counter in the permuted order;
    4,095: the static assignment.  Group seeds wrap int32 inside the launch.
    Three runs must agree: which tile of a group publishes its threshold first
    must never show."""
    case = S.dyn_groups(nb)
    first = _check_blocks(cwq, oracle, case, mode, decode=(mode == 0))
    for _ in range(2):
        gi, gs = _encode(cwq, case, mode)
        assert np.array_equal(gi, first[0])
        _assert_bits_equal(gs, first[1], f"{case.name}: repeated run")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nb", S.TILES_SCAN_NB)
def test_tiles_scan(cwq, oracle, nb, mode):
    """k_imp_tiles' prefix over 16 rounds in registers (16,384 groups) and over
    17 and 18 streamed rounds, a tile above every carry."""
    _check_blocks(cwq, oracle, S.tiles_scan(nb), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [c[0] for c in S.CPT_LADDER])
def test_cpt_ladder(cwq, oracle, name, mode):
    """Tile sizes 1,024 to 16,384 chosen on the device, with groups of one row
    less than a tile up to three tiles less one row."""
    _check_blocks(cwq, oracle, S.cpt_ladder(name), mode, decode=(mode == 0))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,kind", S.CPT_LADDER_NEAR_TIES)
def test_cpt_ladder_near_ties(cwq, oracle, name, kind, mode):
    """Tiles of more rows than the survivor list holds, every score (nearly)
    equal: the list overflows and rows are scored exactly in line; with ties the
    lowest index must win in every tile and across tiles."""
    case = S.cpt_ladder(name, kind)
    gi, _ = _check_blocks(cwq, oracle, case, mode)
    if kind == "ties":
        assert not gi.any()


def _normals(cwq, latent, dev):
    ql, qs, pl, ps = (torch.from_numpy(a).to(dev) for a in latent)
    return cwq.Normal(ql, qs), cwq.Normal(pl, ps)


def _check_grouped(got, want, what):
    sample, indices, starts, (oi, oq) = got
    wsm, wi, wst, (woi, woq) = want
    assert np.array_equal(np.asarray(starts), np.asarray(wst)), what
    bad = np.nonzero(np.asarray(indices) != np.asarray(wi))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(wi)} indices differ, first groups {bad[:8]}"
    assert np.array_equal(oi, woi) and np.array_equal(oq, woq), what
    _assert_bits_equal(sample, wsm, f"{what}: samples")


_GROUPED_REF = {}


def _oracle_grouped(oracle, key, latent, seed, bits):
    if key not in _GROUPED_REF:
        _GROUPED_REF[key] = oracle.code_grouped_importance_sample(*latent, seed, bits)
    return _GROUPED_REF[key]


@pytest.mark.parametrize("mode", MODES)
def test_cpt_grouped(cwq, oracle, mode):
    """More than 2^24 candidates through the grouped call: the host knows the
    tile size (k_imp_eval's CPT_MAX instantiation); the step-by-step path runs
    the same groups with the tile chosen on the device."""
    import compression_without_quantization_amd.coded_importance_sampler as I
    dev = torch.device("cuda", 0)
    latent = S.cpt_grouped_latent()
    want = _oracle_grouped(oracle, "cpt", latent, S.CPT_GROUPED_SEED, S.CPT_GROUPED_BITS)
    t, p = _normals(cwq, latent, dev)
    old = I.USE_FUSED
    try:
        for fused in (True, False):
            I.USE_FUSED = fused
            got = I.code_grouped_importance_sample(None, t, p, S.CPT_GROUPED_SEED,
                                                   S.CPT_GROUPED_BITS, return_indices=True,
                                                   prune_mode=mode)
            _check_grouped(got, want, f"cpt_grouped, fused {fused}, prune_mode {mode}")
    finally:
        I.USE_FUSED = old


@pytest.mark.parametrize("mode", MODES)
def test_dyn_tiles_single(cwq, oracle, mode):
    """One item of at least 8,192 one-tile groups: the fused call knows the tile
    count and hands tiles out dynamically, permuted; the step-by-step path gets
    there by its group count."""
    import compression_without_quantization_amd.coded_importance_sampler as I
    dev = torch.device("cuda", 0)
    latent = S.dyn_tiles_latent(*S.DYN_TILES_SINGLE)
    want = _oracle_grouped(oracle, "single", latent, 17, S.DYN_TILES_BITS)
    t, p = _normals(cwq, latent, dev)
    old = I.USE_FUSED
    try:
        for fused in (True, False):
            I.USE_FUSED = fused
            got = I.code_grouped_importance_sample(None, t, p, 17, S.DYN_TILES_BITS,
                                                   return_indices=True, prune_mode=mode)
            _check_grouped(got, want, f"dyn_tiles, fused {fused}, prune_mode {mode}")
    finally:
        I.USE_FUSED = old


@pytest.mark.parametrize("mode", MODES)
def test_dyn_tiles_batch(cwq, oracle, mode):
    """A batch whose items stay below 8,192 tiles each and pass it together:
    per-group seeds (PER_BLOCK) with the dynamic hand-out; every item against
    the oracle's pipeline on that item alone."""
    import compression_without_quantization_amd.coded_importance_sampler as I
    dev = torch.device("cuda", 0)
    lat = [S.dyn_tiles_latent(*item) for item in S.DYN_TILES_BATCH]
    ts, ps = zip(*(_normals(cwq, l, dev) for l in lat))
    batch = I.code_grouped_importance_sample_batch(None, ts, ps, S.DYN_TILES_BATCH_SEEDS,
                                                   S.DYN_TILES_BITS, return_indices=True,
                                                   prune_mode=mode)
    assert len(batch) == len(lat)
    for i, (l, seed) in enumerate(zip(lat, S.DYN_TILES_BATCH_SEEDS)):
        want = _oracle_grouped(oracle, ("batch", i), l, seed, S.DYN_TILES_BITS)
        _check_grouped(batch[i], want, f"dyn_tiles batch item {i}, prune_mode {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", S.ROW_KINDS)
def test_row_lengths(cwq, oracle, kind, mode):
    """Rows of 0 to 1,025 dims (exact, short, pruned, exact by length) in one,
    two and three tiles; ties (index 0 must win in and across tiles), near-ties
    (survivor list overflow, rows scored in line), a convex log ratio, and a
    dim the value gate rejects (the exact loop on a screenable length)."""
    case = S.row_lengths(kind)
    gi, _ = _check_blocks(cwq, oracle, case, mode)
    if kind == "ties":
        assert not gi[case.sizes > 0].any()


@pytest.mark.parametrize("mode", MODES)
def test_counts_edge(cwq, oracle, mode):
    """Counts 0, -1 and -2^31 are coded as one candidate, like 1."""
    _check_blocks(cwq, oracle, S.counts_edge(), mode)


@pytest.mark.parametrize("d", S.HI_DECODE_D)
def test_hi_counters_decode(cwq, oracle, d):
    """Rows on both sides of the first Philox block index of 2^32 (and, for 255
    dims, the row that straddles it)."""
    rng = np.random.default_rng(d)
    rows = S.hi_decode_rows(d)
    nb = len(rows)
    pl = rng.standard_normal(nb * d).astype(np.float32)
    ps = rng.uniform(0.5, 2.0, nb * d).astype(np.float32)
    off = np.arange(nb + 1, dtype=np.int64) * d
    seed, base = 2 ** 31 - 2, 1
    got = cwq.importance_decode_blocks(rows, pl, ps, off, seed, block_id_base=base).cpu().numpy()
    for g, r in enumerate(rows):
        sg = int(np.int32(np.uint32((seed + base + g) & 0xFFFFFFFF)))
        want = oracle.importance_decode_block(r, pl[g * d:(g + 1) * d], ps[g * d:(g + 1) * d], sg)
        _assert_bits_equal(got[g * d:(g + 1) * d], want, f"d {d}, row {r}")


def test_hi_counters_encode(cwq, oracle):
    """One group of 256 dims and 2^26 + 2^24 candidates: N d > 2^34, so the
    screening loop runs with the full 64-bit Philox counter (HI0 off).

    A weaker reference than elsewhere in this file: the oracle cannot scan
    2.1e10 terms in seconds.  Instead (a) prune_mode 2 must equal prune_mode 0
    on the GPU (the exact loop's 64-bit counters are pinned by
    test_hi_counters_decode and test_gpu.py::test_philox_counter_crosses_2_32),
    (b) the winner's sample must be the oracle's row of that index, and (c) the
    winner's oracle score must be at least the oracle's score of every row of a
    4,096-row window around row 2^26 and of 4,096 seeded random rows, with the
    lower index on equal scores.  The seed is chosen so that the exact-mode
    winner lies past row 2^26, where a wrong high counter would show."""
    case = S.hi_encode()
    tl, ts, pl, ps = case.inputs()
    (i0,), s0 = _encode(cwq, case, 0)
    (i2,), s2 = _encode(cwq, case, 2)
    boundary = S.hi_first_row(S.HI_ENCODE_D)
    assert boundary == 1 << 26
    assert boundary < i0 < S.HI_ENCODE_N, i0
    assert i0 == S.HI_ENCODE_WINNER
    assert i2 == i0
    _assert_bits_equal(s2, s0, "hi_counters: screened vs exact sample")
    _assert_bits_equal(s2, oracle.importance_decode_block(i2, pl, ps, case.seed),
                       "hi_counters: winner's sample")
    rng = np.random.default_rng(26)
    rows = np.concatenate([np.arange(boundary - 2048, boundary + 2048),
                           rng.integers(0, S.HI_ENCODE_N, 4096), [i2]]).astype(np.int64)
    sc = oracle.importance_scores(tl, ts, pl, ps, case.seed, rows)
    win, others, orow = sc[-1], sc[:-1], rows[:-1]
    assert not np.isnan(sc).any()
    assert (others <= win).all(), (int(orow[np.argmax(others)]), float(others.max()), float(win))
    assert (orow[others == win] >= i2).all()
