"""GPU: the batched grouped decoders (cwq_decode_grouped_greedy_batch on
k_decode_csr_q4, cwq_decode_grouped_importance_batch on k_imp_rows) against the
CPU oracle and against the single-item decoders, bit for bit."""
import numpy as np
import pytest
import torch

from compression_without_quantization_amd.synthetic import make_latents

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    C.coded_importance_sampler.VERBOSE = False
    return C


def _bits(a):
    """float32 bit patterns with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7fc00000
    return u


def _assert_bits_equal(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {w.size} differ, first at {bad[:8]}"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------
# 1. edge groups against the CPU oracle
# ---------------------------------------------------------------------------
EDGE_DIMS = [
    [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 0, 0, 255, 256, 257, 1, 1, 1],
    [4095, 1, 1025],
    [3] * 70 + [0] * 70 + [6],   # > 64 groups, and > 64 empty ones, in one wave's quads
]
EDGE_SEEDS = [42, 2147483647, -5]  # the second wraps at + g


@pytest.mark.parametrize("n_steps,bits,rho", [(1, 8, 1.0), (3, 5, 0.7), (2, 30, 1.0),
                                              (30, 14, 1.0)])
def test_batch_decode_edge_groups_vs_oracle(cwq, oracle, n_steps, bits, rho):
    rng = np.random.Generator(np.random.PCG64(1000 * n_steps + bits))
    top = (1 << bits) - 1
    items = []
    for k, dims in enumerate(EDGE_DIMS):
        offs = np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)
        G, D = len(dims), int(offs[-1])
        idx = rng.integers(0, top + 1, size=(G, n_steps), dtype=np.int64)
        idx[0, 0], idx[min(1, G - 1), -1] = 0, top    # the ends of the index range
        if k == 1:
            idx[0, -1] = top   # 4095 dims at 2^30 - 1: the Philox block counter passes 2^32
        p_loc = rng.standard_normal(D).astype(np.float32)      # about half negative
        p_scale = rng.uniform(0.25, 3.0, D).astype(np.float32)
        items.append((offs, idx.astype(np.int32), p_loc, p_scale))
    assert (items[1][1][0, -1].astype(np.int64) * 4095) >> 2 >= (1 << 32) or bits < 30
    # a condition on the inputs: rows start at every word of a Philox block
    seen = set()
    for offs, idx, _, _ in items:
        d = np.diff(offs)
        for g in np.nonzero(d % 4 != 0)[0]:
            seen.update(((idx[g].astype(np.int64) * int(d[g])) % 4).tolist())
    assert seen == {0, 1, 2, 3}
    want = []
    for (offs, idx, p_loc, p_scale), seed in zip(items, EDGE_SEEDS):
        z, o = np.zeros_like(p_loc), np.ones_like(p_loc)
        std = oracle.greedy_decode(idx, z, o, offs, bits, n_steps, seed, rho)
        want.append(oracle.destandardise(std, p_loc, p_scale))
    got = cwq.decode_grouped_greedy_sample_batch(
        None, [cwq.indices_to_bitcode(idx, bits) for _, idx, _, _ in items],
        [offs[:-1].copy() for offs, _, _, _ in items],
        [cwq.Normal(_dev(pl), _dev(ps)) for _, _, pl, ps in items],
        bits, n_steps, EDGE_SEEDS, rho=rho)
    assert len(got) == 3
    for k in range(3):
        _assert_bits_equal(got[k], want[k], f"item {k}")


# ---------------------------------------------------------------------------
# 2. batch == single == the encoder's samples
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def latents():
    out = []
    for k, D in enumerate([1, 3, 37, 4096, 20000]):
        q_loc, q_scale, p_loc, p_scale = make_latents(D, bits_per_dim=1.1, seed=100 + k)
        out.append((_dev(q_loc), _dev(q_scale), _dev(p_loc), _dev(p_scale)))
    return out


@pytest.mark.parametrize("n_steps,bits", [(1, 8), (2, 6)])
def test_batch_decode_equals_single_and_roundtrip(cwq, latents, n_steps, bits):
    targets = [cwq.Normal(a, b) for a, b, _, _ in latents]
    props = [cwq.Normal(c, d) for _, _, c, d in latents]
    seeds = [7, 8, 2147483647, -3, 42]
    enc = cwq.code_grouped_greedy_sample_batch(None, targets, props, n_steps, bits, seeds,
                                               max_group_size_bits=4)
    codes = [e[1] for e in enc]
    # item 0's starts as a list, the others as the batch encoder's arrays
    starts = [enc[0][2].tolist()] + [e[2] for e in enc[1:]]
    keep = [list(starts[0])] + [s.copy() for s in starts[1:]]
    dec = cwq.decode_grouped_greedy_sample_batch(None, codes, starts, props, bits, n_steps, seeds)
    assert starts[0] == keep[0] and all(np.array_equal(a, b) for a, b in zip(starts[1:], keep[1:]))
    assert all(isinstance(d, np.ndarray) and d.dtype == np.float32 for d in dec)
    for i in range(len(enc)):
        _assert_bits_equal(dec[i], enc[i][0], f"item {i} vs the encoder's sample")
        one = cwq.decode_grouped_greedy_sample(None, codes[i], starts[i], props[i], bits, n_steps,
                                               seeds[i])
        _assert_bits_equal(dec[i], one, f"item {i} vs the single call")
    ten = cwq.decode_grouped_greedy_sample_batch(None, codes, starts, props, bits, n_steps, seeds,
                                                 as_tensor=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in ten)
    for i in range(len(enc)):
        _assert_bits_equal(ten[i].cpu().numpy(), dec[i], f"item {i} as_tensor")
    # one seed for every item
    same = cwq.decode_grouped_greedy_sample_batch(None, codes[:1], starts[:1], props[:1], bits,
                                                  n_steps, 7)
    _assert_bits_equal(same[0], dec[0], "int seed")


# ---------------------------------------------------------------------------
# 3. short and bad codes
# ---------------------------------------------------------------------------
def test_batch_decode_short_and_bad_codes(cwq, latents):
    bits, n_steps = 8, 2
    props = [cwq.Normal(c, d) for _, _, c, d in latents[2:4]]
    targets = [cwq.Normal(a, b) for a, b, _, _ in latents[2:4]]
    enc = cwq.code_grouped_greedy_sample_batch(None, targets, props, n_steps, bits, [5, 6],
                                               max_group_size_bits=4)
    codes, starts = [e[1] for e in enc], [e[2] for e in enc]
    # cut 3 chars mid-group: the missing chars read as '0', as in the single call
    cut = [codes[0], codes[1][:-3]]
    dec = cwq.decode_grouped_greedy_sample_batch(None, cut, starts, props, bits, n_steps, [5, 6])
    one = cwq.decode_grouped_greedy_sample(None, cut[1], starts[1], props[1], bits, n_steps, 6)
    _assert_bits_equal(dec[1], one, "short code")
    _assert_bits_equal(dec[0], enc[0][0], "whole code beside it")
    # one group short: the decoded groups no longer cover the item
    short = [codes[0], codes[1][:-bits * n_steps]]
    with pytest.raises(ValueError, match=r"item 1: decoded groups cover \d+ of 4096 dims"):
        cwq.decode_grouped_greedy_sample_batch(None, short, starts, props, bits, n_steps, [5, 6])
    with pytest.raises(ValueError, match=r"decoded groups cover \d+ of 4096 dims"):
        cwq.decode_grouped_greedy_sample(None, short[1], starts[1], props[1], bits, n_steps, 6)
    bad = cwq.Normal(np.zeros(37, np.float64), np.ones(37, np.float64))
    with pytest.raises(Exception, match="Proposal datatype must be float32!"):
        cwq.decode_grouped_greedy_sample_batch(None, codes, starts, [bad, props[1]], bits,
                                               n_steps, [5, 6])
    assert cwq.decode_grouped_greedy_sample_batch(None, [], [], [], bits, n_steps, 5) == []


# ---------------------------------------------------------------------------
# 4. importance decoder
# ---------------------------------------------------------------------------
def test_importance_batch_decode_equals_single(cwq):
    n_bits_per_group = 12
    arrs = []
    for k, D in enumerate([600, 5, 1, 257]):
        q_loc, q_scale, p_loc, p_scale = make_latents(D, bits_per_dim=0.6, seed=200 + k)
        arrs.append([q_loc, q_scale, p_loc, p_scale])
    arrs[0][0][[3, 77, 512]] += np.float32(40.0) * arrs[0][3][[3, 77, 512]]  # outlier dims
    targets = [cwq.Normal(_dev(a[0]), _dev(a[1])) for a in arrs]
    props = [cwq.Normal(_dev(a[2]), _dev(a[3])) for a in arrs]
    seeds = [11, 2147483647, -9, 3]
    enc = cwq.code_grouped_importance_sample_batch(None, targets, props, seeds, n_bits_per_group,
                                                   max_group_size_bits=8)
    enc_i = cwq.code_grouped_importance_sample_batch(None, targets, props, seeds,
                                                     n_bits_per_group, max_group_size_bits=8,
                                                     return_indices=True)
    assert enc[0][3][0].size >= 3, "item 0 must have outliers"
    # the partition always cuts at D - 1, so the 1-dim item is an empty group and
    # one coded group; a lone group is decoded from hand-made starts below
    assert list(enc[2][2]) == [0, 0, 1]
    starts = [np.asarray(e[2])[:-1] for e in enc]
    oi, ov = [e[3][0] for e in enc], [e[3][1] for e in enc]
    for codes, use in (([e[1] for e in enc], False), ([e[1] for e in enc_i], True)):
        dec = cwq.decode_grouped_importance_sample_batch(None, codes, starts, props,
                                                         n_bits_per_group, seeds, oi, ov,
                                                         use_indices=use)
        assert len(dec) == 4
        for i in range(4):
            one = cwq.decode_grouped_importance_sample(None, codes[i], starts[i], props[i],
                                                       n_bits_per_group, seeds[i], oi[i], ov[i],
                                                       use_indices=use)
            _assert_bits_equal(dec[i], one, f"item {i} use_indices={use}")
    # items of a single group (no encoder yields one), any index legal
    rng = np.random.Generator(np.random.PCG64(5))
    lone = [cwq.Normal(_dev(rng.standard_normal(d).astype(np.float32)),
                       _dev(rng.uniform(0.5, 2.0, d).astype(np.float32))) for d in (9, 1, 300)]
    idx1 = [[1], [4096], [77]]
    none = np.zeros(0, np.int64), np.zeros(0, np.uint16)
    dec = cwq.decode_grouped_importance_sample_batch(None, idx1, [[0]] * 3, lone, 12, [1, -2, 3],
                                                     [none[0]] * 3, [none[1]] * 3,
                                                     use_indices=True)
    for i in range(3):
        one = cwq.decode_grouped_importance_sample(None, idx1[i], [0], lone[i], 12, [1, -2, 3][i],
                                                   none[0], none[1], use_indices=True)
        _assert_bits_equal(dec[i], one, f"lone group {i}")
