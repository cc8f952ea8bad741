"""GPU: uniform blocks with a bit budget each (varbits.py on
cwq_greedy_encode_uniform_var, cwq_pack_indices_var, cwq_unpack_indices_var,
cwq_block_bits) against the CPU oracle block by block, against the plain
uniform encoder, and against binary_io's bit strings, bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

from compression_without_quantization_amd import _lib
from compression_without_quantization_amd.binary_io import _pack_bits, to_bit_string

pytestmark = pytest.mark.gpu

SEED = 2147483647 - 5  # seed + g wraps past 2^31 - 1 inside every shape below
# (nb, d, n_steps, max bits): the fast pruned kernel, multi-step; the general
# layout (d % 8 != 0, d % 4 == 0); odd d (the scalar gather)
SHAPES = [(200, 32, 2, 12), (96, 12, 3, 9), (64, 7, 1, 10)]
BIG = (20011, 8, 2)  # ten workgroups of the sort, the last one partial


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    return C


def _wrap32(x):
    return int(np.int32(np.uint32(int(x) & 0xFFFFFFFF)))


def _u32(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _inputs(nb, d, max_bits, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * nb + d))
    D = nb * d
    tl = rng.standard_normal(D).astype(np.float32)
    ts = rng.uniform(0.3, 0.9, D).astype(np.float32)
    pl = (0.25 * rng.standard_normal(D)).astype(np.float32)
    ps = rng.uniform(0.8, 1.3, D).astype(np.float32)
    bits = rng.integers(0, max_bits + 1, nb).astype(np.int32)
    bits[0] = bits[-1] = 0
    bits[nb // 2] = max_bits
    return tl, ts, pl, ps, bits


@functools.lru_cache(maxsize=None)
def _oracle_blocks(nb, d, n_steps, max_bits, rho):
    """The oracle's code_greedy_sample of every block with its own count."""
    from oracle import oracle as O
    tl, ts, pl, ps, bits = _inputs(nb, d, max_bits)
    idx = np.zeros((nb, n_steps), np.int32)
    sample = np.zeros(nb * d, np.float32)
    for g in range(nb):
        sl = slice(g * d, (g + 1) * d)
        i, s = O.code_greedy_sample(tl[sl], ts[sl], pl[sl], ps[sl], int(bits[g]), n_steps,
                                    _wrap32(SEED + g), rho)
        idx[g], sample[sl] = i, s
    return idx, sample


def _ref_stream_loop(idx, bits):
    """binary_io's own bytes: the joined to_bit_string fields through _pack_bits."""
    s = ''.join(to_bit_string(int(idx[g, k]), int(bits[g]))
                for g in range(idx.shape[0]) for k in range(idx.shape[1]))
    return _pack_bits(s), len(s)


def _ref_stream_numpy(idx, bits):
    """The same stream, vectorised: every field's bits LSB first, then packbits."""
    nb, n_steps = idx.shape
    w = np.repeat(bits.astype(np.int64), n_steps)
    v = idx.reshape(-1).astype(np.int64)
    total = int(w.sum())
    start = np.cumsum(w) - w
    field = np.repeat(np.arange(w.size), w)
    pos = np.arange(total) - start[field]
    stream = ((v[field] >> pos) & 1).astype(np.uint8)
    return np.packbits(stream).tobytes(), total


# ---------------------------------------------------------------------------
# 1. against the oracle, block by block
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("prune_mode", [0, None])
@pytest.mark.parametrize("rho", [1.0, 0.7])
@pytest.mark.parametrize("nb,d,n_steps,max_bits", SHAPES)
def test_encode_var_vs_oracle(cwq, oracle, nb, d, n_steps, max_bits, rho, prune_mode):
    tl, ts, pl, ps, bits = _inputs(nb, d, max_bits)
    assert bits[0] == 0 and bits[-1] == 0 and bits.max() == max_bits
    assert SEED + nb > 2147483647
    want_idx, want_sample = _oracle_blocks(nb, d, n_steps, max_bits, rho)
    idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, SEED, rho=rho,
                                        block_dim=d, prune_mode=prune_mode)
    assert idx.shape == (nb, n_steps) and idx.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(_u32(sample), _u32(want_sample))
    assert (want_idx[bits == 0] == 0).all()


# ---------------------------------------------------------------------------
# 2. against the plain call, over many workgroups of the sort
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big_inputs():
    nb, d, n_steps = BIG
    rng = np.random.Generator(np.random.PCG64(99))
    D = nb * d
    tl = rng.standard_normal(D).astype(np.float32)
    ts = rng.uniform(0.3, 0.9, D).astype(np.float32)
    pl = np.zeros(D, np.float32)
    ps = np.ones(D, np.float32)
    bits = rng.choice(np.array([0, 3, 5, 8], np.int32), nb)
    return tuple(torch.from_numpy(a).cuda() for a in (tl, ts, pl, ps)) + (bits,)


def test_encode_var_vs_plain_many_workgroups(cwq):
    nb, d, n_steps = BIG
    tl, ts, pl, ps, bits = _big_inputs()
    base = 12345
    idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, 42, block_dim=d,
                                        block_id_base=base)
    idx = idx.cpu().numpy()
    sample = _u32(sample).reshape(nb, d)
    for b in (0, 3, 5, 8):
        pi, psamp = cwq.encode_blocks(tl, ts, pl, ps, b, n_steps, 42, block_dim=d,
                                      block_id_base=base)
        rows = bits == b
        assert rows.sum() > 1000
        assert np.array_equal(idx[rows], pi.cpu().numpy()[rows]), b
        assert np.array_equal(sample[rows], _u32(psamp).reshape(nb, d)[rows]), b
    # every block at one count: one bucket, the identity permutation
    one = np.full(nb, 5, np.int32)
    idx1, sample1 = cwq.encode_blocks_var(tl, ts, pl, ps, one, n_steps, 42, block_dim=d,
                                          block_id_base=base)
    pi, psamp = cwq.encode_blocks(tl, ts, pl, ps, 5, n_steps, 42, block_dim=d,
                                  block_id_base=base)
    assert torch.equal(idx1, pi)
    assert np.array_equal(_u32(sample1), _u32(psamp))


def test_encode_var_one_block_and_none(cwq):
    d = 8
    tl, ts, pl, ps, _ = _big_inputs()
    idx, sample = cwq.encode_blocks_var(tl[:d], ts[:d], pl[:d], ps[:d], [6], 2, 42, block_dim=d)
    pi, psamp = cwq.encode_blocks(tl[:d], ts[:d], pl[:d], ps[:d], 6, 2, 42, block_dim=d)
    assert torch.equal(idx, pi) and np.array_equal(_u32(sample), _u32(psamp))
    e = torch.empty(0, dtype=torch.float32, device="cuda")
    idx, sample = cwq.encode_blocks_var(e, e, e, e, [], 2, 42, block_dim=d)
    assert idx.shape == (0, 2) and sample.numel() == 0
    code, total = cwq.pack_indices(idx, [])
    assert code.numel() == 0 and total == 0
    assert cwq.unpack_indices(b"", [], 2).shape == (0, 2)


# ---------------------------------------------------------------------------
# 3. the stream
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nb,d,n_steps,max_bits", SHAPES)
def test_pack_matches_binary_io(cwq, oracle, nb, d, n_steps, max_bits):
    bits = _inputs(nb, d, max_bits)[4]
    idx = _oracle_blocks(nb, d, n_steps, max_bits, 1.0)[0]
    want, total = _ref_stream_loop(idx, bits)
    assert _ref_stream_numpy(idx, bits) == (want, total)  # the vectorised reference agrees
    code, got_total = cwq.pack_indices(idx, bits)
    assert got_total == total and code.dtype == torch.uint8
    assert code.cpu().numpy().tobytes() == want
    back = cwq.unpack_indices(code, bits, n_steps)
    assert np.array_equal(back.cpu().numpy(), idx)
    assert np.array_equal(cwq.unpack_indices(want, bits, n_steps).cpu().numpy(), idx)
    # a code cut short by 3 bytes: the missing bits read as 0
    cut = want[:-3]
    keep = 8 * len(cut)
    w = np.repeat(bits.astype(np.int64), n_steps)
    start = np.cumsum(w) - w
    have = np.clip(keep - start, 0, w)  # bits of each field that survive
    want_cut = (idx.reshape(-1).astype(np.int64) & ((1 << have) - 1)).reshape(idx.shape)
    assert (want_cut != idx).any()
    got_cut = cwq.unpack_indices(np.frombuffer(cut, np.uint8), bits, n_steps)
    assert np.array_equal(got_cut.cpu().numpy(), want_cut)


def test_pack_many_workgroups_and_odd_totals(cwq):
    nb, d, n_steps = BIG
    rng = np.random.Generator(np.random.PCG64(5))
    bits = _big_inputs()[4].copy()
    bits[rng.integers(0, nb, 40)] = 30  # fields that span five bytes
    bits[rng.integers(0, nb, 40)] = 1
    bits[0] = 4
    idx = (rng.integers(0, 1 << 30, (nb, n_steps)) & ((1 << bits.astype(np.int64)) - 1)[:, None])
    idx = idx.astype(np.int32)
    want, total = _ref_stream_numpy(idx, bits)
    if total % 8 == 0:  # make the total no multiple of 8
        bits[0] += 1
        want, total = _ref_stream_numpy(idx, bits)
    assert total % 8 != 0
    code, got_total = cwq.pack_indices(idx, bits)
    assert got_total == total
    assert code.cpu().numpy().tobytes() == want
    assert np.array_equal(cwq.unpack_indices(code, bits, n_steps).cpu().numpy(), idx)
    # a total of 0: an empty stream; long runs of empty blocks between fields
    zero = np.zeros(nb, np.int32)
    code, got_total = cwq.pack_indices(np.zeros((nb, n_steps), np.int32), zero)
    assert code.numel() == 0 and got_total == 0
    assert not cwq.unpack_indices(code, zero, n_steps).any()
    sparse = zero.copy()
    sparse[[3, 9000, nb - 1]] = [7, 13, 2]
    sidx = np.zeros((nb, n_steps), np.int32)
    sidx[[3, 9000, nb - 1]] = [[100, 27], [8191, 4097], [3, 1]]
    want, total = _ref_stream_numpy(sidx, sparse)
    code, got_total = cwq.pack_indices(sidx, sparse)
    assert got_total == total == 44 and code.cpu().numpy().tobytes() == want
    assert np.array_equal(cwq.unpack_indices(code, sparse, n_steps).cpu().numpy(), sidx)


# ---------------------------------------------------------------------------
# 4. round trip
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [1.0, 0.7])
@pytest.mark.parametrize("nb,d,n_steps,max_bits", SHAPES)
def test_round_trip(cwq, oracle, nb, d, n_steps, max_bits, rho):
    tl, ts, pl, ps, bits = _inputs(nb, d, max_bits)
    idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, SEED, rho=rho,
                                        block_dim=d)
    code, _ = cwq.pack_indices(idx, bits)
    dec = cwq.decode_blocks_var(code, bits, pl, ps, n_steps, SEED, rho=rho, block_dim=d)
    assert np.array_equal(_u32(dec), _u32(sample))
    dec2 = cwq.decode_blocks_var(idx, bits, pl, ps, n_steps, SEED, rho=rho, block_dim=d)
    assert np.array_equal(_u32(dec2), _u32(sample))
    want_idx, _ = _oracle_blocks(nb, d, n_steps, max_bits, rho)
    want = np.concatenate([
        oracle.decode_greedy_sample(want_idx[g], pl[g * d:(g + 1) * d], ps[g * d:(g + 1) * d],
                                    int(bits[g]), n_steps, _wrap32(SEED + g), rho)
        for g in range(nb)])
    assert np.array_equal(_u32(dec), _u32(want))


def test_encode_decode_with_an_array_of_bits(cwq):
    nb, d, _, max_bits = SHAPES[0]
    tl, ts, pl, ps, bits = _inputs(nb, d, max_bits)
    sh = (nb, d)
    idx, sample = cwq.encode(pl.reshape(sh), ps.reshape(sh), tl.reshape(sh), ts.reshape(sh),
                             SEED, bits, block_id_base=3)
    assert idx.shape == (nb,) and sample.shape == sh and isinstance(sample, np.ndarray)
    vi, vs = cwq.encode_blocks_var(tl, ts, pl, ps, bits, 1, SEED, block_dim=d, block_id_base=3)
    assert np.array_equal(idx, vi.cpu().numpy().reshape(-1))
    assert np.array_equal(_u32(sample).reshape(-1), _u32(vs))
    dec = cwq.decode(idx, pl.reshape(sh), ps.reshape(sh), SEED, bits, block_id_base=3)
    assert np.array_equal(_u32(dec), _u32(sample))
    code, _ = cwq.pack_indices(vi, bits)
    dec = cwq.decode(code.cpu().numpy().tobytes(), pl.reshape(sh), ps.reshape(sh), SEED, bits,
                     block_id_base=3)
    assert np.array_equal(_u32(dec), _u32(sample))
    # one integer still takes the plain path
    pi, psamp = cwq.encode(pl.reshape(sh), ps.reshape(sh), tl.reshape(sh), ts.reshape(sh),
                           SEED, 6)
    qi, qs = cwq.encode_blocks(tl, ts, pl, ps, 6, 1, SEED, block_dim=d)
    assert np.array_equal(pi, qi.cpu().numpy().reshape(-1))
    assert np.array_equal(_u32(psamp).reshape(-1), _u32(qs))


# ---------------------------------------------------------------------------
# 5. block_bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nb,d", [(96, 32), (160, 7)])
def test_block_bits(cwq, oracle, nb, d):
    rng = np.random.Generator(np.random.PCG64(2024 + nb))
    width = rng.uniform(0.5, 1.0, (nb, 1))   # posterior width and shift vary by block
    shift = rng.uniform(0.0, 0.8 * math.sqrt(32.0 / d), (nb, 1))
    ql = (shift * rng.standard_normal((nb, d))).astype(np.float32)
    qs = (width * rng.uniform(0.8, 1.2, (nb, d))).astype(np.float32)
    pl = np.zeros((nb, d), np.float32)
    ps = np.ones((nb, d), np.float32)
    extra = 1.0 / math.log(2.0)
    kl = oracle.kl_normal_normal(ql, qs, pl, ps).reshape(nb, d)
    S = np.cumsum(kl.astype(np.float64), axis=1)[:, -1]
    x = S / np.log(2.0) + extra
    # precondition: no block sits on an integer boundary
    assert np.abs(x - np.round(x)).min() > 1e-6
    want = np.clip(np.ceil(x), 0, 30).astype(np.int32)
    assert want.min() >= 1 and len(set(want.tolist())) > 5
    got, klb = cwq.block_bits(ql, qs, pl, ps, d, return_kl_bits=True)
    assert got.dtype == torch.int32 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(klb.cpu().numpy(), (S / np.log(2.0)).astype(np.float32))
    # clamping at both ends
    lo, hi = int(np.percentile(want, 30)), int(np.percentile(want, 70))
    assert want.min() < lo < hi < want.max()
    got = cwq.block_bits(ql, qs, pl, ps, d, min_bits=lo, max_bits=hi)
    assert np.array_equal(got.cpu().numpy(), np.clip(want, lo, hi))
    # a NaN scale: the most the caller allows
    qs2 = qs.copy()
    qs2[5, d // 2] = np.nan
    got = cwq.block_bits(ql, qs2, pl, ps, d, max_bits=hi).cpu().numpy()
    assert got[5] == hi
    keep = np.arange(nb) != 5
    assert np.array_equal(got[keep], np.clip(want, 0, hi)[keep])
    with pytest.raises(ValueError):
        cwq.block_bits(ql, qs, pl, ps, nb * d - 1)


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [31, -1])
def test_out_of_range_count_refused_before_any_write(cwq, bad):
    nb, d, n_steps, max_bits = SHAPES[1]
    tl, ts, pl, ps, bits = _inputs(nb, d, max_bits)
    bits = bits.copy()
    bits[[10, 40]] = bad
    out_idx = torch.full((nb, n_steps), -77, dtype=torch.int32, device="cuda")
    out_sample = torch.full((nb * d,), -77.0, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.CwqError, match=r"\b2 of 96 n_bits values outside \[0, 30\]"):
        cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, 1, block_dim=d, out_idx=out_idx,
                              out_sample=out_sample)
    assert (out_idx == -77).all() and (out_sample == -77.0).all()
    with pytest.raises(_lib.CwqError, match="outside"):
        cwq.pack_indices(np.zeros((nb, n_steps), np.int32), bits)
    with pytest.raises(_lib.CwqError, match="outside"):
        cwq.unpack_indices(b"\0" * 16, bits, n_steps)


def test_short_workspace_and_wrong_length(cwq):
    from compression_without_quantization_amd.varbits import encode_var_workspace_bytes
    nb, d, n_steps, max_bits = SHAPES[1]
    tl, ts, pl, ps, bits = _inputs(nb, d, max_bits)
    need = encode_var_workspace_bytes(nb, d, n_steps)
    ws = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.CwqError, match=r"\(-3\).*workspace"):
        cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, 1, block_dim=d, workspace=ws)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx, _ = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, 1, block_dim=d, workspace=ws)
    # more steps than the sorted inputs can stage (n_steps > 4 d): the tail region
    d1 = 1
    many = encode_var_workspace_bytes(nb * d, d1, 5)
    assert many > encode_var_workspace_bytes(nb * d, d1, 4)
    b1 = np.resize(bits, nb * d).astype(np.int32)
    i5, s5 = cwq.encode_blocks_var(tl, ts, pl, ps, b1, 5, 1, block_dim=d1)
    for b in (0, max_bits):
        pi, psamp = cwq.encode_blocks(tl, ts, pl, ps, b, 5, 1, block_dim=d1)
        rows = b1 == b
        assert rows.any() and np.array_equal(i5.cpu().numpy()[rows], pi.cpu().numpy()[rows])
        assert np.array_equal(_u32(s5)[rows], _u32(psamp)[rows])
    for wrong in (bits[:-1], np.concatenate([bits, bits[:1]])):
        with pytest.raises(ValueError):
            cwq.encode_blocks_var(tl, ts, pl, ps, wrong, n_steps, 1, block_dim=d)
        with pytest.raises(ValueError):
            cwq.pack_indices(idx, wrong)
        with pytest.raises(ValueError):
            cwq.decode_blocks_var(idx, wrong, pl, ps, n_steps, 1, block_dim=d)
