"""GPU: ragged (CSR) blocks with a bit budget each (varbits.py on
cwq_greedy_encode_var and cwq_block_bits_csr) and the grouped coder with a
budget per group, against the CPU oracle block by block, against the plain CSR
encoder, and against binary_io's bit strings, bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

from compression_without_quantization_amd import _lib
from compression_without_quantization_amd.binary_io import (_pack_bits, bitcode_to_indices,
                                                            to_bit_string)
from compression_without_quantization_amd.synthetic import make_latents

pytestmark = pytest.mark.gpu

SEED = 2147483647 - 5  # seed + g wraps past 2^31 - 1 inside every shape below
LENGTHS = [0, 1, 3, 4, 5, 7, 8, 12, 31, 32, 33, 64, 65, 130]
COUNTS = [0, 1, 3, 5, 6, 8, 11, 12, 13]
NB = 97
BASE = 1000003  # block_id_base


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


def _values(rng, D):
    tl = rng.standard_normal(D).astype(np.float32)
    ts = rng.uniform(0.3, 0.9, D).astype(np.float32)
    pl = (0.25 * rng.standard_normal(D)).astype(np.float32)
    ps = rng.uniform(0.8, 1.3, D).astype(np.float32)
    return tl, ts, pl, ps


@functools.lru_cache(maxsize=None)
def _ragged():
    """97 blocks: every length class, a 0-dim block between non-empty ones, the
    first and the last block at 0 bits."""
    rng = np.random.Generator(np.random.PCG64(4242))
    lens = np.concatenate([np.array(LENGTHS), rng.choice(LENGTHS, NB - len(LENGTHS))])
    rng.shuffle(lens)
    lens[0], lens[-1] = 5, 33
    lens[10:13] = [7, 0, 12]
    bits = rng.choice(np.array(COUNTS, np.int32), NB)
    bits[0] = bits[-1] = 0
    # the long blocks meet the general pruned kernel (>= 4096 candidates)
    bits[np.flatnonzero(lens == 130)[0]] = 13
    bits[np.flatnonzero(lens == 65)[0]] = 12
    bits[np.flatnonzero(lens == 3)[0]] = 13
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return (off,) + _values(rng, int(off[-1])) + (bits,)


@functools.lru_cache(maxsize=None)
def _oracle_ragged(which, n_steps, rho, base):
    """The oracle's code_greedy_sample of every non-empty block with its own count."""
    from oracle import oracle as O
    off, tl, ts, pl, ps, bits = _ragged() if which == "ragged" else _long()
    nb = len(bits)
    idx = np.zeros((nb, n_steps), np.int32)
    sample = np.zeros(int(off[-1]), np.float32)
    for g in range(nb):
        if off[g + 1] == off[g]:
            continue
        sl = slice(int(off[g]), int(off[g + 1]))
        i, s = O.code_greedy_sample(tl[sl], ts[sl], pl[sl], ps[sl], int(bits[g]), n_steps,
                                    _wrap32(SEED + base + g), rho)
        idx[g], sample[sl] = i, s
    return idx, sample


# ---------------------------------------------------------------------------
# 1. against the oracle, block by block
# ---------------------------------------------------------------------------
def test_ragged_inputs_cover_the_paths():
    off, _, _, _, _, bits = _ragged()
    lens = np.diff(off)
    assert len(bits) == NB and off[0] == 0
    assert set(lens.tolist()) == set(LENGTHS)
    assert len(set(bits.tolist())) >= 6 and set(bits.tolist()) <= set(COUNTS)
    assert lens[11] == 0 and lens[10] > 0 and lens[12] > 0
    assert bits[0] == 0 and bits[-1] == 0 and lens[0] > 0 and lens[-1] > 0
    assert SEED + BASE + NB > 2147483647


@pytest.mark.parametrize("prune_mode", [0, None])
@pytest.mark.parametrize("rho", [1.0, 0.7])
@pytest.mark.parametrize("n_steps", [1, 3])
def test_encode_var_csr_vs_oracle(cwq, oracle, n_steps, rho, prune_mode):
    off, tl, ts, pl, ps, bits = _ragged()
    want_idx, want_sample = _oracle_ragged("ragged", n_steps, rho, BASE)
    idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, SEED, rho=rho,
                                        block_off=off, block_id_base=BASE,
                                        prune_mode=prune_mode)
    assert idx.shape == (NB, n_steps) and idx.dtype == torch.int32
    idx = idx.cpu().numpy()
    full = np.diff(off) > 0
    assert np.array_equal(idx[full], want_idx[full])
    assert np.array_equal(_u32(sample), _u32(want_sample))
    # 0-dim blocks: what the plain CSR call writes for them at that count
    for b in sorted(set(bits[~full].tolist())):
        pi, _ = cwq.encode_blocks(tl, ts, pl, ps, b, n_steps, SEED, rho=rho, block_off=off,
                                  block_id_base=BASE)
        rows = ~full & (bits == b)
        assert np.array_equal(idx[rows], pi.cpu().numpy()[rows]), b


# ---------------------------------------------------------------------------
# 2. a long block: visit-order records, the fork inside a bucket, and a bucket
# whose own longest block is far below the call's
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long():
    rng = np.random.Generator(np.random.PCG64(77))
    off = np.array([0, 5, 1105, 1105, 1145], np.int64)
    bits = np.array([8, 12, 3, 12], np.int32)
    return (off,) + _values(rng, int(off[-1])) + (bits,)


def test_encode_var_csr_long_block(cwq, oracle):
    off, tl, ts, pl, ps, bits = _long()
    assert np.diff(off).tolist() == [5, 1100, 0, 40]
    want_idx, want_sample = _oracle_ragged("long", 2, 1.0, 0)
    idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, 2, SEED, block_off=off)
    idx = idx.cpu().numpy()
    full = np.diff(off) > 0
    assert np.array_equal(idx[full], want_idx[full])
    assert np.array_equal(_u32(sample), _u32(want_sample))
    pi, _ = cwq.encode_blocks(tl, ts, pl, ps, 3, 2, SEED, block_off=off)
    assert np.array_equal(idx[2], pi.cpu().numpy()[2])


# ---------------------------------------------------------------------------
# 3. many workgroups of the sort, against the plain CSR call
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big():
    nb = 20011  # ten workgroups of the sort, the last one partial
    rng = np.random.Generator(np.random.PCG64(99))
    lens = rng.integers(0, 10, nb)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = int(off[-1])
    tl = rng.standard_normal(D).astype(np.float32)
    ts = rng.uniform(0.3, 0.9, D).astype(np.float32)
    bits = rng.choice(np.array([0, 3, 5, 8], np.int32), nb)
    t = tuple(torch.from_numpy(a).cuda() for a in (tl, ts, np.zeros(D, np.float32),
                                                   np.ones(D, np.float32)))
    return (off,) + t + (bits,)


def test_encode_var_csr_vs_plain_many_workgroups(cwq):
    off, tl, ts, pl, ps, bits = _big()
    nb, n_steps, base = len(bits), 2, 12345
    dim_block = np.repeat(np.arange(nb), np.diff(off))  # the block of every dim
    idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, 42, block_off=off,
                                        block_id_base=base)
    idx, sample = idx.cpu().numpy(), _u32(sample)
    plain5 = None
    for b in (0, 3, 5, 8):
        pi, psamp = cwq.encode_blocks(tl, ts, pl, ps, b, n_steps, 42, block_off=off,
                                      block_id_base=base)
        if b == 5:
            plain5 = (pi, psamp)
        rows = bits == b
        assert rows.sum() > 1000
        assert np.array_equal(idx[rows], pi.cpu().numpy()[rows]), b
        dims = rows[dim_block]
        assert np.array_equal(sample[dims], _u32(psamp)[dims]), b
    # every block at one count: one bucket, the identity permutation
    idx1, sample1 = cwq.encode_blocks_var(tl, ts, pl, ps, np.full(nb, 5, np.int32), n_steps, 42,
                                          block_off=off, block_id_base=base)
    assert torch.equal(idx1, plain5[0])
    assert np.array_equal(_u32(sample1), _u32(plain5[1]))


# ---------------------------------------------------------------------------
# 4. round trip
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [1, 3])
def test_round_trip_csr(cwq, n_steps):
    off, tl, ts, pl, ps, bits = _ragged()
    idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, SEED, rho=0.7,
                                        block_off=off, block_id_base=BASE)
    code, total = cwq.pack_indices(idx, bits)
    ih = idx.cpu().numpy()
    s = ''.join(to_bit_string(int(ih[g, k]), int(bits[g]))
                for g in range(NB) for k in range(n_steps))
    assert total == len(s) and code.cpu().numpy().tobytes() == _pack_bits(s)
    dec = cwq.decode_blocks_var(code, bits, pl, ps, n_steps, SEED, rho=0.7, block_off=off,
                                block_id_base=BASE)
    assert np.array_equal(_u32(dec), _u32(sample))
    dec2 = cwq.decode_blocks_var(idx, bits, pl, ps, n_steps, SEED, rho=0.7, block_off=off,
                                 block_id_base=BASE)
    assert np.array_equal(_u32(dec2), _u32(sample))


# ---------------------------------------------------------------------------
# 5. block_bits(block_off=...)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [1, 3])
def test_block_bits_csr(cwq, oracle, n_steps):
    rng = np.random.Generator(np.random.PCG64(2024 + n_steps))
    nb = 160
    lens = rng.choice(np.array([0, 1, 3, 7, 32, 63, 64, 65, 200]), nb)
    lens[:3] = [200, 0, 65]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = int(off[-1])
    blk = np.repeat(np.arange(nb), lens)
    shift = rng.uniform(0.0, 1.5, nb)[blk] / np.sqrt(np.maximum(lens[blk], 1) / 8.0)
    ql = (shift * rng.standard_normal(D)).astype(np.float32)
    qs = (rng.uniform(0.5, 1.0, nb)[blk] * rng.uniform(0.8, 1.2, D)).astype(np.float32)
    pl = np.zeros(D, np.float32)
    ps = np.ones(D, np.float32)
    extra = 1.0 / math.log(2.0)
    kl = oracle.kl_normal_normal(ql, qs, pl, ps)
    S = np.array([np.cumsum(kl[off[g]:off[g + 1]].astype(np.float64))[-1]
                  if lens[g] else 0.0 for g in range(nb)])
    x = (S / np.log(2.0) + extra) / float(n_steps)
    # precondition: no block sits on an integer boundary
    assert np.abs(x - np.round(x)).min() > 1e-6
    want = np.clip(np.ceil(x), 0, 30).astype(np.int32)
    assert len(set(want.tolist())) > 4
    got, klb = cwq.block_bits(ql, qs, pl, ps, block_off=off, n_steps=n_steps,
                              return_kl_bits=True)
    assert got.dtype == torch.int32 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(klb.cpu().numpy(), (S / np.log(2.0)).astype(np.float32))
    assert (klb.cpu().numpy()[lens == 0] == 0).all()
    # clamping at both ends
    lo, hi = int(np.percentile(want, 30)), int(np.percentile(want, 70))
    assert want.min() < lo < hi < want.max()
    got = cwq.block_bits(ql, qs, pl, ps, block_off=off, n_steps=n_steps, min_bits=lo,
                         max_bits=hi)
    assert np.array_equal(got.cpu().numpy(), np.clip(want, lo, hi))
    # a NaN scale: the most the caller allows
    qs2 = qs.copy()
    qs2[off[2] + 40] = np.nan
    got = cwq.block_bits(ql, qs2, pl, ps, block_off=off, n_steps=n_steps, max_bits=hi)
    got = got.cpu().numpy()
    assert got[2] == hi
    keep = np.arange(nb) != 2
    assert np.array_equal(got[keep], np.clip(want, 0, hi)[keep])


@pytest.mark.parametrize("nb,d", [(96, 32), (160, 7), (3, 200)])
def test_block_bits_csr_equal_lengths_is_block_bits(cwq, nb, d):
    rng = np.random.Generator(np.random.PCG64(5 + d))
    D = nb * d
    ql = (0.6 * rng.standard_normal(D)).astype(np.float32)
    qs = rng.uniform(0.4, 1.2, D).astype(np.float32)
    pl = (0.1 * rng.standard_normal(D)).astype(np.float32)
    ps = rng.uniform(0.8, 1.3, D).astype(np.float32)
    a, ka = cwq.block_bits(ql, qs, pl, ps, block_dim=d, return_kl_bits=True)
    b, kb = cwq.block_bits(ql, qs, pl, ps, block_off=np.arange(nb + 1) * d, n_steps=1,
                           return_kl_bits=True)
    assert torch.equal(a, b) and np.array_equal(_u32(ka), _u32(kb))


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [31, -1])
def test_out_of_range_count_refused_before_any_write_csr(cwq, bad):
    off, tl, ts, pl, ps, bits = _ragged()
    bits = bits.copy()
    bits[[10, 40]] = bad
    out_idx = torch.full((NB, 2), -77, dtype=torch.int32, device="cuda")
    out_sample = torch.full((int(off[-1]),), -77.0, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.CwqError, match=r"\b2 of 97 n_bits values outside \[0, 30\]"):
        cwq.encode_blocks_var(tl, ts, pl, ps, bits, 2, 1, block_off=off, out_idx=out_idx,
                              out_sample=out_sample)
    assert (out_idx == -77).all() and (out_sample == -77.0).all()


def test_short_workspace_wrong_length_and_block_arguments(cwq, cwqlib):
    off, tl, ts, pl, ps, bits = _ragged()
    D, n_steps = int(off[-1]), 2
    need = cwqlib.cwq_greedy_encode_var_workspace_size(NB, D, int(np.diff(off).max()), n_steps)
    ws = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.CwqError, match=r"\(-3\).*workspace"):
        cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, 1, block_off=off, workspace=ws)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, 1, block_off=off,
                                        workspace=ws)
    fresh, fsample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, 1, block_off=off)
    assert torch.equal(idx, fresh) and np.array_equal(_u32(sample), _u32(fsample))
    # what only the buckets' facts can tell, through the raw call: the real
    # arrays at full length (every read stays inside them) and one scalar or one
    # offset wrong; the workspace is the true shape's
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    arrays = [dev(a) for a in (tl, ts, pl, ps)]
    bits_d, longest = dev(bits), int(np.diff(off).max())
    lowered = off.copy()
    lowered[2] = off[1] - 1  # block 1 ends before it starts; block 2 is longer by as much
    assert 0 <= lowered[2] < lowered[1] and lowered.max() == D
    for offs, total, maxd, msg in [
            (off, D - 1, longest, b"the blocks hold %d dims, total_dims=%d" % (D, D - 1)),
            (off, D, longest - 1, b"a block holds %d dims, max_block_dim=%d" % (longest,
                                                                                longest - 1)),
            (lowered, D, longest, b"block_off decreases at 1 blocks")]:
        offs_d = dev(offs)
        out_idx = torch.full((NB, n_steps), -77, dtype=torch.int32, device="cuda")
        out_sample = torch.full((D,), -77.0, dtype=torch.float32, device="cuda")
        rc = cwqlib.cwq_greedy_encode_var(
            *[a.data_ptr() for a in arrays], offs_d.data_ptr(), NB, total, maxd,
            bits_d.data_ptr(), n_steps, 1, 1.0, 0, out_idx.data_ptr(), out_sample.data_ptr(),
            ws.data_ptr(), need, None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == -1 and cwqlib.cwq_last_error() == msg, cwqlib.cwq_last_error()
        assert (out_idx == -77).all() and (out_sample == -77.0).all()
    for kw in ({}, {"block_dim": 1, "block_off": off}):
        with pytest.raises(ValueError):
            cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, 1, **kw)
        with pytest.raises(ValueError):
            cwq.decode_blocks_var(idx, bits, pl, ps, n_steps, 1, **kw)
        with pytest.raises(ValueError):
            cwq.block_bits(tl, ts, pl, ps, **kw)
    for wrong in (bits[:-1], np.concatenate([bits, bits[:1]])):
        with pytest.raises(ValueError):
            cwq.encode_blocks_var(tl, ts, pl, ps, wrong, n_steps, 1, block_off=off)
        with pytest.raises(ValueError):
            cwq.decode_blocks_var(idx, wrong, pl, ps, n_steps, 1, block_off=off)
    # no blocks at all
    e = torch.empty(0, dtype=torch.float32, device="cuda")
    idx0, sample0 = cwq.encode_blocks_var(e, e, e, e, [], 2, 42, block_off=[0])
    assert idx0.shape == (0, 2) and sample0.numel() == 0
    assert cwq.block_bits(e, e, e, e, block_off=[0]).numel() == 0
    assert cwq.decode_blocks_var(idx0, [], e, e, 2, 42, block_off=[0]).numel() == 0


# ---------------------------------------------------------------------------
# 7. / 8. the grouped coder with a budget per group
# ---------------------------------------------------------------------------
MGS_BITS = 6  # groups close at a size a test can reach
GROUPED = [(2304, 1, 10), (2304, 3, 4), (16389, 1, 10), (16389, 3, 4)]


@functools.lru_cache(maxsize=None)
def _latents(D):
    ql, qs, pl, ps = make_latents(D, bits_per_dim=1.1, off_fraction=0.5, seed=31 + D)
    a = D // 3  # a stretch of inactive dims: several groups close at the size limit
    ql, qs = ql.copy(), qs.copy()
    ql[a:a + 300] = pl[a:a + 300]
    qs[a:a + 300] = ps[a:a + 300]
    return ql, qs, pl, ps


@functools.lru_cache(maxsize=None)
def _oracle_grouped(D, n_steps, n_bits, min_bits):
    """The composition on the oracle: the reference's partition, a budget per
    group from the same float32 per-dim KLs, the groups coded one by one."""
    from oracle import oracle as O
    from compression_without_quantization_amd import group_size_threshold
    ql, qs, pl, ps = _latents(D)
    tl, ts = O.standardise(ql, qs, pl, ps)
    kl = O.kl_normal_normal(ql, qs, pl, ps)
    thr = group_size_threshold(MGS_BITS)
    starts = O.group_starts(kl, n_bits * n_steps, thr)
    G = len(starts) - 1
    S = np.array([np.cumsum(kl[starts[g]:starts[g + 1]].astype(np.float64))[-1]
                  if starts[g + 1] > starts[g] else 0.0 for g in range(G)])
    x = (S / np.log(2.0) + 1.0 / math.log(2.0)) / float(n_steps)
    assert np.abs(x - np.round(x)).min() > 1e-6  # no group on an integer boundary
    bits = np.clip(np.ceil(x), min_bits, n_bits).astype(np.int32)
    samp = np.zeros(D, np.float32)
    idx = np.zeros((G, n_steps), np.int32)
    zeros, ones = np.zeros(D, np.float32), np.ones(D, np.float32)
    for g in range(G):
        sl = slice(starts[g], starts[g + 1])
        if sl.stop == sl.start:
            continue
        i, s = O.code_greedy_sample(tl[sl], ts[sl], zeros[sl], ones[sl], int(bits[g]), n_steps,
                                    _wrap32(SEED + g), 1.0)
        idx[g], samp[sl] = i, s
    return O.destandardise(samp, pl, ps), idx, starts, bits, thr


@pytest.mark.parametrize("D,n_steps,n_bits", GROUPED)
def test_grouped_var_vs_oracle(cwq, oracle, D, n_steps, n_bits):
    ql, qs, pl, ps = _latents(D)
    want, want_idx, starts, bits, thr = _oracle_grouped(D, n_steps, n_bits, 0)
    lens = np.diff(starts)
    # the inputs: three budgets or more, a group closed by size, one closed by KL
    assert len(set(bits.tolist())) >= 3
    assert (lens[:-2] == thr).any() and (lens[:-2] < thr).any() and lens.max() <= thr
    assert SEED + len(bits) > 2147483647
    sample, code, total, got_starts, got_bits = cwq.code_grouped_greedy_sample_var(
        cwq.Normal(ql, qs), cwq.Normal(pl, ps), n_steps, n_bits, SEED,
        max_group_size_bits=MGS_BITS)
    assert got_starts == starts
    assert got_bits.dtype == np.int32 and np.array_equal(got_bits, bits)
    assert (got_bits <= n_bits).all()
    assert isinstance(code, bytes) and total == int(bits.sum()) * n_steps
    assert len(code) == (total + 7) // 8
    full = lens > 0
    got_idx = cwq.unpack_indices(code, got_bits, n_steps).cpu().numpy()
    assert np.array_equal(got_idx[full], want_idx[full])
    assert np.array_equal(_u32(sample), _u32(want))
    dec = cwq.decode_grouped_greedy_sample_var(code, got_starts, got_bits, cwq.Normal(pl, ps),
                                               n_steps, SEED)
    assert np.array_equal(_u32(dec), _u32(sample))


@pytest.mark.parametrize("D,n_steps,n_bits", GROUPED)
def test_grouped_var_forced_to_the_cap(cwq, D, n_steps, n_bits):
    ql, qs, pl, ps = _latents(D)
    t, p = cwq.Normal(ql, qs), cwq.Normal(pl, ps)
    ref_sample, ref_code, ref_starts = cwq.code_grouped_greedy_sample(
        None, t, p, n_steps, n_bits, SEED, max_group_size_bits=MGS_BITS)
    sample, code, total, starts, bits = cwq.code_grouped_greedy_sample_var(
        t, p, n_steps, n_bits, SEED, max_group_size_bits=MGS_BITS, min_bits=n_bits)
    G = len(ref_starts) - 1
    assert starts == ref_starts and (bits == n_bits).all() and len(bits) == G
    assert total == G * n_steps * n_bits == len(ref_code)
    ref_idx = bitcode_to_indices(ref_code, n_bits, G * n_steps).reshape(G, n_steps)
    assert np.array_equal(cwq.unpack_indices(code, bits, n_steps).cpu().numpy(), ref_idx)
    assert np.array_equal(_u32(sample), _u32(ref_sample))
