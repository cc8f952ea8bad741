"""GPU: the wave-per-row encoder kernel (k_encode_rows_wave) against the CPU
oracle block by block, through its test entry (every block forced onto it) and
through cwq_greedy_encode_var's bucket rule, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from encode_shapes import LONG_BITS, LONG_LENS, ROWS_WAVE_BITS
from encode_shapes import ROWS_WAVE_LENGTHS as LENGTHS

pytestmark = pytest.mark.gpu

SEED = 2147483647 - 5  # seed + base + g wraps past 2^31 - 1 inside every call below
BASE = 3               # block_id_base


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
    rng = np.random.Generator(np.random.PCG64(1717))
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    return (off,) + _values(rng, int(off[-1]))


def _rows_wave(cwqlib, tl, ts, pl, ps, off, n_bits, n_steps, seed, rho=1.0, base=0, ws=None):
    """cwq_selftest_encode_rows_wave on cuda:0 -> (idx [nb, n_steps], sample [D]) tensors."""
    dev = torch.device("cuda")
    f = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dev).contiguous()
    tl, ts, pl, ps = f(tl), f(ts), f(pl), f(ps)
    offs = torch.as_tensor(np.asarray(off, np.int64)).to(dev)
    nb, D = int(offs.numel()) - 1, int(tl.numel())
    longest = int(np.diff(np.asarray(off)).max()) if nb else 0
    need = int(cwqlib.cwq_greedy_encode_workspace_size(nb, D, longest))
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    idx = torch.full((nb, n_steps), -77, dtype=torch.int32, device=dev)
    sample = torch.full((D,), -77.0, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rc = cwqlib.cwq_selftest_encode_rows_wave(
        tl.data_ptr(), ts.data_ptr(), pl.data_ptr(), ps.data_ptr(), offs.data_ptr(), nb, D,
        longest, int(n_bits), int(n_steps), _wrap32(seed), float(rho), int(base),
        idx.data_ptr(), sample.data_ptr(), ws.data_ptr(), ws.numel(), st)
    assert rc == 0, cwqlib.cwq_last_error()
    # the inputs stay referenced until the caller has synchronised
    return idx, sample, (tl, ts, pl, ps, offs, ws)


# ---------------------------------------------------------------------------
# (a) every block on the new kernel, against the oracle
# ---------------------------------------------------------------------------
def test_inputs_cover_the_paths():
    off = _ragged()[0]
    lens = np.diff(off)
    assert set(lens.tolist()) == {0, 1, 3, 4, 5, 7, 8, 9, 247, 248, 249, 255, 256, 257, 496, 1023,
                                  1025, 4095}
    assert lens[2] == 0 and lens[1] > 0 and lens[3] > 0
    assert SEED + BASE + len(lens) > 2147483647 and BASE != 0


# 1 .. 2,048 candidates: one row a block, fewer rows than the grid's waves
# (18 .. 576), more rows than the grid holds (36,864 > 4 * 2,048 waves)
@pytest.mark.parametrize("rho", [1.0, 0.7])
@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("n_bits", ROWS_WAVE_BITS)
def test_rows_wave_vs_oracle(cwqlib, oracle, n_bits, n_steps, rho):
    off, tl, ts, pl, ps = _ragged()
    want_idx, want_sample = oracle.greedy_encode(tl, ts, pl, ps, off, n_bits, n_steps,
                                                 _wrap32(SEED), rho, BASE)
    idx, sample, _keep = _rows_wave(cwqlib, tl, ts, pl, ps, off, n_bits, n_steps, SEED, rho, BASE)
    idx = idx.cpu().numpy()
    full = np.diff(off) > 0
    bad = np.flatnonzero((idx[full] != want_idx[full]).any(axis=1))
    assert bad.size == 0, (np.diff(off)[full][bad], idx[full][bad], want_idx[full][bad])
    assert (idx[~full] == 0).all()  # an empty block: index 0, as the other kernels write
    assert np.array_equal(_u32(sample), _u32(want_sample))


# ---------------------------------------------------------------------------
# (b) adversarial rows
# ---------------------------------------------------------------------------
def test_rows_wave_adversarial(cwqlib, oracle):
    rng = np.random.Generator(np.random.PCG64(99))
    lens = [300, 257, 9, 300, 257, 64]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tl, ts, pl, ps = _values(rng, int(off[-1]))
    tl[off[0] + 250] = np.nan   # every candidate's value is NaN: index 0
    ps[off[1]:off[2]] = 0.0     # scale_s == 0: every candidate ties, the lowest index wins
    tl[off[2] + 8] = np.inf     # every candidate at -inf: index 0
    n_bits, n_steps = 5, 2
    want_idx, want_sample = oracle.greedy_encode(tl, ts, pl, ps, off, n_bits, n_steps, 42, 1.0, 0)
    idx, sample, _keep = _rows_wave(cwqlib, tl, ts, pl, ps, off, n_bits, n_steps, 42)
    idx = idx.cpu().numpy()
    assert np.array_equal(idx, want_idx)
    assert (idx[:3] == 0).all() and (idx[3:] != 0).any()
    assert np.array_equal(_u32(sample), _u32(want_sample))


# ---------------------------------------------------------------------------
# (c) cwq_greedy_encode_var sends buckets of long blocks there
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long(n_short):
    rng = np.random.Generator(np.random.PCG64(31))
    lens = LONG_LENS + [3] * n_short
    bits = np.array(LONG_BITS + [9] * n_short, np.int32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return (off,) + _values(rng, int(off[-1])) + (bits,)


@functools.lru_cache(maxsize=None)
def _oracle_long(n_short, n_steps):
    from oracle import oracle as O
    off, tl, ts, pl, ps, bits = _long(n_short)
    idx = np.zeros((len(bits), n_steps), np.int32)
    sample = np.zeros(int(off[-1]), np.float32)
    for g in range(len(bits)):
        sl = slice(int(off[g]), int(off[g + 1]))
        i, s = O.code_greedy_sample(tl[sl], ts[sl], pl[sl], ps[sl], int(bits[g]), n_steps,
                                    _wrap32(SEED + g), 1.0)
        idx[g], sample[sl] = i, s
    return idx, sample


@pytest.mark.parametrize("n_short", [0, 40])
def test_encode_var_long_buckets(cwq, oracle, n_short):
    """n_short == 0: every bucket's mean block reaches 256 dims below 4,096
    candidates, so the default mode codes all of them with a wave per row and
    prune_mode=0 with k_encode_eval.  With 40 blocks of 3 dims at 9 bits that
    bucket's mean falls under 256 and it stays on the small-candidate path."""
    off, tl, ts, pl, ps, bits = _long(n_short)
    n_steps = 3
    lens = np.diff(off)
    for b in set(bits.tolist()):
        rule = lens[bits == b].sum() >= 256 * (bits == b).sum() and (1 << b) < 4096
        assert rule == (not (n_short and b == 9)), b
    want_idx, want_sample = _oracle_long(n_short, n_steps)
    got = {}
    for mode in (None, 0):
        idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, SEED, block_off=off,
                                            prune_mode=mode)
        got[mode] = (idx.cpu().numpy(), _u32(sample))
    assert np.array_equal(got[None][0], got[0][0]) and np.array_equal(got[None][1], got[0][1])
    assert np.array_equal(got[None][0], want_idx)
    assert np.array_equal(got[None][1], _u32(want_sample))


# ---------------------------------------------------------------------------
# (d) stream hygiene: nothing of a call is left in keys or LDS for the next
# ---------------------------------------------------------------------------
def test_back_to_back_calls_on_a_side_stream(cwqlib):
    off, tl, ts, pl, ps = _ragged()
    n_bits, n_steps = 5, 3
    seeds = (SEED, 99)
    single = []
    for s in seeds:
        i, x, _keep = _rows_wave(cwqlib, tl, ts, pl, ps, off, n_bits, n_steps, s, 1.0, BASE)
        single.append((i.cpu().numpy(), _u32(x)))
    assert not np.array_equal(single[0][0], single[1][0])
    nb, D = len(off) - 1, int(off[-1])
    ws = torch.empty(int(cwqlib.cwq_greedy_encode_workspace_size(nb, D, 4095)), dtype=torch.uint8,
                     device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the uploads and the output fills run on it too
        assert torch.cuda.current_stream() == side
        runs = [_rows_wave(cwqlib, tl, ts, pl, ps, off, n_bits, n_steps, s, 1.0, BASE, ws=ws)
                for s in seeds]
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for (i, x, _keep), (wi, wx) in zip(runs, single):
        assert np.array_equal(i.cpu().numpy(), wi)
        assert np.array_equal(_u32(x), wx)
