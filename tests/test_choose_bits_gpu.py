"""GPU: budgets from a rate table (cwq_choose_bits, choose_bits_total,
encode_blocks_rate).  choose_bits is held to its NumPy restatement
(tests/rate_reference.py) bit for bit: float64, a multiply then a subtract, the
lowest b among equal maxima."""
import functools

import numpy as np
import pytest
import torch

import rate_reference as RR

pytestmark = pytest.mark.gpu

LOWEST = np.float32(-3.4028234663852886e38)
NB, D, B, SEED = 300, 32, 12, 7


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    return C


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.Generator(np.random.PCG64(300))
    tl, ts, pl, ps = RR.inputs(rng, NB * D)
    # mixed KL: every fourth block far from the prior, every fourth on it
    tl = tl.reshape(NB, D)
    tl[0::4] *= np.float32(2.5)
    tl[1::4] *= np.float32(0.1)
    return tl.reshape(-1), ts, pl, ps


@pytest.fixture(scope="module")
def real(cwq):
    """(idx, value) of the inputs' table, host copies; computed once."""
    idx, value = cwq.rate_table(*_inputs(), B, SEED, block_dim=D)
    idx, value = idx.cpu().numpy(), value.cpu().numpy()
    idx.setflags(write=False)
    value.setflags(write=False)
    return idx, value


def _crafted():
    v = np.zeros((8, 6), np.float32)
    v[0] = 1.5                                   # flat: the lowest b wins
    v[1] = LOWEST                                # a row at the clamp
    v[2] = [0, 1, 2, 3, 4, 5]                    # lam = 1: every b ties
    v[3] = [0, 0.5, 3, 3.5, 6, 6.25]             # lam = 1.5: b = 2 and b = 4 tie at 0
    v[4] = [-40, -30, -20, -12, -11.5, -11.25]   # concave
    v[5] = [-1e30, -1e30, -1e30, 0, 0, 0]
    v[6] = [0, 2 ** -24, 2 ** -23, 2 ** -22, 2 ** -21, 2 ** -20]
    v[7] = [-7, -7, -7, -7, -7, -6.5]
    return v


@pytest.mark.parametrize("lam", [0.0, 0.25, 0.5, 1.0, 1.5, 2.0 ** -25, 3.0, 1e30])
@pytest.mark.parametrize("lo,hi", [(0, None), (2, 4), (0, 3), (5, 5), (1, 30)])
def test_choose_bits_on_crafted_tables(cwq, lam, lo, hi):
    v = _crafted()
    got = cwq.choose_bits(v, lam, min_bits=lo, max_bits=hi).cpu().numpy()
    want = RR.choose_bits(v, lam, lo, hi)
    assert got.dtype == np.int32 and np.array_equal(got, want), (got, want)
    top = 5 if hi is None else min(hi, 5)
    assert got[0] == lo and got[1] == lo and (got >= lo).all() and (got <= top).all()


def test_choose_bits_ties_take_the_lower_budget(cwq):
    v = _crafted()
    assert cwq.choose_bits(v, 1.0).cpu().numpy()[2] == 0
    assert cwq.choose_bits(v, 1.5).cpu().numpy()[3] == 0      # 0, 2 and 4 tie at 0
    assert cwq.choose_bits(v, 1.5, min_bits=1).cpu().numpy()[3] == 2
    assert cwq.choose_bits(v, 0.0).cpu().numpy().tolist() == [0, 0, 5, 5, 5, 3, 5, 5]


@pytest.mark.parametrize("lam", [0.0, 0.1, 0.6931471805599453, 1.0, 2.5])
def test_choose_bits_on_a_real_table(cwq, real, lam):
    _, value = real
    got = cwq.choose_bits(value, lam).cpu().numpy()
    assert np.array_equal(got, RR.choose_bits(value, lam))
    got = cwq.choose_bits(value, lam, min_bits=3, max_bits=9).cpu().numpy()
    assert np.array_equal(got, RR.choose_bits(value, lam, 3, 9))


def test_choose_bits_total(cwq, real):
    _, value = real
    free = RR.choose_bits(value, 0.0)
    assert 2 * NB < int(free.sum()) <= NB * B
    for target in (NB * 2, NB * 5 + 17, int(free.sum()) - 1):
        bits, lam = cwq.choose_bits_total(value, target)
        bits = bits.cpu().numpy()
        assert int(bits.sum()) <= target and lam > 0.0
        assert np.array_equal(bits, RR.choose_bits(value, lam))
        assert np.array_equal(bits, cwq.choose_bits(value, lam).cpu().numpy())
    # a target that lam = 0 meets returns lam = 0's choice
    bits, lam = cwq.choose_bits_total(value, NB * B)
    assert lam == 0.0 and np.array_equal(bits.cpu().numpy(), free)
    # clamps
    bits, lam = cwq.choose_bits_total(value, NB * 6, min_bits=4, max_bits=9)
    bits = bits.cpu().numpy()
    assert bits.min() >= 4 and bits.max() <= 9 and int(bits.sum()) <= NB * 6
    assert np.array_equal(bits, RR.choose_bits(value, lam, 4, 9))
    with pytest.raises(ValueError, match="exceed total_bits"):
        cwq.choose_bits_total(value, NB * 4 - 1, min_bits=4)
    bits, lam = cwq.choose_bits_total(value, NB * 4, min_bits=4)
    assert (bits.cpu().numpy() == 4).all()


@pytest.mark.parametrize("how", [dict(lam=0.6931471805599453), dict(total_bits=NB * 6)])
def test_encode_blocks_rate_is_encode_blocks_var_at_the_chosen_budgets(cwq, real, how):
    tidx, tval = real
    ins = _inputs()
    idx, sample, n_bits = cwq.encode_blocks_rate(*ins, SEED, B, block_dim=D, **how)
    bits = n_bits.cpu().numpy()
    assert idx.shape == (NB, 1) and idx.dtype == torch.int32 and n_bits.dtype == torch.int32
    assert len(set(bits.tolist())) > 3, "the blocks' budgets should differ"
    if "total_bits" in how:
        assert int(bits.sum()) <= how["total_bits"]
    else:
        assert np.array_equal(bits, RR.choose_bits(tval, how["lam"]))
    assert np.array_equal(idx.cpu().numpy()[:, 0], tidx[np.arange(NB), bits])
    code, total = cwq.pack_indices(idx, n_bits)
    assert total == int(bits.sum())
    dec = cwq.decode_blocks_var(code, n_bits, ins[2], ins[3], 1, SEED, block_dim=D)
    assert np.array_equal(dec.cpu().numpy().view(np.uint32), sample.cpu().numpy().view(np.uint32))
    vidx, vsample = cwq.encode_blocks_var(*ins, n_bits, 1, SEED, block_dim=D)
    assert np.array_equal(vidx.cpu().numpy(), idx.cpu().numpy())
    assert np.array_equal(vsample.cpu().numpy().view(np.uint32),
                          sample.cpu().numpy().view(np.uint32))


def test_encode_blocks_rate_ragged(cwq):
    off = np.array([0, 0, 1, 6, 70, 70, 335], np.int64)
    rng = np.random.Generator(np.random.PCG64(5))
    ins = RR.inputs(rng, int(off[-1]))
    idx, sample, n_bits = cwq.encode_blocks_rate(*ins, 11, 10, lam=0.5, block_off=off)
    vidx, vsample = cwq.encode_blocks_var(*ins, n_bits, 1, 11, block_off=off)
    assert np.array_equal(vidx.cpu().numpy(), idx.cpu().numpy())
    assert np.array_equal(vsample.cpu().numpy().view(np.uint32),
                          sample.cpu().numpy().view(np.uint32))
    assert n_bits.cpu().numpy()[[0, 4]].tolist() == [0, 0], "an empty block wins nothing"
