"""CPU: tests/beam_reference.py, the NumPy restatement of the beam encoder, is
held to the oracle before the GPU tests trust it: at beam 1 it is the oracle's
greedy coder bit for bit, and above 1 the oracle's decoder rebuilds its sample
from its indices (so a beam path is decodable by today's decoders)."""
import numpy as np
import pytest

import beam_reference as R

LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257]
SEED = 2147483647 - 4  # seed + base + g wraps past 2^31 - 1 inside every call below
BASE = 2


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _values(rng, D):
    tl = rng.standard_normal(D).astype(np.float32)
    ts = rng.uniform(0.3, 0.9, D).astype(np.float32)
    pl = (0.25 * rng.standard_normal(D)).astype(np.float32)
    ps = rng.uniform(0.8, 1.3, D).astype(np.float32)
    return tl, ts, pl, ps


def _ragged():
    rng = np.random.Generator(np.random.PCG64(4242))
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    return (off,) + _values(rng, int(off[-1]))


def _adversarial():
    """The blocks of test_rows_wave_gpu.py::test_rows_wave_adversarial."""
    rng = np.random.Generator(np.random.PCG64(99))
    lens = [300, 257, 9, 300, 257, 64]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tl, ts, pl, ps = _values(rng, int(off[-1]))
    tl[off[0] + 250] = np.nan   # every candidate's value is NaN
    ps[off[1]:off[2]] = 0.0     # scale_s == 0: every candidate ties
    tl[off[2] + 8] = np.inf     # every candidate at -inf
    return off, tl, ts, pl, ps


def test_seed_wraps():
    assert SEED + BASE + len(LENGTHS) > 2147483647 and BASE != 0


def test_eigen_order_forms_agree(oracle):
    rng = np.random.Generator(np.random.PCG64(5))
    for d in (0, 1, 7, 8, 9, 17, 64, 257):
        x = (rng.standard_normal((6, d)) * 100).astype(np.float32)
        want = np.array([oracle.eigen_rowsum(r) for r in x], np.float32)
        assert np.array_equal(_u32(R.eigen_rowsums(x)), _u32(want)), d


@pytest.mark.parametrize("rho", [1.0, 0.7])
@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("n_bits", [0, 1, 5])
def test_beam_one_is_the_greedy_coder(oracle, n_bits, n_steps, rho):
    off, tl, ts, pl, ps = _ragged()
    want_idx, want_sample = oracle.greedy_encode(tl, ts, pl, ps, off, n_bits, n_steps,
                                                 R.wrap32(SEED), rho, BASE)
    idx, sample, _ = R.beam_encode(oracle, tl, ts, pl, ps, off, n_bits, n_steps, SEED, 1, rho, BASE)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(_u32(sample), _u32(want_sample))


def test_beam_one_adversarial(oracle):
    off, tl, ts, pl, ps = _adversarial()
    want_idx, want_sample = oracle.greedy_encode(tl, ts, pl, ps, off, 5, 2, 42, 1.0, 0)
    idx, sample, value = R.beam_encode(oracle, tl, ts, pl, ps, off, 5, 2, 42, 1)
    assert np.array_equal(idx, want_idx)
    assert (idx[:3] == 0).all() and (idx[3:] != 0).any()
    assert np.array_equal(_u32(sample), _u32(want_sample))
    assert value[0] == R.LOWEST and value[2] == R.LOWEST


@pytest.mark.parametrize("beam", [2, 3, 16])
def test_beam_paths_decode(oracle, beam):
    off, tl, ts, pl, ps = _ragged()
    n_bits, n_steps, rho = 5, 3, 0.7
    idx, sample, value = R.beam_encode(oracle, tl, ts, pl, ps, off, n_bits, n_steps, SEED, beam,
                                       rho, BASE)
    back = oracle.greedy_decode(idx, pl, ps, off, n_bits, n_steps, R.wrap32(SEED), rho, BASE)
    assert np.array_equal(_u32(back), _u32(sample))
    # a beam does search: some block leaves the greedy path
    greedy = oracle.greedy_encode(tl, ts, pl, ps, off, n_bits, n_steps, R.wrap32(SEED), rho, BASE)[0]
    assert not np.array_equal(idx, greedy)
    assert value[0] == 0.0 and not np.signbit(value[0])  # the empty block: the sum of no terms


def test_beam_adversarial_ties_take_the_lowest_candidate(oracle):
    off, tl, ts, pl, ps = _adversarial()
    idx, sample, _ = R.beam_encode(oracle, tl, ts, pl, ps, off, 5, 2, 42, 4)
    assert (idx[:3] == 0).all()  # all candidates tie: beam 0 is (k, r) = (0, 0) at every step
    back = oracle.greedy_decode(idx, pl, ps, off, 5, 2, 42, 1.0, 0)
    assert np.array_equal(_u32(back), _u32(sample))
