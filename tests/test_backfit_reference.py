"""CPU: tests/backfit_reference.py, the NumPy restatement of backfitting, is
held to the oracle before the GPU tests trust it: with no sweep it returns the
oracle's greedy code, its dec() is the oracle's decoder, and sweeps never lower
a block's value while changing some."""
import numpy as np
import pytest

import backfit_reference as B
import beam_reference as R

# ragged: the 8-wide vector / tail boundary, an empty block, a block past 64 dims
LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 13, 32, 32, 63, 64, 65, 130]
SEED = 2147483647 - 4  # seed + base + g wraps past 2^31 - 1 inside every call below
BASE = 2
N_BITS, N_STEPS, RHO = 5, 3, 0.7


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _layout():
    rng = np.random.Generator(np.random.PCG64(2024))
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    D = int(off[-1])
    tl = rng.standard_normal(D).astype(np.float32)
    ts = rng.uniform(0.3, 0.9, D).astype(np.float32)
    pl = (0.25 * rng.standard_normal(D)).astype(np.float32)
    ps = rng.uniform(0.8, 1.3, D).astype(np.float32)
    return off, tl, ts, pl, ps


def _greedy(oracle, n_bits=N_BITS, n_steps=N_STEPS, rho=RHO):
    off, tl, ts, pl, ps = _layout()
    return oracle.greedy_encode(tl, ts, pl, ps, off, n_bits, n_steps, R.wrap32(SEED), rho, BASE)


def test_seed_wraps():
    assert SEED + BASE + len(LENGTHS) > 2147483647 and BASE != 0


@pytest.mark.parametrize("n_bits,n_steps,rho", [(0, 2, 1.0), (1, 4, 0.7), (5, 3, 0.7), (5, 1, 1.0)])
def test_no_sweep_is_the_greedy_code(oracle, n_bits, n_steps, rho):
    off, tl, ts, pl, ps = _layout()
    gidx, gsample = _greedy(oracle, n_bits, n_steps, rho)
    idx, sample, values, accepted, _ = B.backfit(oracle, gidx, tl, ts, pl, ps, off, n_bits,
                                                 n_steps, SEED, 0, rho, BASE)
    assert np.array_equal(idx, gidx)
    assert np.array_equal(_u32(sample), _u32(gsample))
    assert values.shape == (len(LENGTHS), 1) and not accepted.any()
    # the value is the one the beam restatement reports for the greedy path
    _, _, bvalue = R.beam_encode(oracle, tl, ts, pl, ps, off, n_bits, n_steps, SEED, 1, rho, BASE)
    assert np.array_equal(_u32(values[:, 0]), _u32(bvalue))


def test_dec_is_the_oracles_decoder(oracle):
    off, tl, ts, pl, ps = _layout()
    rng = np.random.Generator(np.random.PCG64(3))
    table = rng.integers(0, 1 << N_BITS, (len(LENGTHS), N_STEPS)).astype(np.int32)
    _, sample, _, _, _ = B.backfit(oracle, table, tl, ts, pl, ps, off, N_BITS, N_STEPS, SEED, 0,
                                   RHO, BASE)
    want = oracle.greedy_decode(table, pl, ps, off, N_BITS, N_STEPS, R.wrap32(SEED), RHO, BASE)
    assert np.array_equal(_u32(sample), _u32(want))


def test_sweeps_never_lower_a_block_and_change_some(oracle):
    off, tl, ts, pl, ps = _layout()
    gidx, _ = _greedy(oracle)
    idx, sample, values, accepted, steps = B.backfit(oracle, gidx, tl, ts, pl, ps, off, N_BITS,
                                                     N_STEPS, SEED, 3, RHO, BASE)
    assert values.shape == (len(LENGTHS), 4)
    assert (np.diff(values, axis=1) >= 0).all()
    changed = [g for g in range(len(LENGTHS)) if steps[g][0]]
    assert len(changed) >= 1, "no block changes in sweep 1: the test shows nothing"
    assert (values[changed, 1] > values[changed, 0]).all()
    assert accepted.sum() == sum(len(a) for g in steps for a in steps[g])
    assert accepted[0] == 0 and values[0, 0] == 0.0  # the empty block
    # what comes out is what the decoder rebuilds
    back = oracle.greedy_decode(idx, pl, ps, off, N_BITS, N_STEPS, R.wrap32(SEED), RHO, BASE)
    assert np.array_equal(_u32(back), _u32(sample))
    assert idx.min() >= 0 and idx.max() < (1 << N_BITS)


def test_one_step_and_no_bits_never_change(oracle):
    off, tl, ts, pl, ps = _layout()
    for n_bits, n_steps in ((5, 1), (0, 3)):
        gidx, _ = _greedy(oracle, n_bits, n_steps, 1.0)
        idx, _, values, accepted, _ = B.backfit(oracle, gidx, tl, ts, pl, ps, off, n_bits,
                                                n_steps, SEED, 2, 1.0, BASE)
        assert np.array_equal(idx, gidx) and not accepted.any()
        assert (values == values[:, :1]).all()
