"""CPU: tests/beam_var_reference.py, the restatement of the beam encoder under
per-block bit budgets, is held to the oracle before the GPU tests trust it: at
beam 1 it is the oracle's greedy coder run on each block alone at that block's
bit count, indices and sample bit for bit."""
import numpy as np
import pytest

import beam_reference as R
import beam_var_reference as RV
from encode_shapes import ROWS_WAVE_LENGTHS as LENGTHS

SEED = 2147483647 - 5  # seed + base + g wraps past 2^31 - 1 inside the call
BASE = 3


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _layout():
    rng = np.random.Generator(np.random.PCG64(1717))
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    D = int(off[-1])
    tl = rng.standard_normal(D).astype(np.float32)
    ts = rng.uniform(0.3, 0.9, D).astype(np.float32)
    pl = (0.25 * rng.standard_normal(D)).astype(np.float32)
    ps = rng.uniform(0.8, 1.3, D).astype(np.float32)
    return off, tl, ts, pl, ps


def test_budgets_cover_the_range():
    bits = [(3 * g + 1) % 8 for g in range(len(LENGTHS))]
    assert set(bits) == set(range(8))
    assert SEED + BASE + len(LENGTHS) > 2147483647 and BASE != 0


@pytest.mark.parametrize("n_steps,rho", [(1, 1.0), (2, 0.7)])
def test_beam_one_is_the_greedy_coder_per_block(oracle, n_steps, rho):
    off, tl, ts, pl, ps = _layout()
    nb = len(off) - 1
    bits = np.array([(3 * g + 1) % 8 for g in range(nb)], np.int32)
    idx, sample, _ = RV.beam_encode_var(oracle, tl, ts, pl, ps, off, bits, n_steps, SEED, 1, rho,
                                        BASE)
    for g in range(nb):
        sl = slice(int(off[g]), int(off[g + 1]))
        one = np.array([0, off[g + 1] - off[g]], np.int64)
        # the block alone: block_id_base carries its place, seed + base + g
        widx, wsample = oracle.greedy_encode(tl[sl], ts[sl], pl[sl], ps[sl], one, int(bits[g]),
                                             n_steps, R.wrap32(SEED), rho, BASE + g)
        assert np.array_equal(idx[g], np.asarray(widx).reshape(-1)), g
        assert np.array_equal(_u32(sample[sl]), _u32(wsample)), g
        assert idx[g].max(initial=0) < (1 << int(bits[g]))


def test_equal_budgets_are_the_fixed_restatement(oracle):
    off, tl, ts, pl, ps = _layout()
    nb = len(off) - 1
    blocks = [0, 2, 5, 8, 10]
    got = RV.beam_encode_var(oracle, tl, ts, pl, ps, off, [4] * nb, 2, SEED, 3, 0.7, BASE, blocks)
    want = R.beam_encode(oracle, tl, ts, pl, ps, off, 4, 2, SEED, 3, 0.7, BASE, blocks)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(_u32(got[1]), _u32(want[1]))
    assert np.array_equal(_u32(got[2]), _u32(want[2]))
