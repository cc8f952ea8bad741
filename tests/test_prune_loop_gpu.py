"""GPU: k_encode_prune's screening loop and survivor phase.  The loop walks one
48-byte LDS record per visit position and carries each lane's row as a
pre-scaled Philox-block offset; survivors are scored with a lane per Philox
block.  Every case encodes with prune_mode 0 (k_encode_eval), 1 (exact pass)
and 2 (screening pass) and requires equal indices and equal sample words;
where 2^bits * d * nb <= 2^22 the CPU oracle judges as well."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 42


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    return C


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _encode(cwq, v, d, bits, n_steps, mode, seed=SEED, base=0):
    tl, ts, pl, ps = v
    i, s = cwq.encode_blocks(tl, ts, pl, ps, bits, n_steps, seed, block_dim=d,
                             block_id_base=base, prune_mode=mode)
    torch.cuda.synchronize()
    return i.cpu().numpy(), s.cpu().numpy()


def _check(cwq, oracle, v, d, bits, n_steps, seed=SEED, base=0, force_oracle=False):
    """Modes 1 and 2 against mode 0, and the oracle where it is affordable.
    Returns mode 2's (idx, sample)."""
    nb = v[0].size // d
    i0, s0 = _encode(cwq, v, d, bits, n_steps, 0, seed, base)
    for mode in (1, 2):
        i, s = _encode(cwq, v, d, bits, n_steps, mode, seed, base)
        assert np.array_equal(i, i0), f"indices, mode {mode} vs 0 (d={d}, bits={bits}, nb={nb})"
        assert np.array_equal(_u32(s), _u32(s0)), f"sample words, mode {mode} vs 0 (d={d})"
    if force_oracle or (1 << bits) * d * nb <= (1 << 22):
        wi, ws = oracle.greedy_encode(*v, np.arange(nb + 1) * d, bits, n_steps, seed, 1.0, base)
        assert np.array_equal(i, wi), f"indices vs oracle (d={d}, bits={bits}, nb={nb})"
        assert np.array_equal(_u32(s), _u32(ws)), f"sample words vs oracle (d={d})"
    return i, s


def _blocks(nb, d, bits, seed):
    from compression_without_quantization_amd.synthetic import make_blocks
    b = make_blocks(nb, d, bits, seed=seed)
    return tuple(b[k].reshape(-1) for k in ("post_loc", "post_scale", "prior_loc", "prior_scale"))


@pytest.mark.parametrize("d", [8, 16, 24, 32, 40, 48, 56, 64])
def test_every_block_dim_two_steps(cwq, oracle, d):
    """Each instantiation's record stride and completion test (G = d / 4 visit
    positions), at step 0 and with the carried best of step 1."""
    _check(cwq, oracle, _blocks(5, d, 11, 900 + d), d, 11, 2)


@pytest.mark.parametrize("nb", [16384, 16385])
def test_one_tile_per_block(cwq, oracle, nb):
    """One tile per block, many more tiles than resident workgroups: the
    non-interleaved instance, as the 10^6-block configuration runs it."""
    _check(cwq, oracle, _blocks(nb, 8, 8, 31), 8, 8, 1)


def _flat_target(nb, d, seed):
    """Posterior scale 2^20 x the prior's: the log-density is flat over the
    candidates to the last bit, so every completed row stays inside the
    bracket (4,096 rows against the 1,024-entry survivor list) and all rows of
    a block tie exactly."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pl = rng.standard_normal(nb * d).astype(np.float32)
    ps = rng.uniform(0.5, 2.0, nb * d).astype(np.float32)
    tl = (pl + 0.25 * ps * rng.standard_normal(nb * d)).astype(np.float32)
    ts = (ps * np.float32(2.0 ** 20)).astype(np.float32)
    return tl, ts, pl, ps


@pytest.mark.parametrize("d", [32, 8])
def test_many_survivors_and_ties(cwq, oracle, d):
    """Every row survives and the list overflows, so both the lane-parallel
    survivor phase and the in-loop exact path score rows; among equal values
    the lowest index wins.  The same blocks under a second (seed,
    block_id_base) pair with the same per-block seeds give the same result."""
    v = _flat_target(2, d, 5 + d)
    ia, sa = _check(cwq, oracle, v, d, 12, 1, seed=SEED, base=3, force_oracle=True)
    ib, sb = _check(cwq, oracle, v, d, 12, 1, seed=SEED - 4, base=7, force_oracle=True)
    assert np.array_equal(ia, ib)
    assert np.array_equal(_u32(sa), _u32(sb))


def test_gate_fails_exact_pass(cwq, oracle):
    """One sigma = 2^-70 per block: the screening gate fails, prune_mode 2
    runs the exact pass on those tiles."""
    nb, d = 4, 16
    tl, ts, pl, ps = (a.copy() for a in _blocks(nb, d, 10, 17))
    ts[np.arange(nb) * d + np.arange(nb) * 5] = np.float32(2.0 ** -70)
    _check(cwq, oracle, (tl, ts, pl, ps), d, 10, 1)


def test_prescaled_index_limit(cwq, oracle):
    """d = 64 at 20 bits: 2^24 Philox blocks per row set, sixteen per row, the
    largest pre-scaled row offsets of any instantiation."""
    _check(cwq, oracle, _blocks(1, 64, 20, 64020), 64, 20, 1)
