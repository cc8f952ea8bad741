"""GPU: k_encode_prune's static-stride refill and linked visit records.

A wave hands the first S(R) rows of its share of R rows to its lanes by stride
(lane l owns rows l, l + 64, ...) and the rest by rank among the finished
lanes (csrc/cwq_refill.h); the screening pass walks its LDS records by their
links.  Neither may change a result: prune_mode 0 (the exact kernel), 1 (the
pruned kernel's exact pass) and 2 (its screening pass) give the same indices
and the same sample words bit for bit, and mode 2 those of the CPU oracle on a
sample of the blocks.

Shapes: tests/prune_refill_shapes.py (tests/test_refill_plan.py checks on the
CPU which kernel each takes and its waves' shares: R = 64, 128, 256 and 1,024
in one-tile blocks, 64 and 256 in INTER tiles).
"""
import functools

import numpy as np
import pytest
import torch

import prune_refill_shapes as R

pytestmark = pytest.mark.gpu

SEED, BASE = 42, 3


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    return C


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind="normal"):
    """(t_loc, t_scale, p_loc, p_scale) flat float32 host arrays of a shape."""
    from compression_without_quantization_amd.synthetic import make_blocks
    d, bits, nb, _ = shape
    b = make_blocks(nb, d, bits, seed=700 + d + bits)
    tl, ts, pl, ps = (np.ascontiguousarray(b[k].reshape(-1)).copy() for k in
                      ("post_loc", "post_scale", "prior_loc", "prior_scale"))
    if kind == "flat_target":           # every row within rounding of every other: all complete
        ts[:] = np.float32(2.0 ** 40)
    elif kind == "posterior_is_prior":
        tl, ts = pl.copy(), ps.copy()
    elif kind == "huge_locs":           # outside the screening gate: these tiles take the exact pass
        pl = (np.float32(1.0e35) * np.where(pl < 0, -1, 1)).astype(np.float32)
        tl = pl.copy()
        ps = (np.abs(ps) * np.float32(1e33)).astype(np.float32)
        ts = ps.copy()
    else:
        assert kind == "normal"
    return tl, ts, pl, ps


def _encode(cwq, shape, host, prune):
    d, bits, nb, n_steps = shape
    dev = [torch.from_numpy(a).cuda() for a in host]
    idx, sample = cwq.encode_blocks(*dev, bits, n_steps, SEED, rho=1.0, block_dim=d,
                                    block_id_base=BASE, prune_mode=prune)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy().astype(np.int64)
    words = sample.cpu().numpy().view(np.uint32).copy()
    assert idx.shape == (nb, n_steps) and words.shape == (nb * d,)
    return idx, words


def _same(got, want, what):
    for name, g, w in zip(("indices", "sample words"), got, want):
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, f"{what}: {name}: {bad.size} of {w.size} differ, first at {bad[:8]}"


def _oracle_blocks(nb):
    if nb >= R.MANY:
        return np.unique(np.concatenate([np.arange(0, nb, R.ORACLE_STRIDE), [nb - 1]]))
    return np.unique(np.linspace(0, nb - 1, min(nb, 4)).astype(np.int64))


@functools.lru_cache(maxsize=None)
def _oracle(shape, kind="normal"):
    """(block numbers, indices, sample words) of a sample of the blocks from
    the CPU oracle, each coded alone under its own number."""
    from oracle import oracle as O
    d, bits, nb, n_steps = shape
    tl, ts, pl, ps = _inputs(shape, kind)
    blocks = _oracle_blocks(nb)
    wi = np.zeros((blocks.size, n_steps), np.int64)
    ww = np.zeros((blocks.size, d), np.uint32)
    for k, g in enumerate(blocks):
        sl = slice(g * d, (g + 1) * d)
        i, s = O.greedy_encode(tl[sl], ts[sl], pl[sl], ps[sl], [0, d], bits, n_steps, SEED, 1.0,
                               BASE + int(g))
        wi[k] = np.asarray(i).reshape(-1)
        ww[k] = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return blocks, wi, ww


def _check(cwq, oracle, shape, kind="normal"):
    host = _inputs(shape, kind)
    out = [_encode(cwq, shape, host, prune) for prune in (0, 1, 2)]
    _same(out[1], out[0], f"{shape} {kind}: mode 1 against mode 0")
    _same(out[2], out[0], f"{shape} {kind}: mode 2 against mode 0")
    blocks, wi, ww = _oracle(shape, kind)
    idx, words = out[2]
    _same((idx[blocks], words.reshape(-1, shape[0])[blocks]), (wi, ww),
          f"{shape} {kind}: mode 2 against the oracle")
    return out


@pytest.mark.parametrize("shape", R.SINGLE_TILE, ids=lambda s: "d%d_b%d" % s[:2])
def test_single_tile(cwq, oracle, shape):
    """16,384 one-tile blocks at d in {8, 32, 64} and 8, 9, 10 and 12 bits: a
    wave's share is 64 rows (no static region), 128 (one static row per lane,
    then the pool), 256 and 1,024; and d = 16 at 10 bits."""
    _check(cwq, oracle, shape)


@pytest.mark.parametrize("shape", R.INTER, ids=lambda s: "d%d_b%d_nb%d" % s[:3])
def test_inter_tiles(cwq, oracle, shape):
    """Several tiles per block: four blocks in tiles of 256 candidates at 12
    and 16 bits, and 64 blocks at 18 bits in tiles of 1,024 (a static region)
    whose last ones are cut in four; later tiles start from keys[g]'s value."""
    _check(cwq, oracle, shape)


@pytest.mark.parametrize("kind", ["flat_target", "posterior_is_prior", "huge_locs"])
def test_adversarial(cwq, oracle, kind):
    """d = 32 at 10 bits.  A flat target: every row completes and is kept, the
    survivor list fills to its last slot.  Posterior = prior.  Locations
    outside the screening gate: the exact pass runs the same refill."""
    _check(cwq, oracle, R.ADVERSARIAL, kind)


def test_flat_target_list_full(cwq):
    """The flat target at 12 bits, where the 4,096 rows of a tile pass the
    survivor list's 1,024 slots: the list-full branch scores rows in the loop."""
    shape = (32, 12, R.MANY, 1)
    host = _inputs(shape, "flat_target")
    out = [_encode(cwq, shape, host, prune) for prune in (0, 1, 2)]
    _same(out[1], out[0], "flat target, 12 bits: mode 1 against mode 0")
    _same(out[2], out[0], "flat target, 12 bits: mode 2 against mode 0")


def test_three_steps(cwq, oracle):
    """n_steps = 3: the second and third steps run the STEP0 = false instance."""
    _check(cwq, oracle, R.MULTI_STEP)
