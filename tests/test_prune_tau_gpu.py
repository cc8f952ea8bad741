"""GPU: k_encode_prune with a wave-uniform threshold.

The pruned kernel raises tau for the whole wave when a row completes, pushes
to the survivor list only the completed rows whose upper end reaches the raised
tau, and shares tau between a workgroup's waves through one returning LDS float
max.  None of that may change a result: prune_mode 0 (the exact kernel), 1 (the
pruned kernel's exact pass) and 2 (its screening pass) give the same indices and
the same sample words, and mode 2 those of the CPU oracle.

Shapes: tests/prune_tau_shapes.py (tests/test_prune_tau_plan.py checks on the
CPU that each takes the uniform pruned kernel, and how it is tiled).
"""
import functools

import numpy as np
import pytest
import torch

import prune_tau_shapes as P
from poison import poisoned

pytestmark = pytest.mark.gpu

SEED, BASE = 42, 3
PATTERNS = (0x00, 0xFF, "random")


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
    b = make_blocks(nb, d, bits, seed=500 + d + bits)
    tl, ts, pl, ps = (np.ascontiguousarray(b[k].reshape(-1)).copy() for k in
                      ("post_loc", "post_scale", "prior_loc", "prior_scale"))
    if kind == "tied_zero_scale":      # every candidate is the same point
        ps[:] = 0.0
    elif kind == "tied_wide_target":   # values differ far below one ulp of their sum
        ts[:] = np.float32(2.0 ** 40)
    elif kind == "nan_block":          # block 1 of 3 has one NaN location
        tl[d + d // 2] = np.float32("nan")
    else:
        assert kind == "normal"
    return tl, ts, pl, ps


def _encode(cwq, shape, host, prune, workspace=None):
    d, bits, nb, n_steps = shape
    dev = [torch.from_numpy(a).cuda() for a in host]
    idx, sample = cwq.encode_blocks(*dev, bits, n_steps, SEED, rho=1.0, block_dim=d,
                                    block_id_base=BASE, prune_mode=prune, workspace=workspace)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy().astype(np.int64)
    words = sample.cpu().numpy().view(np.uint32).copy()
    assert idx.shape == (nb, n_steps) and words.shape == (nb * d,)
    return idx, words


def _same(got, want, what):
    for name, g, w in zip(("indices", "sample words"), got, want):
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, f"{what}: {name}: {bad.size} of {w.size} differ, first at {bad[:8]}"


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """(block numbers, indices, sample words of those blocks) from the CPU
    oracle: every block, or of P.MANY blocks every P.ORACLE_STRIDE-th and the
    last, each coded alone under its own number (the same seed as in the call)."""
    from oracle import oracle as O
    d, bits, nb, n_steps = shape
    tl, ts, pl, ps = _inputs(shape)
    blocks = np.arange(nb) if nb < P.MANY else \
        np.unique(np.concatenate([np.arange(0, nb, P.ORACLE_STRIDE), [nb - 1]]))
    wi = np.zeros((blocks.size, n_steps), np.int64)
    ww = np.zeros((blocks.size, d), np.uint32)
    for k, g in enumerate(blocks):
        sl = slice(g * d, (g + 1) * d)
        i, s = O.greedy_encode(tl[sl], ts[sl], pl[sl], ps[sl], [0, d], bits, n_steps, SEED, 1.0,
                               BASE + int(g))
        wi[k] = np.asarray(i).reshape(-1)
        ww[k] = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return blocks, wi, ww


def _check_oracle(got, shape, what):
    d = shape[0]
    blocks, wi, ww = _oracle(shape)
    idx, words = got
    _same((idx[blocks], words.reshape(-1, d)[blocks]), (wi, ww), what + " against the oracle")


def _three_modes(cwq, shape, kind="normal"):
    host = _inputs(shape, kind)
    out = [_encode(cwq, shape, host, prune) for prune in (0, 1, 2)]
    _same(out[1], out[0], f"{shape} {kind}: mode 1 against mode 0")
    _same(out[2], out[0], f"{shape} {kind}: mode 2 against mode 0")
    return out


@pytest.mark.parametrize("shape", P.MODES_CASES,
                         ids=lambda s: "d%d_b%d_nb%d_s%d" % s)
def test_modes_agree_and_match_oracle(cwq, oracle, shape):
    """One step at d in {8, 32, 64} with tiles of 2^4, 2^8 and 2^12 candidates
    (most lanes idle; one row per lane, all completing at once against
    tau = -inf; refills and several shares), the workload's own 2^16-candidate
    tile at d = 32 and four of its blocks alone, two steps at d = 16 (STEP0
    false) in whole tiles and in INTER tiles, and two more INTER shapes (2
    tiles per block, the fewest; 4,096 tiles per block, where later tiles start
    from keys[g])."""
    out = _three_modes(cwq, shape)
    _check_oracle(out[2], shape, f"{shape}: mode 2")


@pytest.mark.parametrize("kind", ["tied_zero_scale", "tied_wide_target"])
@pytest.mark.parametrize("shape", P.TIED, ids=lambda s: "d%d_b%d" % s[:2])
def test_all_rows_tied(cwq, shape, kind):
    """Every candidate has the same value, so every row reaches every tau: more
    than CWQ_SURVIVOR_CAP rows are kept (the list-full path) and the first one
    wins, in each of the 16,384 one-tile blocks.  Zero proposal scale: all rows
    are the same point (whichever pass the range gate gives the tile).  Target
    scale 2^40 with finite locations: the rows differ, but far below the
    rounding of their values, and the tile passes the gate."""
    d, bits, nb, n_steps = shape
    assert (1 << bits) > 1024  # CWQ_SURVIVOR_CAP
    for idx, _ in _three_modes(cwq, shape, kind):
        assert (idx == 0).all(), f"{shape} {kind}: {idx.reshape(-1)}"


def test_nan_block(cwq, oracle):
    """A NaN location makes every row of its block NaN: no row is dropped, none
    is kept, and the block's index is the argmax's start, 0, as in mode 0.  The
    other blocks are untouched."""
    shape = P.NAN_BLOCK
    d, bits, nb, n_steps = shape
    out = _three_modes(cwq, shape, "nan_block")
    _, want_i, want_w = _oracle(shape)
    for idx, words in out:
        assert (idx[1] == 0).all()
        for g in (0, 2):
            assert np.array_equal(idx[g], want_i[g])
            assert np.array_equal(words[g * d:(g + 1) * d], want_w[g])


def test_back_to_back_on_one_workspace(cwq, cwqlib, oracle):
    """Modes 2, 1, 2 of both shapes in turn on one workspace that nothing
    clears: the threshold cell, the survivor count and the keys are written by
    each call before it reads them."""
    need = max(int(cwqlib.cwq_greedy_encode_uniform_workspace_size(nb, d))
               for d, _, nb, _ in P.WORKSPACE)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        for shape in P.WORKSPACE:
            for prune in (2, 1, 2):
                got = _encode(cwq, shape, _inputs(shape), prune, workspace=ws)
                _check_oracle(got, shape, f"{shape} mode {prune} on a used workspace")


@pytest.mark.parametrize("shape", P.WORKSPACE, ids=lambda s: "d%d_b%d" % s[:2])
def test_poisoned_buffers(cwq, oracle, shape):
    """Every buffer the wrapper allocates filled with 0x00, 0xFF and seeded
    random bytes: the same results, the oracle's."""
    for prune in (1, 2):
        for p in PATTERNS:
            with poisoned(p) as filled:
                got = _encode(cwq, shape, _inputs(shape), prune)
            assert filled.count("device") >= 1
            _check_oracle(got, shape, f"{shape} mode {prune} pattern {p!r}")
