"""GPU: the beam encoder (csrc/cwq_beam.hip) against tests/beam_reference.py,
the NumPy restatement that tests/test_beam_reference.py holds to the oracle.
Every comparison is bit for bit: int32 indices, uint32 views of samples and
values; no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import beam_reference as R
from encode_shapes import ROWS_WAVE_LENGTHS as LENGTHS
from poison import poisoned

pytestmark = pytest.mark.gpu

SEED = 2147483647 - 5  # seed + base + g wraps past 2^31 - 1 inside every call below
BASE = 3               # block_id_base


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    return C


def _u32(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _i32(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _values(rng, D):
    tl = rng.standard_normal(D).astype(np.float32)
    ts = rng.uniform(0.3, 0.9, D).astype(np.float32)
    pl = (0.25 * rng.standard_normal(D)).astype(np.float32)
    ps = rng.uniform(0.8, 1.3, D).astype(np.float32)
    return tl, ts, pl, ps


def _layout(lens, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return (off,) + _values(rng, int(off[-1]))


@functools.lru_cache(maxsize=None)
def _ragged():
    return _layout(LENGTHS, 1717)


SHORT_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 0, 15, 16, 17, 31, 33, 40, 63, 64]


@functools.lru_cache(maxsize=None)
def _short():
    return _layout(SHORT_LENGTHS, 88)


@functools.lru_cache(maxsize=None)
def _uniform(d, nb):
    return _layout([d] * nb, 1000 + d)


@functools.lru_cache(maxsize=None)
def _reference(layout, n_bits, n_steps, beam, rho, seed, base, blocks=None):
    """The helper's (idx, sample bits, value bits), computed once per case."""
    from oracle import oracle as O
    O.build()
    off, tl, ts, pl, ps = layout()
    idx, sample, value = R.beam_encode(O, tl, ts, pl, ps, off, n_bits, n_steps, seed, beam, rho,
                                       base, blocks)
    return idx, _u32(sample), _u32(value)


def _same(got, want, blocks=None, off=None):
    """got: encode_blocks_beam's triple; want: _reference's."""
    gi, gs, gv = _i32(got[0]), _u32(got[1]), _u32(got[2])
    if blocks is None:
        assert np.array_equal(gi, want[0]), np.flatnonzero((gi != want[0]).any(axis=1))
        assert np.array_equal(gs, want[1])
        assert np.array_equal(gv, want[2]), np.flatnonzero(gv != want[2])
        return
    for g in blocks:
        sl = slice(int(off[g]), int(off[g + 1]))
        assert np.array_equal(gi[g], want[0][g]), g
        assert np.array_equal(gs[sl], want[1][sl]), g
        assert gv[g] == want[2][g], g


def test_inputs_cover_the_paths(cwq):
    assert cwq.beam.MAX_BEAM == 16 and max(c[0] for c in RAGGED_CASES) == cwq.beam.MAX_BEAM
    lens = np.diff(_ragged()[0])
    assert set(lens.tolist()) == {0, 1, 3, 4, 5, 7, 8, 9, 247, 248, 249, 255, 256, 257, 496, 1023,
                                  1025, 4095}
    assert SEED + BASE + len(lens) > 2147483647 and BASE != 0
    assert max(SHORT_LENGTHS) == 64 and 0 in SHORT_LENGTHS and min(SHORT_LENGTHS[:8]) == 1


# ---------------------------------------------------------------------------
# beam 1 is the greedy coder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("shape", [8, 13, 32, "ragged"])
def test_beam_one_equals_encode_blocks(cwq, shape, n_steps):
    if shape == "ragged":
        off, tl, ts, pl, ps = _ragged()
        kw, n_bits = dict(block_off=off), 5
    else:
        off, tl, ts, pl, ps = _uniform(shape, 40)
        kw, n_bits = dict(block_dim=shape), 7
    idx, sample = cwq.encode_blocks_beam(tl, ts, pl, ps, n_bits, n_steps, SEED, 1, rho=0.7,
                                         block_id_base=BASE, **kw)
    for mode in (0, 2):
        widx, wsample = cwq.encode_blocks(tl, ts, pl, ps, n_bits, n_steps, SEED, rho=0.7,
                                          block_id_base=BASE, prune_mode=mode, **kw)
        assert np.array_equal(_i32(idx), _i32(widx)), mode
        assert np.array_equal(_u32(sample), _u32(wsample)), mode


# ---------------------------------------------------------------------------
# beams against the restatement, ragged blocks (the wave-per-row kernel)
# ---------------------------------------------------------------------------
# b = 0: one beam for ever.  b = 1, B = 8: the live beams go 1, 2, 4, 8 and the
# candidates are fewer than B.  b = 6: 18 blocks x 64 rows, fewer rows than the
# grid's waves.
RAGGED_CASES = [(2, 0, 2, 1.0), (2, 1, 1, 1.0), (8, 1, 4, 0.7), (3, 3, 2, 1.0), (16, 3, 4, 0.7),
                (16, 6, 2, 1.0), (3, 6, 4, 0.7), (8, 6, 1, 1.0)]


@pytest.mark.parametrize("beam,n_bits,n_steps,rho", RAGGED_CASES)
def test_ragged_vs_reference(cwq, beam, n_bits, n_steps, rho):
    off, tl, ts, pl, ps = _ragged()
    got = cwq.encode_blocks_beam(tl, ts, pl, ps, n_bits, n_steps, SEED, beam, rho=rho,
                                 block_off=off, block_id_base=BASE, return_value=True)
    want = _reference(_ragged, n_bits, n_steps, beam, rho, SEED, BASE)
    _same(got, want)
    empty = np.flatnonzero(np.diff(off) == 0)
    assert (_i32(got[0])[empty] == 0).all() and (_u32(got[2])[empty] == 0).all()  # value +0
    back = cwq.decode_blocks(got[0], pl, ps, n_bits, n_steps, SEED, rho=rho, block_off=off,
                             block_id_base=BASE)
    assert np.array_equal(_u32(back), _u32(got[1]))


# ---------------------------------------------------------------------------
# both kernels on the same input
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("beam,n_bits,n_steps", [(5, 4, 3), (16, 8, 2)])
def test_both_kernels_same_bits(cwq, beam, n_bits, n_steps):
    """Blocks of 0 - 64 dims on the lane-per-row kernel (path 0), the
    wave-per-row kernel (1), and both with tiles a quarter of the size (2, 3);
    2^8 rows make the lane kernel loop over its tile."""
    off, tl, ts, pl, ps = _short()
    want = _reference(_short, n_bits, n_steps, beam, 1.0, SEED, BASE)
    for path in (None, 0, 1, 2, 3):
        got = cwq.encode_blocks_beam(tl, ts, pl, ps, n_bits, n_steps, SEED, beam, block_off=off,
                                     block_id_base=BASE, return_value=True, _path=path)
        _same(got, want)


# ---------------------------------------------------------------------------
# uniform blocks; more tiles than the grid holds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d,nb,n_bits,beam", [(8, 300, 5, 4), (12, 300, 5, 4), (32, 300, 5, 4),
                                              (64, 300, 5, 4), (72, 300, 5, 4),
                                              (5, 5000, 3, 3)])
def test_uniform_vs_reference(cwq, d, nb, n_bits, beam):
    """The restatement on 24 sampled blocks; on all blocks the decoder rebuilds
    the sample from the indices.  5,000 blocks are 5,000 tiles, more than the
    4,096 workgroups a scoring launch is capped at: tiles are strided."""
    n_steps = 2
    off, tl, ts, pl, ps = _uniform(d, nb)
    blocks = tuple(sorted(np.random.Generator(np.random.PCG64(d)).choice(nb, 24, replace=False)
                          .tolist() + [0, nb - 1]))
    got = cwq.encode_blocks_beam(tl, ts, pl, ps, n_bits, n_steps, SEED, beam, rho=0.7,
                                 block_dim=d, block_id_base=BASE, return_value=True)
    want = _reference(functools.partial(_uniform, d, nb), n_bits, n_steps, beam, 0.7, SEED, BASE,
                      blocks)
    _same(got, want, blocks, off)
    back = cwq.decode_blocks(got[0], pl, ps, n_bits, n_steps, SEED, rho=0.7, block_dim=d,
                             block_id_base=BASE)
    assert np.array_equal(_u32(back), _u32(got[1]))
    idx = _i32(got[0])
    assert idx.min() >= 0 and idx.max() < (1 << n_bits)


# ---------------------------------------------------------------------------
# adversarial blocks
# ---------------------------------------------------------------------------
def _adversarial(lens):
    rng = np.random.Generator(np.random.PCG64(99))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tl, ts, pl, ps = _values(rng, int(off[-1]))
    tl[off[0] + lens[0] - 5] = np.nan  # every candidate's value is NaN
    ps[off[1]:off[2]] = 0.0            # scale_s == 0: every candidate ties, beams hold equal sums
    tl[off[2] + 8] = np.inf            # every candidate at -inf
    return off, tl, ts, pl, ps


@functools.lru_cache(maxsize=None)
def _adversarial_long():
    return _adversarial([300, 257, 9, 300, 257, 64])  # test_rows_wave_adversarial's blocks


@functools.lru_cache(maxsize=None)
def _adversarial_short():
    return _adversarial([40, 33, 9, 40, 33, 64])


@pytest.mark.parametrize("layout,paths", [(_adversarial_long, (None,)),
                                          (_adversarial_short, (0, 1))])
def test_adversarial(cwq, layout, paths):
    """Ties resolve to the lowest candidate (k, r): a block whose candidates all
    tie keeps beams (0, 0), (0, 1), ... with bit-equal sums and yields indices 0."""
    off, tl, ts, pl, ps = layout()
    want = _reference(layout, 5, 2, 4, 1.0, 42, 0)
    assert (want[0][:3] == 0).all() and (want[0][3:] != 0).any()
    for path in paths:
        got = cwq.encode_blocks_beam(tl, ts, pl, ps, 5, 2, 42, 4, block_off=off,
                                     return_value=True, _path=path)
        _same(got, want)


# ---------------------------------------------------------------------------
# determinism: the same call twice, and with tiles a quarter of the size
# ---------------------------------------------------------------------------
def test_deterministic_and_tiling_independent(cwq):
    off, tl, ts, pl, ps = _ragged()
    runs = [cwq.encode_blocks_beam(tl, ts, pl, ps, 6, 3, SEED, 8, block_off=off,
                                   block_id_base=BASE, return_value=True, _path=p)
            for p in (None, None, 1, 3)]
    u = _uniform(32, 10)
    runs_u = [cwq.encode_blocks_beam(u[1], u[2], u[3], u[4], 9, 3, SEED, 8, block_dim=32,
                                     return_value=True, _path=p) for p in (None, None, 0, 2)]
    for rs in (runs, runs_u):
        for r in rs[1:]:
            assert np.array_equal(_i32(r[0]), _i32(rs[0][0]))
            assert np.array_equal(_u32(r[1]), _u32(rs[0][1]))
            assert np.array_equal(_u32(r[2]), _u32(rs[0][2]))


# ---------------------------------------------------------------------------
# workspace and output buffers: their contents on entry never matter
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0x00, 0xFF, "random", "guard"])
def test_poisoned_workspace_and_outputs(cwq, cwqlib, pattern):
    """The "guard" case: zeros between guard bands (tests/poison.py), which must stay intact."""
    guard = pattern == "guard"
    pattern = 0x00 if guard else pattern
    off, tl, ts, pl, ps = _ragged()
    want = _reference(_ragged, 3, 4, 16, 0.7, SEED, BASE)  # a case of test_ragged_vs_reference
    nb, D = len(off) - 1, int(off[-1])
    with poisoned(pattern, guard=guard) as f:
        got = cwq.encode_blocks_beam(tl, ts, pl, ps, 3, 4, SEED, 16, rho=0.7, block_off=off,
                                     block_id_base=BASE, return_value=True)
        torch.cuda.synchronize()
        assert f.assert_guards_intact("beam") >= int(guard)
    f.assert_workspace(int(cwqlib.cwq_beam_encode_workspace_size(nb, D, 4095, 4, 16)), "beam")
    assert f.count("device", torch.int32, 4 * nb * 4) >= 1   # out_idx was poisoned too
    _same(got, want)
    s = _short()
    want_s = _reference(_short, 4, 3, 5, 1.0, SEED, BASE)  # a case of test_both_kernels_same_bits
    with poisoned(pattern, guard=guard) as f:
        got_s = cwq.encode_blocks_beam(s[1], s[2], s[3], s[4], 4, 3, SEED, 5, block_off=s[0],
                                       block_id_base=BASE, return_value=True)
        torch.cuda.synchronize()
        assert f.assert_guards_intact("beam, short blocks") >= int(guard)
    _same(got_s, want_s)


def test_back_to_back_on_one_workspace(cwq, cwqlib):
    """B = 8 then B = 2 on other shapes, one uncleared workspace, stream order only."""
    a, b = _ragged(), _short()
    need = max(int(cwqlib.cwq_beam_encode_workspace_size(len(a[0]) - 1, int(a[0][-1]), 4095, 2, 8)),
               int(cwqlib.cwq_beam_encode_workspace_size(len(b[0]) - 1, int(b[0][-1]), 64, 3, 2)))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = cwq.encode_blocks_beam(a[1], a[2], a[3], a[4], 6, 2, SEED, 8, block_off=a[0],
                                       block_id_base=BASE, return_value=True, workspace=ws)
        second = cwq.encode_blocks_beam(b[1], b[2], b[3], b[4], 4, 3, SEED, 2, block_off=b[0],
                                        block_id_base=BASE, return_value=True, workspace=ws)
        again = cwq.encode_blocks_beam(a[1], a[2], a[3], a[4], 6, 2, SEED, 8, block_off=a[0],
                                       block_id_base=BASE, return_value=True, workspace=ws)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    alone_a = cwq.encode_blocks_beam(a[1], a[2], a[3], a[4], 6, 2, SEED, 8, block_off=a[0],
                                     block_id_base=BASE, return_value=True)
    alone_b = cwq.encode_blocks_beam(b[1], b[2], b[3], b[4], 4, 3, SEED, 2, block_off=b[0],
                                     block_id_base=BASE, return_value=True)
    for got, want in ((first, alone_a), (second, alone_b), (again, alone_a)):
        for x, y in zip(got, want):
            assert np.array_equal(_u32(x) if x.dtype == torch.float32 else _i32(x),
                                  _u32(y) if y.dtype == torch.float32 else _i32(y))
    _same(second, _reference(_short, 4, 3, 2, 1.0, SEED, BASE))


def _raw(cwqlib, t, n_bits, n_steps, beam, ws_bytes=None, stream=None):
    """cwq_beam_encode on tensors made beforehand (t: dict); returns the code."""
    return cwqlib.cwq_beam_encode(
        t["tl"].data_ptr(), t["ts"].data_ptr(), t["pl"].data_ptr(), t["ps"].data_ptr(),
        t["off"].data_ptr(), t["nb"], t["D"], t["longest"], n_bits, n_steps, beam,
        R.wrap32(SEED), 1.0, BASE, t["idx"].data_ptr(), t["sample"].data_ptr(),
        t["value"].data_ptr(), t["ws"].data_ptr(), t["ws"].numel() if ws_bytes is None else ws_bytes,
        None, torch.cuda.current_stream().cuda_stream if stream is None else stream)


def _tensors(cwqlib, layout, n_steps, beam):
    off, tl, ts, pl, ps = layout
    dev = torch.device("cuda")
    nb, D = len(off) - 1, int(off[-1])
    longest = int(np.diff(off).max())
    f = lambda a: torch.from_numpy(a).to(dev)
    need = int(cwqlib.cwq_beam_encode_workspace_size(nb, D, longest, n_steps, beam))
    return dict(tl=f(tl), ts=f(ts), pl=f(pl), ps=f(ps), off=f(off), nb=nb, D=D, longest=longest,
                idx=torch.full((nb, n_steps), -77, dtype=torch.int32, device=dev),
                sample=torch.full((D,), -77.0, device=dev),
                value=torch.full((nb,), -77.0, device=dev), need=need,
                ws=torch.empty(need, dtype=torch.uint8, device=dev))


def test_argument_errors(cwqlib):
    t = _tensors(cwqlib, _short(), 2, 4)
    assert _raw(cwqlib, t, 4, 2, 4, ws_bytes=t["need"] - 1) == -3
    assert b"workspace" in cwqlib.cwq_last_error()
    for beam in (0, 17):
        assert _raw(cwqlib, t, 4, 2, beam) == -1 and b"beam" in cwqlib.cwq_last_error()
    assert _raw(cwqlib, t, 30, 2, 4) == -1 and b"2^31" in cwqlib.cwq_last_error()
    torch.cuda.synchronize()
    assert (t["idx"] == -77).all() and (t["sample"] == -77).all()  # nothing was launched
    assert _raw(cwqlib, t, 4, 2, 4) == 0
    torch.cuda.synchronize()
    assert (t["idx"] >= 0).all()


# ---------------------------------------------------------------------------
# HIP graph: one beam encode captured on one stream
# ---------------------------------------------------------------------------
def test_graph_capture_and_replay(cwqlib):
    t = _tensors(cwqlib, _ragged(), 3, 4)
    assert _raw(cwqlib, t, 5, 3, 4) == 0
    torch.cuda.synchronize()
    outs = (t["idx"], t["sample"], t["value"])
    want = [x.clone() for x in outs]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert _raw(cwqlib, t, 5, 3, 4) == 0
    for _ in range(2):
        for x in outs:
            x.fill_(-5)
        t["ws"].fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        for got, w in zip(outs, want):
            assert torch.equal(got.view(torch.int32), w.view(torch.int32))
    ref = _reference(_ragged, 5, 3, 4, 1.0, SEED, BASE)
    _same(outs, ref)


# ---------------------------------------------------------------------------
# the grouped wrapper
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _latent():
    """3,000 dims whose partition (2 steps x 6 bits: a group closes at 7.3 nats)
    has groups of one dim (a dim of 8 nats on its own), of more than 64 dims
    (dims of 0.005 nats) and the one-dim last group the end closes."""
    rng = np.random.Generator(np.random.PCG64(7))
    D = 3000
    pl = rng.standard_normal(D).astype(np.float32)
    ps = rng.uniform(0.5, 2.0, D).astype(np.float32)
    delta = np.where(np.arange(D) < 1500, 0.1, rng.uniform(0.5, 1.5, D))
    delta[[100, 1700, 1701, 2500]] = 4.0
    ql = (pl + delta * ps * rng.choice([-1.0, 1.0], D)).astype(np.float32)
    qs = (ps * np.where(np.arange(D) < 1500, 1.0, rng.uniform(0.4, 0.9, D))).astype(np.float32)
    return ql, qs, pl, ps


def test_grouped_wrapper(cwq, oracle):
    ql, qs, pl, ps = _latent()
    n_steps, n_bits, seed, rho = 2, 6, 11, 1.0
    tl, ts = oracle.standardise(ql, qs, pl, ps)
    kl = oracle.kl_normal_normal(ql, qs, pl, ps)
    starts = oracle.group_starts(kl, n_bits * n_steps, cwq.group_size_threshold(12))
    sizes = np.diff(starts)
    assert (sizes == 1).sum() >= 3 and sizes.max() > 64 and starts[-2] == 2999
    target, proposal = cwq.Normal(ql, qs), cwq.Normal(pl, ps)
    # beam 1: the greedy wrapper's triple
    s1, c1, g1 = cwq.code_grouped_greedy_sample_beam(target, proposal, n_steps, n_bits, seed, 1)
    ws, wc, wg = cwq.code_grouped_greedy_sample(None, target, proposal, n_steps, n_bits, seed)
    assert np.array_equal(_u32(s1), _u32(ws)) and c1 == wc and list(g1) == list(wg)
    # beam 4: the oracle's pipeline around the restatement
    s4, c4, g4 = cwq.code_grouped_greedy_sample_beam(target, proposal, n_steps, n_bits, seed, 4,
                                                     rho=rho)
    assert list(g4) == list(starts)
    D = ql.size
    idx, samp, _ = R.beam_encode(oracle, tl, ts, np.zeros(D, np.float32), np.ones(D, np.float32),
                                 starts, n_bits, n_steps, seed, 4, rho, 0)
    assert c4 == cwq.indices_to_bitcode(idx, n_bits)
    assert np.array_equal(_u32(s4), _u32(oracle.destandardise(samp, pl, ps)))
    assert c4 != c1 and len(c4) == len(c1)  # the same bits spent, another path
    back = cwq.decode_grouped_greedy_sample(None, c4, g4[:-1], proposal, n_bits, n_steps, seed)
    assert np.array_equal(_u32(back), _u32(s4))


# ---------------------------------------------------------------------------
# the PLN codec
# ---------------------------------------------------------------------------
def test_pln_beam_width(cwq, oracle, tmp_path):
    """test_pln_gpu.py's smallest image and settings: beam_width=4 writes a
    file of the plain call's size that decode_image_greedy reads back to the
    encoder's latents; beam_width=1 gives the plain call's bytes."""
    import test_pln_gpu as T
    P = cwq.pln
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    model = T._model(P, seed=4)
    img = T._image(64, 64, seed=5)
    plain, one, four = (str(tmp_path / n) for n in ("plain.miracle", "one.miracle", "four.miracle"))
    (p2, p1), _ = model.code_image_greedy(None, img, 3, comp_file_path=plain, **T.KW)
    (o2, o1), _ = model.code_image_greedy(None, img, 3, comp_file_path=one, beam_width=1, **T.KW)
    (f2, f1), _ = model.code_image_greedy(None, img, 3, comp_file_path=four, beam_width=4, **T.KW)
    assert open(one, "rb").read() == open(plain, "rb").read()
    T._eq(o1, p1, "level-1 sample, beam_width=1")
    T._eq(f2, p2, "level-2 sample")
    assert len(open(four, "rb").read()) == len(open(plain, "rb").read())
    rec = model.decode_image_greedy(None, four, use_importance_sampling=False,
                                    greedy_max_group_size_bits=12,
                                    first_level_max_group_size_bits=4,
                                    second_level_max_group_size_bits=2)
    shape1 = tuple(model.latent_distributions(img, 3)["q1"].loc.shape)
    perm1, _ = oracle.pln_permutations(3, int(np.prod(shape1)), 1)
    z1 = P.unpermute_unflatten(torch.from_numpy(np.asarray(f1, np.float32)).cuda(),
                               torch.from_numpy(perm1).cuda(), shape1)
    with torch.no_grad():
        want = model.synthesis_transform_1(z1)[0].permute(1, 2, 0).cpu().numpy()
    T._eq(rec, want, "reconstruction from the beam file")
    for kw in (dict(use_importance_sampling=True), dict(first_level_group_bits=True)):
        with pytest.raises(ValueError, match="beam_width"):
            model.code_image_greedy(None, img, 3, beam_width=2, **{**T.KW, **kw})
