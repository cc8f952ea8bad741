"""GPU: backfitting (csrc/cwq_backfit.hip) against tests/backfit_reference.py,
the NumPy restatement that tests/test_backfit_reference.py holds to the oracle.
Every comparison is bit for bit: int32 indices and counts, uint32 views of
samples and values; no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import backfit_reference as B
import beam_reference as R
import encode_shapes as S
from poison import poisoned
from test_beam_gpu import SHORT_LENGTHS

pytestmark = pytest.mark.gpu

SEED = 2147483647 - 5  # seed + base + g wraps past 2^31 - 1 inside every call below
BASE = 3               # block_id_base


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    return C


class _Fn:
    """f(*args) as a hashable call, equal when f and args are: a key for the
    caches below (functools.partial objects compare by identity)."""

    def __init__(self, f, *args):
        self.key = (f, args)

    def __call__(self):
        return self.key[0](*self.key[1])

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return isinstance(other, _Fn) and self.key == other.key


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


@functools.lru_cache(maxsize=None)
def _layout(lens, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return (off,) + _values(rng, int(off[-1]))


def _ragged():
    return _layout(tuple(S.ROWS_WAVE_LENGTHS), 1717)


def _short():
    return _layout(tuple(SHORT_LENGTHS), 88)


def _uniform(d, nb):
    return _layout((d,) * nb, 1000 + d)


def _kw(layout, uniform_d=None):
    return dict(block_dim=uniform_d) if uniform_d else dict(block_off=layout[0])


@functools.lru_cache(maxsize=None)
def _greedy_table(layout, n_bits, n_steps, rho, seed, base):
    """encode_blocks' table for the layout (a host copy), once per case."""
    import compression_without_quantization_amd as C
    off, tl, ts, pl, ps = layout()
    idx, _ = C.encode_blocks(tl, ts, pl, ps, n_bits, n_steps, seed, rho=rho, block_off=off,
                             block_id_base=base)
    return idx.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(layout, table, n_bits, n_steps, sweeps, rho, seed, base, blocks=None):
    """The helper from table() (a function returning the host table): (idx,
    sample bits, values [nb, sweeps + 1], accepted, steps), once per case."""
    from oracle import oracle as O
    O.build()
    off, tl, ts, pl, ps = layout()
    idx, sample, values, accepted, steps = B.backfit(O, table(), tl, ts, pl, ps, off, n_bits,
                                                     n_steps, seed, sweeps, rho, base, blocks)
    return idx, _u32(sample), values, accepted, steps


def _same(got, want, blocks=None, off=None):
    """got: backfit_blocks' (idx, sample, value, accepted); want: _reference's."""
    gi, gs, gv, ga = _i32(got[0]), _u32(got[1]), _u32(got[2]), _i32(got[3])
    wv = _u32(want[2][:, -1])
    if blocks is None:
        assert np.array_equal(gi, want[0]), np.flatnonzero((gi != want[0]).any(axis=1))
        assert np.array_equal(gs, want[1])
        assert np.array_equal(gv, wv), np.flatnonzero(gv != wv)
        assert np.array_equal(ga, want[3]), np.flatnonzero(ga != want[3])
        return
    for g in blocks:
        sl = slice(int(off[g]), int(off[g + 1]))
        assert np.array_equal(gi[g], want[0][g]), g
        assert np.array_equal(gs[sl], want[1][sl]), g
        assert gv[g] == wv[g] and ga[g] == want[3][g], g


def _run(cwq, layout, table, n_bits, n_steps, sweeps, rho, uniform_d=None, **kw):
    off, tl, ts, pl, ps = layout
    return cwq.backfit_blocks(table, tl, ts, pl, ps, n_bits, n_steps, SEED, sweeps, rho=rho,
                              block_id_base=BASE, return_value=True, return_accepted=True,
                              **_kw(layout, uniform_d), **kw)


def _decodes(cwq, layout, got, n_bits, n_steps, rho, uniform_d=None, seed=SEED, base=BASE):
    off, tl, ts, pl, ps = layout
    back = cwq.decode_blocks(got[0], pl, ps, n_bits, n_steps, seed, rho=rho, block_id_base=base,
                             **_kw(layout, uniform_d))
    assert np.array_equal(_u32(back), _u32(got[1]))


# ---------------------------------------------------------------------------
# no sweep: the table, its sample and its value
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [8, 13, 32, "ragged"])
def test_no_sweep_returns_the_table(cwq, shape):
    if shape == "ragged":
        layout, d, n_bits = _ragged(), None, 5
    else:
        layout, d, n_bits = _uniform(shape, 40), shape, 7
    off, tl, ts, pl, ps = layout
    kw = dict(rho=0.7, block_id_base=BASE, **_kw(layout, d))
    idx, sample = cwq.encode_blocks(tl, ts, pl, ps, n_bits, 3, SEED, **kw)
    got = cwq.backfit_blocks(idx, tl, ts, pl, ps, n_bits, 3, SEED, 0, return_value=True,
                             return_accepted=True, **kw)
    _, _, value = cwq.encode_blocks_beam(tl, ts, pl, ps, n_bits, 3, SEED, 1, return_value=True,
                                         **kw)
    assert np.array_equal(_i32(got[0]), _i32(idx))
    assert np.array_equal(_u32(got[1]), _u32(sample))
    assert np.array_equal(_u32(got[2]), _u32(value))
    assert not _i32(got[3]).any()
    both = cwq.encode_blocks_backfit(tl, ts, pl, ps, n_bits, 3, SEED, 0, **kw)
    assert np.array_equal(_i32(both[0]), _i32(idx)) and np.array_equal(_u32(both[1]), _u32(sample))


# ---------------------------------------------------------------------------
# against the restatement
# ---------------------------------------------------------------------------
LAYOUTS = {"u8": (_Fn(_uniform, 8, 300), 8),
           "u13": (_Fn(_uniform, 13, 300), 13),
           "u32": (_Fn(_uniform, 32, 300), 32),
           "ragged": (_ragged, None), "short": (_short, None)}
CASES = [(name, 5, 3, 0.7, k) for name in LAYOUTS for k in (1, 2, 3)] + \
        [(name, b, n, rho, 2) for name in ("ragged", "short") for b, n, rho in ((0, 2, 1.0),
                                                                                (1, 4, 0.7))]


def test_inputs_cover_the_steps(cwq):
    """Accepted replacements at s = 0, at the middle step and at the last."""
    assert SEED + BASE + 300 > 2147483647 and BASE != 0
    seen = set()
    for name in ("u32", "ragged", "short"):
        layout = LAYOUTS[name][0]
        table = _Fn(_greedy_table, layout, 5, 3, 0.7, SEED, BASE)
        want = _reference(layout, table, 5, 3, 1, 0.7, SEED, BASE)
        here = {s for st in want[4].values() for sweep in st for s in sweep}
        assert here, name  # every layout has a block that changes
        seen |= here
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("name,n_bits,n_steps,rho,sweeps", CASES)
def test_vs_reference(cwq, name, n_bits, n_steps, rho, sweeps):
    layout, d = LAYOUTS[name]
    table = _Fn(_greedy_table, layout, n_bits, n_steps, rho, SEED, BASE)
    got = _run(cwq, layout(), table(), n_bits, n_steps, sweeps, rho, d)
    want = _reference(layout, table, n_bits, n_steps, sweeps, rho, SEED, BASE)
    _same(got, want)
    _decodes(cwq, layout(), got, n_bits, n_steps, rho, d)
    idx = _i32(got[0])
    assert idx.min() >= 0 and idx.max() < (1 << n_bits)
    if n_bits == 0:
        assert not _i32(got[3]).any()
    empty = np.flatnonzero(np.diff(layout()[0]) == 0)
    assert (_u32(got[2])[empty] == 0).all() and not _i32(got[3])[empty].any()  # value +0


def test_monotone_per_block(cwq):
    layout, table = _uniform(32, 300), _greedy_table(_Fn(_uniform, 32, 300), 5, 3,
                                                      0.7, SEED, BASE)
    vals = [_run(cwq, layout, table, 5, 3, k, 0.7, 32)[2].cpu().numpy() for k in range(4)]
    for k in range(1, 4):
        assert (vals[k] >= vals[k - 1]).all(), k
    assert (vals[1] > vals[0]).any()
    ragged = _ragged()
    table = _greedy_table(_ragged, 5, 3, 0.7, SEED, BASE)
    vals = [_run(cwq, ragged, table, 5, 3, k, 0.7)[2].cpu().numpy() for k in (0, 1, 16)]
    assert (vals[1] >= vals[0]).all() and (vals[2] >= vals[1]).all()


# ---------------------------------------------------------------------------
# a lane per block: 16,384 blocks and more, none above 64 dims
# ---------------------------------------------------------------------------
def _many_short():
    return _layout(tuple(SHORT_LENGTHS) * 1000, 89)  # 17,000 blocks


@pytest.mark.parametrize("name", ["u8x16384", "u13x16384", "short_x1000"])
def test_lane_per_block_vs_reference(cwq, name):
    """The helper on sampled blocks; on all blocks the decoder rebuilds the
    sample, and the values never fall below the table's."""
    if name == "short_x1000":
        layout, d = _many_short, None
    else:
        d = int(name[1:].split("x")[0])
        layout = _Fn(_uniform, d, 16384)
    off = layout()[0]
    nb = len(off) - 1
    assert nb >= 16384 and np.diff(off).max() <= 64
    table = _Fn(_greedy_table, layout, 5, 3, 0.7, SEED, BASE)
    rng = np.random.Generator(np.random.PCG64(nb))
    blocks = tuple(sorted(set(rng.choice(nb, 40, replace=False).tolist() + [0, 8, nb - 1])))
    got = _run(cwq, layout(), table(), 5, 3, 2, 0.7, d)
    want = _reference(layout, table, 5, 3, 2, 0.7, SEED, BASE, blocks)
    assert sum(want[3][g] for g in blocks) > 0
    _same(got, want, blocks, off)
    _decodes(cwq, layout(), got, 5, 3, 0.7, d)
    start = _run(cwq, layout(), table(), 5, 3, 0, 0.7, d)
    assert (got[2] >= start[2]).all()


# ---------------------------------------------------------------------------
# every scoring path, the same bits in prune_mode 0, 1 and 2
# ---------------------------------------------------------------------------
def _path_shapes():
    d, bits, nb, _ = S.WS_UNIFORM_PRUNED
    yield "uniform_pruned", (d,) * nb, d, bits, 2, None
    yield "csr_lane", tuple(S.WS_CSR_LANE[0]), None, S.WS_CSR_LANE[1], S.WS_CSR_LANE[2], None
    yield "csr_all", tuple(S.WS_CSR_ALL[0]), None, S.WS_CSR_ALL[1], S.WS_CSR_ALL[2], (1, 5, 7)
    for kind in ("pipeline", "three_kernel"):
        sizes, bits, steps = S.WS_SMALL[kind]
        yield "small_" + kind, tuple(sizes), None, bits, steps, None
    yield "eval_ragged", tuple(S.WS_EVAL_RAGGED[0]), None, S.WS_EVAL_RAGGED[1], \
        S.WS_EVAL_RAGGED[2], None
    d, bits, nb, steps = S.WS_UNIFORM_GENERAL[0]
    yield "uniform_general", (d,) * nb, d, bits, steps, None


PATHS = {p[0]: p[1:] for p in _path_shapes()}


@pytest.mark.parametrize("name", list(PATHS))
def test_every_scoring_path_same_bits(cwq, name):
    lens, d, n_bits, n_steps, blocks = PATHS[name]
    assert n_steps >= 2
    layout = _Fn(_layout, lens, 555)
    off = layout()[0]
    table = _Fn(_greedy_table, layout, n_bits, n_steps, 1.0, SEED, BASE)
    want = _reference(layout, table, n_bits, n_steps, 2, 1.0, SEED, BASE, blocks)
    runs = [_run(cwq, layout(), table(), n_bits, n_steps, 2, 1.0, d, prune_mode=m)
            for m in (0, 1, 2)]
    for got in runs:
        _same(got, want, blocks if blocks else None, off)
        for x, y in zip(got, runs[0]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    _decodes(cwq, layout(), runs[2], n_bits, n_steps, 1.0, d)


# ---------------------------------------------------------------------------
# from a beam's table
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _beam_table():
    import compression_without_quantization_amd as C
    off, tl, ts, pl, ps = _short()
    idx, _ = C.encode_blocks_beam(tl, ts, pl, ps, 5, 3, SEED, 4, rho=0.7, block_off=off,
                                  block_id_base=BASE)
    return idx.cpu().numpy()


def test_from_a_beam(cwq):
    assert not np.array_equal(_beam_table(), _greedy_table(_short, 5, 3, 0.7, SEED, BASE))
    got = _run(cwq, _short(), _beam_table(), 5, 3, 2, 0.7)
    want = _reference(_short, _beam_table, 5, 3, 2, 0.7, SEED, BASE)
    _same(got, want)
    _decodes(cwq, _short(), got, 5, 3, 0.7)
    off, tl, ts, pl, ps = _short()
    both = cwq.encode_blocks_backfit(tl, ts, pl, ps, 5, 3, SEED, 2, beam=4, rho=0.7,
                                     block_off=off, block_id_base=BASE, return_value=True,
                                     return_accepted=True)
    for x, y in zip(both, got):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------------------
# adversarial blocks
# ---------------------------------------------------------------------------
ADV_LENS = (40, 33, 9, 300, 33, 64, 0, 20, 24, 17, 12, 0, 257)


@functools.lru_cache(maxsize=None)
def _adversarial():
    rng = np.random.Generator(np.random.PCG64(99))
    off = np.concatenate([[0], np.cumsum(ADV_LENS)]).astype(np.int64)
    tl, ts, pl, ps = _values(rng, int(off[-1]))
    tl[off[0] + 35] = np.nan           # a NaN mean: every candidate's value is NaN
    ps[off[1]:off[2]] = 0.0            # scale_s == 0: every candidate ties
    tl[off[2] + 8] = np.inf            # every candidate at -inf
    tl[off[7]:off[8]] = pl[off[7]:off[8]]  # posterior = prior
    ts[off[7]:off[8]] = ps[off[7]:off[8]]
    ts[off[8]:off[9]] = 1.0e6          # a flat target: near-ties everywhere
    ts[off[9]:off[10]] = 1.0e-6        # a tiny target scale: huge deficits
    ts[off[10]], ts[off[10] + 1], ts[off[10] + 2] = np.inf, 0.0, np.nan
    tl[off[12] + 250:off[12] + 257] = np.nan  # NaN means in the tail of a long block
    return off, tl, ts, pl, ps


@pytest.mark.parametrize("mode", [0, 2])
def test_adversarial(cwq, mode):
    table = _Fn(_greedy_table, _adversarial, 5, 3, 1.0, 42, 0)
    want = _reference(_adversarial, table, 5, 3, 2, 1.0, 42, 0)
    assert (want[0][:3] == 0).all() and not want[3][:3].any()  # all rows tie: nothing to accept
    assert want[3][3:].any() and not want[3][[6, 11]].any()
    off, tl, ts, pl, ps = _adversarial()
    got = cwq.backfit_blocks(table(), tl, ts, pl, ps, 5, 3, 42, 2, block_off=off,
                             return_value=True, return_accepted=True, prune_mode=mode)
    _same(got, want)
    _decodes(cwq, _adversarial(), got, 5, 3, 1.0, seed=42, base=0)


# ---------------------------------------------------------------------------
# workspace and output buffers: their contents on entry never matter
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0x00, 0xFF, "random", "guard"])
def test_poisoned_workspace_and_outputs(cwq, cwqlib, pattern):
    """The "guard" case: zeros between guard bands (tests/poison.py), which must stay intact."""
    guard = pattern == "guard"
    pattern = 0x00 if guard else pattern
    off = _ragged()[0]
    nb, D = len(off) - 1, int(off[-1])
    table = _Fn(_greedy_table, _ragged, 5, 3, 0.7, SEED, BASE)
    want = _reference(_ragged, table, 5, 3, 2, 0.7, SEED, BASE)  # a case of test_vs_reference
    tab = table()
    with poisoned(pattern, guard=guard) as f:
        got = _run(cwq, _ragged(), tab, 5, 3, 2, 0.7)
        torch.cuda.synchronize()
        assert f.assert_guards_intact("backfit") >= int(guard)
    f.assert_workspace(int(cwqlib.cwq_greedy_backfit_workspace_size(nb, D, 4095, 3)), "backfit")
    assert f.count("device", torch.float32, 4 * D) >= 1   # out_sample was poisoned too
    _same(got, want)
    lens, d, n_bits, n_steps, _ = PATHS["small_pipeline"]
    layout = _Fn(_layout, lens, 555)
    table_s = _Fn(_greedy_table, layout, n_bits, n_steps, 1.0, SEED, BASE)
    want_s = _reference(layout, table_s, n_bits, n_steps, 2, 1.0, SEED, BASE, None)
    tab = table_s()
    with poisoned(pattern, guard=guard) as f:
        got_s = _run(cwq, layout(), tab, n_bits, n_steps, 2, 1.0)
        torch.cuda.synchronize()
        assert f.assert_guards_intact("backfit, short blocks") >= int(guard)
    _same(got_s, want_s)


def test_back_to_back_on_one_workspace(cwq, cwqlib):
    """Two shapes in turn on one uncleared workspace, stream order only."""
    a, b = _ragged(), _short()
    ta = _greedy_table(_ragged, 5, 3, 0.7, SEED, BASE)
    tb = _beam_table()
    need = max(int(cwqlib.cwq_greedy_backfit_workspace_size(len(a[0]) - 1, int(a[0][-1]), 4095, 3)),
               int(cwqlib.cwq_greedy_backfit_workspace_size(len(b[0]) - 1, int(b[0][-1]), 64, 3)))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = _run(cwq, a, ta, 5, 3, 2, 0.7, workspace=ws)
        second = _run(cwq, b, tb, 5, 3, 2, 0.7, workspace=ws)
        again = _run(cwq, a, ta, 5, 3, 2, 0.7, workspace=ws)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    alone_a = _run(cwq, a, ta, 5, 3, 2, 0.7)
    alone_b = _run(cwq, b, tb, 5, 3, 2, 0.7)
    for got, want in ((first, alone_a), (second, alone_b), (again, alone_a)):
        for x, y in zip(got, want):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    _same(second, _reference(_short, _beam_table, 5, 3, 2, 0.7, SEED, BASE))


# ---------------------------------------------------------------------------
# the C call: argument errors, HIP graph
# ---------------------------------------------------------------------------
def _raw(cwqlib, t, n_bits, n_steps, sweeps, ws_bytes=None):
    """cwq_greedy_backfit on tensors made beforehand (t: dict); returns the code."""
    return cwqlib.cwq_greedy_backfit(
        t["tl"].data_ptr(), t["ts"].data_ptr(), t["pl"].data_ptr(), t["ps"].data_ptr(),
        t["off"].data_ptr(), t["nb"], t["D"], t["longest"], n_bits, n_steps, sweeps,
        R.wrap32(SEED), 0.7, BASE, t["idx"].data_ptr(), t["sample"].data_ptr(),
        t["value"].data_ptr(), t["acc"].data_ptr(), t["ws"].data_ptr(),
        t["ws"].numel() if ws_bytes is None else ws_bytes, None,
        torch.cuda.current_stream().cuda_stream)


def _tensors(cwqlib, layout, table, n_steps):
    off, tl, ts, pl, ps = layout
    dev = torch.device("cuda")
    nb, D = len(off) - 1, int(off[-1])
    longest = int(np.diff(off).max())
    f = lambda a: torch.from_numpy(a).to(dev)
    need = int(cwqlib.cwq_greedy_backfit_workspace_size(nb, D, longest, n_steps))
    return dict(tl=f(tl), ts=f(ts), pl=f(pl), ps=f(ps), off=f(off), nb=nb, D=D, longest=longest,
                idx=f(table.copy()), sample=torch.full((D,), -77.0, device=dev),
                value=torch.full((nb,), -77.0, device=dev),
                acc=torch.full((nb,), -77, dtype=torch.int32, device=dev), need=need,
                ws=torch.empty(need, dtype=torch.uint8, device=dev))


def test_argument_errors(cwq, cwqlib):
    table = _greedy_table(_short, 5, 3, 0.7, SEED, BASE)
    t = _tensors(cwqlib, _short(), table, 3)
    assert _raw(cwqlib, t, 5, 3, 1, ws_bytes=t["need"] - 1) == -3
    assert b"workspace" in cwqlib.cwq_last_error()
    for sweeps in (-1, 17):
        assert _raw(cwqlib, t, 5, 3, sweeps) == -1 and b"sweeps" in cwqlib.cwq_last_error()
    torch.cuda.synchronize()
    assert (t["sample"] == -77).all() and (t["acc"] == -77).all()  # nothing was launched
    assert np.array_equal(t["idx"].cpu().numpy(), table)
    assert _raw(cwqlib, t, 5, 3, 1) == 0
    torch.cuda.synchronize()
    assert (t["acc"] >= 0).all()
    off, tl, ts, pl, ps = _short()
    for bad in (-1, 32):
        spoiled = table.copy()
        spoiled[5, 1] = bad
        with pytest.raises(ValueError, match="outside"):
            cwq.backfit_blocks(spoiled, tl, ts, pl, ps, 5, 3, SEED, 1, block_off=off)
    with pytest.raises(cwq._lib.CwqError, match="sweeps"):
        cwq.backfit_blocks(table, tl, ts, pl, ps, 5, 3, SEED, 17, block_off=off)
    with pytest.raises(ValueError):
        cwq.backfit_blocks(table, tl, ts, pl, ps, 5, 3, SEED, 1)
    with pytest.raises(ValueError):
        cwq.backfit_blocks(table, tl, ts, pl, ps, 5, 3, SEED, 1, block_off=off, block_dim=4)
    with pytest.raises(ValueError, match="entries"):
        cwq.backfit_blocks(table[:-1], tl, ts, pl, ps, 5, 3, SEED, 1, block_off=off)


def test_graph_capture_and_replay(cwqlib):
    table = _greedy_table(_ragged, 5, 3, 0.7, SEED, BASE)
    t = _tensors(cwqlib, _ragged(), table, 3)
    start = t["idx"].clone()
    assert _raw(cwqlib, t, 5, 3, 2) == 0
    torch.cuda.synchronize()
    outs = (t["idx"], t["sample"], t["value"], t["acc"])
    want = [x.clone() for x in outs]
    t["idx"].copy_(start)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert _raw(cwqlib, t, 5, 3, 2) == 0
    for _ in range(2):
        for x in outs[1:]:
            x.fill_(-5)
        t["idx"].copy_(start)  # the table is refined in place: every replay starts from it
        t["ws"].fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        for got, w in zip(outs, want):
            assert torch.equal(got.view(torch.int32), w.view(torch.int32))
    ref = _reference(_ragged, _Fn(_greedy_table, _ragged, 5, 3, 0.7, SEED, BASE),
                     5, 3, 2, 0.7, SEED, BASE)
    _same(outs, ref)


# ---------------------------------------------------------------------------
# the grouped wrapper and the PLN codec
# ---------------------------------------------------------------------------
def test_grouped_wrapper(cwq, oracle):
    from test_beam_gpu import _latent
    ql, qs, pl, ps = _latent()
    n_steps, n_bits, seed = 2, 6, 11
    tl, ts = oracle.standardise(ql, qs, pl, ps)
    kl = oracle.kl_normal_normal(ql, qs, pl, ps)
    starts = oracle.group_starts(kl, n_bits * n_steps, cwq.group_size_threshold(12))
    target, proposal = cwq.Normal(ql, qs), cwq.Normal(pl, ps)
    # no sweep: the greedy wrapper's triple
    s0, c0, g0 = cwq.code_grouped_greedy_sample_backfit(target, proposal, n_steps, n_bits, seed, 0)
    ws, wc, wg = cwq.code_grouped_greedy_sample(None, target, proposal, n_steps, n_bits, seed)
    assert np.array_equal(_u32(s0), _u32(ws)) and c0 == wc and list(g0) == list(wg)
    # two sweeps: the oracle's pipeline around the restatement
    s2, c2, g2 = cwq.code_grouped_greedy_sample_backfit(target, proposal, n_steps, n_bits, seed, 2)
    assert list(g2) == list(starts)
    D = ql.size
    zeros, ones = np.zeros(D, np.float32), np.ones(D, np.float32)
    gidx, _ = oracle.greedy_encode(tl, ts, zeros, ones, starts, n_bits, n_steps, seed, 1.0, 0)
    idx, samp, _, accepted, _ = B.backfit(oracle, gidx, tl, ts, zeros, ones, starts, n_bits,
                                          n_steps, seed, 2, 1.0, 0)
    assert accepted.sum() > 0
    assert c2 == cwq.indices_to_bitcode(idx, n_bits)
    assert np.array_equal(_u32(s2), _u32(oracle.destandardise(samp, pl, ps)))
    assert c2 != c0 and len(c2) == len(c0)  # the same bits spent, other rows
    back = cwq.decode_grouped_greedy_sample(None, c2, g2[:-1], proposal, n_bits, n_steps, seed)
    assert np.array_equal(_u32(back), _u32(s2))
    # after a beam: still decodable
    s4, c4, g4 = cwq.code_grouped_greedy_sample_backfit(target, proposal, n_steps, n_bits, seed, 1,
                                                        beam=4)
    back = cwq.decode_grouped_greedy_sample(None, c4, g4[:-1], proposal, n_bits, n_steps, seed)
    assert np.array_equal(_u32(back), _u32(s4)) and len(c4) == len(c0)


def test_pln_backfit_sweeps(cwq, oracle, tmp_path):
    """test_pln_gpu.py's smallest image and settings: backfit_sweeps=2 writes a
    file of the plain call's size that decode_image_greedy reads back to the
    encoder's latents; backfit_sweeps=0 gives the plain call's bytes."""
    import test_pln_gpu as T
    P = cwq.pln
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    model = T._model(P, seed=4)
    img = T._image(64, 64, seed=5)
    plain, zero, two, mixed = (str(tmp_path / n) for n in ("plain.miracle", "zero.miracle",
                                                            "two.miracle", "mixed.miracle"))
    (p2, p1), _ = model.code_image_greedy(None, img, 3, comp_file_path=plain, **T.KW)
    (z2, z1), _ = model.code_image_greedy(None, img, 3, comp_file_path=zero, backfit_sweeps=0,
                                          backfitting_steps_level_1=5, **T.KW)
    (f2, f1), _ = model.code_image_greedy(None, img, 3, comp_file_path=two, backfit_sweeps=2,
                                          **T.KW)
    model.code_image_greedy(None, img, 3, comp_file_path=mixed, backfit_sweeps=1, beam_width=2,
                            **T.KW)
    assert open(zero, "rb").read() == open(plain, "rb").read()
    T._eq(z1, p1, "level-1 sample, backfit_sweeps=0")
    T._eq(f2, p2, "level-2 sample")
    assert len(open(two, "rb").read()) == len(open(plain, "rb").read())
    assert len(open(mixed, "rb").read()) == len(open(plain, "rb").read())
    rec = model.decode_image_greedy(None, two, use_importance_sampling=False,
                                    greedy_max_group_size_bits=12,
                                    first_level_max_group_size_bits=4,
                                    second_level_max_group_size_bits=2)
    shape1 = tuple(model.latent_distributions(img, 3)["q1"].loc.shape)
    perm1, _ = oracle.pln_permutations(3, int(np.prod(shape1)), 1)
    z1 = P.unpermute_unflatten(torch.from_numpy(np.asarray(f1, np.float32)).cuda(),
                               torch.from_numpy(perm1).cuda(), shape1)
    with torch.no_grad():
        want = model.synthesis_transform_1(z1)[0].permute(1, 2, 0).cpu().numpy()
    T._eq(rec, want, "reconstruction from the backfitted file")
    for kw in (dict(use_importance_sampling=True), dict(first_level_group_bits=True)):
        with pytest.raises(ValueError, match="backfit_sweeps"):
            model.code_image_greedy(None, img, 3, backfit_sweeps=2, **{**T.KW, **kw})
