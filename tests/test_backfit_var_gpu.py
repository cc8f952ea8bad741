"""GPU: backfitting under per-block bit budgets (cwq_greedy_backfit_var, DESIGN.md
4h) against tests/backfit_reference.py called per budget with the rows of that
budget.  Every comparison is bit for bit: int32 indices and counts, uint32
views of samples and values; no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import backfit_reference as B
import beam_reference as R
import encode_shapes as S
from poison import poisoned

pytestmark = pytest.mark.gpu

SEED = 2147483647 - 5  # seed + base + g wraps past 2^31 - 1 inside every call below
BASE = 3               # block_id_base
ADV_LENS = (40, 33, 9, 300, 33, 64, 0, 20, 24, 17, 12, 0, 257)
SHORT_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 0, 15, 16, 17, 31, 33, 40, 63, 64)


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


@functools.lru_cache(maxsize=None)
def _layout(lens, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return (off,) + _values(rng, int(off[-1]))


def _cycle(nb, budgets):
    return tuple(budgets[g % len(budgets)] for g in range(nb))


def _rows18_bits():
    cyc = (0, 3, 6, 12)
    return tuple(5 if d >= 496 else 8 if 247 <= d <= 257 else cyc[i % 4]
                 for i, d in enumerate(S.ROWS_WAVE_LENGTHS))


# name -> (block lengths, layout seed, uniform d or None, budgets, n_steps, rho)
INPUTS = {
    "adv39": (ADV_LENS * 3, 21, None, _cycle(39, (0, 3, 6, 8, 12, 1)), 3, 0.7),
    "rows18": (tuple(S.ROWS_WAVE_LENGTHS), 1717, None, _rows18_bits(), 3, 0.7),
    "u32x60": ((32,) * 60, 23, 32, _cycle(60, (0, 3, 6, 8, 12, 1)), 3, 0.7),
    "u13x60": ((13,) * 60, 24, 13, _cycle(60, (0, 3, 6, 8, 12, 1)), 2, 1.0),
    "short17000": (SHORT_LENGTHS * 1000, 89, None, _cycle(17000, (0, 3, 6, 8, 1)), 3, 0.7),
}


def _input(name):
    lens, seed, d, bits, n_steps, rho = INPUTS[name]
    return _layout(lens, seed), d, np.asarray(bits, np.int32), n_steps, rho


def _kw(layout, d):
    return dict(block_dim=d) if d else dict(block_off=layout[0])


@functools.lru_cache(maxsize=None)
def _greedy_table(name, bits=None):
    """encode_blocks_var's table for the input (a host copy), once per case."""
    import compression_without_quantization_amd as C
    layout, d, b, n_steps, rho = _input(name)
    off, tl, ts, pl, ps = layout
    idx, _ = C.encode_blocks_var(tl, ts, pl, ps, b if bits is None else np.asarray(bits, np.int32),
                                 n_steps, SEED, rho=rho, block_id_base=BASE, **_kw(layout, d))
    return idx.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _oracle_table(name):
    """The greedy table per budget from the oracle's greedy coder."""
    from oracle import oracle as O
    O.build()
    layout, d, bits, n_steps, rho = _input(name)
    off, tl, ts, pl, ps = layout
    out = np.zeros((len(bits), n_steps), np.int32)
    for g, b in enumerate(bits):
        sl = slice(int(off[g]), int(off[g + 1]))
        idx, _ = O.greedy_encode(tl[sl], ts[sl], pl[sl], ps[sl], [0, sl.stop - sl.start], int(b),
                                 n_steps, R.wrap32(SEED), rho, BASE + g)
        out[g] = np.asarray(idx).reshape(-1)
    return out


class _Tab:
    """A hashable function returning a host table (a key for _reference)."""

    def __init__(self, f, *args):
        self.key = (f, args)

    def __call__(self):
        return self.key[0](*self.key[1])

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return isinstance(other, _Tab) and self.key == other.key


@functools.lru_cache(maxsize=None)
def _reference(name, table, sweeps, blocks=None, bits=None):
    """The restatement per budget with blocks= the rows of that budget: (idx,
    sample bits, values [nb, sweeps + 1], accepted, steps), once per case."""
    from oracle import oracle as O
    O.build()
    layout, d, b, n_steps, rho = _input(name)
    b = b if bits is None else np.asarray(bits, np.int32)
    off, tl, ts, pl, ps = layout
    nb = len(off) - 1
    tab = table()
    idx = np.zeros((nb, n_steps), np.int32)
    sample = np.zeros(tl.size, np.float32)
    values = np.zeros((nb, sweeps + 1), np.float32)
    accepted = np.zeros(nb, np.int32)
    steps = {}
    for budget in sorted(set(b.tolist())):
        rows = [g for g in (range(nb) if blocks is None else blocks) if b[g] == budget]
        if not rows:
            continue
        i, s, v, a, st = B.backfit(O, tab, tl, ts, pl, ps, off, budget, n_steps, SEED, sweeps, rho,
                                   BASE, rows)
        for g in rows:
            sl = slice(int(off[g]), int(off[g + 1]))
            idx[g], sample[sl], values[g], accepted[g] = i[g], s[sl], v[g], a[g]
        steps.update(st)
    return idx, _u32(sample), values, accepted, steps


def _same(got, want, blocks=None, off=None, column=-1):
    gi, gs, gv, ga = _i32(got[0]), _u32(got[1]), _u32(got[2]), _i32(got[3])
    wv = _u32(want[2][:, column])
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


def _bitwise_equal(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def _run(cwq, name, table, sweeps, bits=None, **kw):
    layout, d, b, n_steps, rho = _input(name)
    off, tl, ts, pl, ps = layout
    return cwq.backfit_blocks_var(table, tl, ts, pl, ps, b if bits is None else bits, n_steps,
                                  SEED, sweeps, rho=rho, block_id_base=BASE, return_value=True,
                                  return_accepted=True, **_kw(layout, d), **kw)


def _decodes(cwq, name, got, bits=None):
    """decode_blocks_var from the indices and from their packed stream."""
    layout, d, b, n_steps, rho = _input(name)
    b = b if bits is None else bits
    off, tl, ts, pl, ps = layout
    kw = dict(rho=rho, block_id_base=BASE, **_kw(layout, d))
    back = cwq.decode_blocks_var(got[0], b, pl, ps, n_steps, SEED, **kw)
    assert np.array_equal(_u32(back), _u32(got[1]))
    code, total = cwq.pack_indices(got[0], b)
    assert total == int(np.asarray(b, np.int64).sum()) * n_steps
    back = cwq.decode_blocks_var(code, b, pl, ps, n_steps, SEED, **kw)
    assert np.array_equal(_u32(back), _u32(got[1]))
    idx = _i32(got[0])
    assert (idx >= 0).all() and (idx < (1 << np.asarray(b, np.int64))[:, None]).all()


def _accepting_buckets(name, want, bits=None):
    b = _input(name)[2] if bits is None else np.asarray(bits)
    return {int(v): int((want[3][b == v] > 0).sum()) for v in sorted(set(b.tolist()))}


def _check_reference_accepts(name, want):
    """What the reference accepts in 2 sweeps on each input: no comparison
    below is vacuous."""
    per = _accepting_buckets(name, want)
    assert per.get(0, 0) == 0
    if name in ("adv39", "u32x60"):
        assert all(per[b] > 0 for b in (1, 3, 6, 8, 12)), per
    if name == "adv39":
        seen = {s for st in want[4].values() for sweep in st for s in sweep}
        assert seen == {0, 1, 2}
    if name == "rows18":
        assert per[5] >= 1 and per[8] == 4, per
    if name == "u13x60":
        assert per[3] > 0 and per[6] > 0, per


# ---------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adv39", "rows18", "u32x60", "u13x60"])
def test_vs_restatement(cwq, name):
    table = _Tab(_greedy_table, name)
    assert np.array_equal(table(), _oracle_table(name))
    _check_reference_accepts(name, _reference(name, table, 2))
    for sweeps in (1, 2):
        got = _run(cwq, name, table(), sweeps)
        _same(got, _reference(name, table, sweeps))
        _decodes(cwq, name, got)
    layout, bits = _input(name)[0], _input(name)[2]
    quiet = np.flatnonzero((bits == 0) | (np.diff(layout[0]) == 0))
    assert not _i32(got[3])[quiet].any()
    assert np.array_equal(_i32(got[0])[quiet], table()[quiet])


# ---------------------------------------------------------------------------
# 2. every budget equal: cwq_greedy_backfit at that budget
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adv39", "u32x60"])
@pytest.mark.parametrize("b", [5, 12])
def test_every_budget_equal(cwq, name, b):
    layout, d, _, n_steps, rho = _input(name)
    off, tl, ts, pl, ps = layout
    nb = len(off) - 1
    bits = np.full(nb, b, np.int32)
    kw = dict(rho=rho, block_id_base=BASE, **_kw(layout, d))
    idx, sample = cwq.encode_blocks(tl, ts, pl, ps, b, n_steps, SEED, **kw)
    vidx, vsample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, n_steps, SEED, **kw)
    _bitwise_equal((vidx, vsample), (idx, sample))
    for sweeps in (0, 2):
        one = cwq.backfit_blocks(idx, tl, ts, pl, ps, b, n_steps, SEED, sweeps, return_value=True,
                                 return_accepted=True, **kw)
        got = _run(cwq, name, idx, sweeps, bits=bits)
        _bitwise_equal(got, one)
        if sweeps:
            assert _i32(got[3]).any()
    both = cwq.encode_blocks_var_backfit(tl, ts, pl, ps, bits, n_steps, SEED, 0, **kw)
    _bitwise_equal(both, (vidx, vsample))
    mixed = _input(name)[2]
    both = cwq.encode_blocks_var_backfit(tl, ts, pl, ps, mixed, n_steps, SEED, 0, **kw)
    _bitwise_equal(both, cwq.encode_blocks_var(tl, ts, pl, ps, mixed, n_steps, SEED, **kw))


# ---------------------------------------------------------------------------
# 3. no block ever falls
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_table(name):
    bits, n_steps = _input(name)[2], _input(name)[3]
    rng = np.random.Generator(np.random.PCG64(4242))
    return (rng.integers(0, 1 << 30, (len(bits), n_steps)) % (1 << bits.astype(np.int64))[:, None]) \
        .astype(np.int32)


@pytest.mark.parametrize("start", ["greedy", "random"])
def test_monotone_per_block(cwq, start):
    table = _Tab(_greedy_table, "adv39") if start == "greedy" else _Tab(_random_table, "adv39")
    runs = [_run(cwq, "adv39", table(), k) for k in range(4)]
    vals = [r[2].cpu().numpy() for r in runs]
    for k in range(1, 4):
        assert (vals[k] >= vals[k - 1]).all(), k
    assert (vals[1] > vals[0]).any()
    assert np.array_equal(_i32(runs[0][0]), table()) and not _i32(runs[0][3]).any()
    if start == "random":
        want = _reference("adv39", table, 3)
        for k in range(4):
            assert np.array_equal(_u32(vals[k]), _u32(want[2][:, k])), k
        _same(runs[3], want)
        _decodes(cwq, "adv39", runs[3])


# ---------------------------------------------------------------------------
# 4. the same bits in prune_mode 0, 1 and 2
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adv39", "rows18"])
def test_prune_modes_same_bits(cwq, name):
    table = _Tab(_greedy_table, name)
    want = _reference(name, table, 2)
    for mode in (0, 1, 2):
        _same(_run(cwq, name, table(), 2, prune_mode=mode), want)


# ---------------------------------------------------------------------------
# 5. a lane per block: 17,000 blocks, none above 64 dims
# ---------------------------------------------------------------------------
def test_lane_per_block(cwq):
    name = "short17000"
    layout, _, bits, n_steps, _ = _input(name)
    off = layout[0]
    nb = len(off) - 1
    assert nb >= 16384 and np.diff(off).max() <= 64
    table = _Tab(_greedy_table, name)
    rng = np.random.Generator(np.random.PCG64(nb))
    blocks = tuple(sorted(set(rng.choice(nb, 40, replace=False).tolist() + [0, nb - 1])))
    got = _run(cwq, name, table(), 2)
    want = _reference(name, table, 2, blocks)
    assert sum(want[3][g] for g in blocks) > 0
    _same(got, want, blocks, off)
    _decodes(cwq, name, got)
    start = _run(cwq, name, table(), 0)
    assert (got[2] >= start[2]).all() and (got[2] > start[2]).any()
    assert np.array_equal(_i32(start[0]), table())


# ---------------------------------------------------------------------------
# 6. workspace and output buffers: their contents on entry never matter
# ---------------------------------------------------------------------------
def _need(cwq, name):
    layout, d, _, n_steps, _ = _input(name)
    off = layout[0]
    return cwq.backfit.backfit_var_workspace_bytes(len(off) - 1, int(off[-1]),
                                                   int(np.diff(off).max()), n_steps,
                                                   uniform=d is not None)


@pytest.mark.parametrize("pattern", [0x00, 0xFF, "random", "guard"])
def test_poisoned_workspace_and_outputs(cwq, pattern):
    """The "guard" case: zeros between guard bands (tests/poison.py), which must stay intact."""
    guard = pattern == "guard"
    pattern = 0x00 if guard else pattern
    for name in ("adv39", "u13x60"):
        table = _Tab(_greedy_table, name)
        want = _reference(name, table, 2)  # a case of test_vs_restatement
        tab = table()
        D = int(_input(name)[0][0][-1])
        with poisoned(pattern, guard=guard) as f:
            got = _run(cwq, name, tab, 2)
            torch.cuda.synchronize()
            assert f.assert_guards_intact(name) >= int(guard)
        f.assert_workspace(_need(cwq, name), name)
        assert f.count("device", torch.float32, 4 * D) >= 1   # out_sample was poisoned too
        _same(got, want)


def test_back_to_back_on_one_workspace(cwq):
    """Two budget vectors in turn on one uncleared workspace, stream order only."""
    name = "adv39"
    bits_a = _input(name)[2]
    bits_b = np.roll(bits_a, 1)
    ta, tb = _greedy_table(name), _greedy_table(name, tuple(bits_b.tolist()))
    ws = torch.empty(_need(cwq, name), dtype=torch.uint8, device="cuda")
    first = _run(cwq, name, ta, 2, workspace=ws)
    second = _run(cwq, name, tb, 2, bits=bits_b, workspace=ws)
    again = _run(cwq, name, ta, 2, workspace=ws)
    alone_a = _run(cwq, name, ta, 2)
    alone_b = _run(cwq, name, tb, 2, bits=bits_b)
    for got, want in ((first, alone_a), (second, alone_b), (again, alone_a)):
        _bitwise_equal(got, want)
    _same(first, _reference(name, _Tab(_greedy_table, name), 2))
    _same(second, _reference(name, _Tab(_greedy_table, name, tuple(bits_b.tolist())), 2,
                             None, tuple(bits_b.tolist())))


# ---------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------
def _tensors(cwq, name, table, bits=None):
    layout, d, b, n_steps, _ = _input(name)
    off, tl, ts, pl, ps = layout
    dev = torch.device("cuda")
    nb, D = len(off) - 1, int(off[-1])
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    need = _need(cwq, name)
    return dict(tl=f(tl), ts=f(ts), pl=f(pl), ps=f(ps), off=None if d else f(off), nb=nb, D=D,
                longest=int(np.diff(off).max()), bits=f(b if bits is None else bits),
                n_steps=n_steps, idx=f(table.copy()), sample=torch.full((D,), -77.0, device=dev),
                value=torch.full((nb,), -77.0, device=dev),
                acc=torch.full((nb,), -77, dtype=torch.int32, device=dev), need=need,
                ws=torch.empty(need, dtype=torch.uint8, device=dev))


def _raw(cwqlib, t, sweeps, ws_bytes=None):
    return cwqlib.cwq_greedy_backfit_var(
        t["tl"].data_ptr(), t["ts"].data_ptr(), t["pl"].data_ptr(), t["ps"].data_ptr(),
        t["off"].data_ptr() if t["off"] is not None else None, t["nb"], t["D"], t["longest"],
        t["bits"].data_ptr(), t["n_steps"], sweeps, R.wrap32(SEED), 0.7, BASE,
        t["idx"].data_ptr(), t["sample"].data_ptr(), t["value"].data_ptr(), t["acc"].data_ptr(),
        t["ws"].data_ptr(), t["ws"].numel() if ws_bytes is None else ws_bytes, None,
        torch.cuda.current_stream().cuda_stream)


def _untouched(t, table):
    torch.cuda.synchronize()
    assert (t["sample"] == -77).all() and (t["value"] == -77).all() and (t["acc"] == -77).all()
    assert np.array_equal(t["idx"].cpu().numpy(), table)


@pytest.mark.parametrize("name", ["adv39", "u32x60"])
def test_refusals_leave_the_callers_arrays(cwq, cwqlib, name):
    bits = _input(name)[2]
    table = _greedy_table(name)
    # one entry equal to 2^n_bits[g] in a 3-bit block, far below the call's largest count
    g = int(np.flatnonzero((bits == 3) & (np.diff(_input(name)[0][0]) > 0))[0])
    spoiled = table.copy()
    spoiled[g, 1] = 8
    t = _tensors(cwq, name, spoiled)
    assert _raw(cwqlib, t, 1) == -1
    msg = cwqlib.cwq_last_error()
    assert msg.startswith(b"1 of ") and b"idx_inout" in msg, msg
    _untouched(t, spoiled)
    spoiled[g, 1] = -1
    spoiled[g + 6, 0] = 1 << 20
    t = _tensors(cwq, name, spoiled)
    assert _raw(cwqlib, t, 1) == -1 and cwqlib.cwq_last_error().startswith(b"2 of ")
    _untouched(t, spoiled)
    # a budget of 31
    wide = bits.copy()
    wide[5] = 31
    t = _tensors(cwq, name, table, wide)
    assert _raw(cwqlib, t, 1) == -1 and b"n_bits" in cwqlib.cwq_last_error()
    _untouched(t, table)
    # ragged blocks: what only the buckets' facts can tell.  The real arrays at
    # full length (every read stays inside them), one scalar or one offset wrong
    if _input(name)[1] is None:
        off = _input(name)[0][0]
        lowered = off.copy()
        lowered[2] = off[1] - 1  # block 1 ends before it starts; block 2 is longer by as much
        D, longest = int(off[-1]), int(np.diff(off).max())
        assert 0 <= lowered[2] < lowered[1] and lowered.max() == D
        for change, msg in [
                (dict(D=D - 1), b"the blocks hold %d dims, total_dims=%d" % (D, D - 1)),
                (dict(longest=longest - 1),
                 b"a block holds %d dims, max_block_dim=%d" % (longest, longest - 1)),
                (dict(off=torch.from_numpy(lowered).cuda()), b"block_off decreases at 1 blocks")]:
            t = _tensors(cwq, name, table)
            t.update(change)
            assert _raw(cwqlib, t, 1) == -1 and cwqlib.cwq_last_error() == msg, \
                cwqlib.cwq_last_error()
            _untouched(t, table)
    # a workspace one byte short
    t = _tensors(cwq, name, table)
    assert _raw(cwqlib, t, 1, ws_bytes=t["need"] - 1) == -3
    assert b"workspace" in cwqlib.cwq_last_error()
    _untouched(t, table)
    assert _raw(cwqlib, t, 1) == 0
    torch.cuda.synchronize()
    assert (t["acc"] >= 0).all()
    _bitwise_equal((t["idx"], t["sample"], t["value"], t["acc"]), _run(cwq, name, table, 1))


def test_python_argument_errors(cwq):
    name = "adv39"
    layout, _, bits, n_steps, _ = _input(name)
    off, tl, ts, pl, ps = layout
    table = _greedy_table(name)
    spoiled = table.copy()
    spoiled[1, 1] = 8  # block 1: 3 bits
    with pytest.raises(cwq._lib.CwqError, match="1 of .*idx_inout"):
        cwq.backfit_blocks_var(spoiled, tl, ts, pl, ps, bits, n_steps, SEED, 1, block_off=off)
    assert spoiled[1, 1] == 8
    wide = bits.copy()
    wide[0] = 31
    with pytest.raises(cwq._lib.CwqError, match="n_bits"):
        cwq.backfit_blocks_var(table, tl, ts, pl, ps, wide, n_steps, SEED, 1, block_off=off)
    with pytest.raises(cwq._lib.CwqError, match="sweeps"):
        cwq.backfit_blocks_var(table, tl, ts, pl, ps, bits, n_steps, SEED, 17, block_off=off)
    with pytest.raises(ValueError):
        cwq.backfit_blocks_var(table, tl, ts, pl, ps, bits, n_steps, SEED, 1)
    with pytest.raises(ValueError):
        cwq.backfit_blocks_var(table, tl, ts, pl, ps, bits, n_steps, SEED, 1, block_off=off,
                               block_dim=4)
    with pytest.raises(ValueError, match="entries"):
        cwq.backfit_blocks_var(table[:-1], tl, ts, pl, ps, bits, n_steps, SEED, 1, block_off=off)
    with pytest.raises(ValueError, match="counts"):
        cwq.backfit_blocks_var(table, tl, ts, pl, ps, bits[:-1], n_steps, SEED, 1, block_off=off)


# ---------------------------------------------------------------------------
# 8. degenerate calls: returned as given
# ---------------------------------------------------------------------------
def test_degenerate_calls(cwq):
    e = np.zeros(0, np.float32)
    for kw in (dict(block_off=[0]), dict(block_dim=8)):
        got = cwq.backfit_blocks_var(np.zeros((0, 3), np.int32), e, e, e, e, [], 3, SEED, 2,
                                     return_value=True, return_accepted=True, **kw)
        assert [x.numel() for x in got] == [0, 0, 0, 0]
    # empty blocks only
    table = np.zeros((4, 3), np.int32)
    table[1] = (1, 0, 3)
    got = cwq.backfit_blocks_var(table, e, e, e, e, [5, 2, 0, 3], 3, SEED, 2, block_off=[0] * 5,
                                 return_value=True, return_accepted=True)
    assert np.array_equal(_i32(got[0]), table) and got[1].numel() == 0
    assert not _u32(got[2]).any() and not _i32(got[3]).any()
    # all budgets 0; one step
    for name in ("adv39", "u13x60"):
        layout, d, bits, n_steps, rho = _input(name)
        off, tl, ts, pl, ps = layout
        nb = len(off) - 1
        kw = dict(rho=rho, block_id_base=BASE, **_kw(layout, d))
        zero = np.zeros(nb, np.int32)
        idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, zero, n_steps, SEED, **kw)
        got = cwq.backfit_blocks_var(idx, tl, ts, pl, ps, zero, n_steps, SEED, 3,
                                     return_value=True, return_accepted=True, **kw)
        assert not _i32(got[0]).any() and not _i32(got[3]).any()
        assert np.array_equal(_u32(got[1]), _u32(sample))
        idx, sample = cwq.encode_blocks_var(tl, ts, pl, ps, bits, 1, SEED, **kw)
        got = cwq.backfit_blocks_var(idx, tl, ts, pl, ps, bits, 1, SEED, 3, return_value=True,
                                     return_accepted=True, **kw)
        assert torch.equal(got[0], idx) and not _i32(got[3]).any()
        assert np.array_equal(_u32(got[1]), _u32(sample))


# ---------------------------------------------------------------------------
# 9. the grouped wrapper
# ---------------------------------------------------------------------------
def _latent():
    """2,000 dims: a quiet half (long groups, low budgets) and a loud half."""
    rng = np.random.Generator(np.random.PCG64(7))
    D = 2000
    pl = rng.standard_normal(D).astype(np.float32)
    ps = rng.uniform(0.5, 2.0, D).astype(np.float32)
    delta = np.where(np.arange(D) < 1000, 0.1, rng.uniform(0.5, 1.5, D))
    delta[[100, 1200, 1201, 1800]] = 4.0
    ql = (pl + delta * ps * rng.choice([-1.0, 1.0], D)).astype(np.float32)
    qs = (ps * np.where(np.arange(D) < 1000, 1.0, rng.uniform(0.4, 0.9, D))).astype(np.float32)
    return ql, qs, pl, ps


def test_grouped_wrapper(cwq, oracle):
    ql, qs, pl, ps = _latent()
    n_steps, n_bits, seed = 3, 6, 11
    target, proposal = cwq.Normal(ql, qs), cwq.Normal(pl, ps)
    plain = cwq.code_grouped_greedy_sample_var(target, proposal, n_steps, n_bits, seed)
    zero = cwq.code_grouped_greedy_sample_var_backfit(target, proposal, n_steps, n_bits, seed, 0)
    assert np.array_equal(_u32(zero[0]), _u32(plain[0])) and zero[1] == plain[1]
    assert zero[2] == plain[2] and list(zero[3]) == list(plain[3])
    assert np.array_equal(zero[4], plain[4])
    two = cwq.code_grouped_greedy_sample_var_backfit(target, proposal, n_steps, n_bits, seed, 2)
    assert two[2] == plain[2] and list(two[3]) == list(plain[3])
    assert np.array_equal(two[4], plain[4]) and len(two[1]) == len(plain[1])
    assert len(set(np.asarray(two[4]).tolist())) > 2  # budgets differ between groups
    back = cwq.decode_grouped_greedy_sample_var(two[1], two[3], two[4], proposal, n_steps, seed)
    assert np.array_equal(_u32(back), _u32(two[0]))
    # each group's log-density in the coder's arithmetic, from the decoded
    # standardised samples
    tl, ts = oracle.standardise(ql, qs, pl, ps)
    starts = np.asarray(two[3], np.int64)
    zeros, ones = np.zeros(ql.size, np.float32), np.ones(ql.size, np.float32)
    cn = R.lognorms(oracle, ts)

    def values(code):
        x = cwq.decode_blocks_var(np.frombuffer(code, np.uint8), two[4], zeros, ones, n_steps,
                                  seed, block_off=starts).cpu().numpy()
        with np.errstate(all="ignore"):
            z = (x - tl) / ts
            lp = (np.float32(-0.5) * (z * z)) - cn
        return np.array([R.keyed_values(R.eigen_rowsums(lp[None, a:b]))[0]
                         for a, b in zip(starts[:-1], starts[1:])], np.float32)

    v0, v2 = values(plain[1]), values(two[1])
    assert (v2 >= v0).all() and (v2 > v0).any()
