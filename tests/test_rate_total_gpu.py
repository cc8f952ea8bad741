"""GPU: budgets under a bit total solved on the device (cwq_choose_bits_total,
cwq_greedy_encode_rate).

The device solver is defined as equal to ratetable.choose_bits_total, the host's
60-step loop: every comparison here is bit for bit (int32 bits and indices, the
price as a float64 bit pattern, uint32 views of samples); no tolerance anywhere.
Crafted tables are held both to choose_bits_total on the same device table and
to its NumPy restatement (tests/rate_solve_reference.py).  The row counts are
the smallest that cross each boundary of the sweeps: one row, a wave's tile of
64 rows and one either side of it, several workgroups, and more rows than the
grid has lanes."""
import functools

import numpy as np
import pytest
import torch

import rate_reference as RR
import rate_solve_reference as SR
from graph_replay import PATTERNS, fill

pytestmark = pytest.mark.gpu

NB = (1, 63, 64, 65, 257, 4097)
SEED = 2147483647 - 3


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    return C


def _u32(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _assert_solved(got, want_bits, want_lam, what, target=None):
    """got: choose_bits_total_device's triple."""
    bits, lam, total = (_np(t) for t in got)
    want_bits = np.asarray(want_bits)
    bad = np.flatnonzero(bits != want_bits)
    assert bad.size == 0, f"{what}: {bad.size} budgets differ, first blocks {bad[:4].tolist()}: " \
                          f"got {bits[bad[:4]].tolist()}, want {want_bits[bad[:4]].tolist()}"
    assert SR.lam_bits(lam[0]) == SR.lam_bits(want_lam), f"{what}: lam {lam[0]!r}, want {want_lam!r}"
    assert int(total[0]) == int(want_bits.sum(dtype=np.int64)), what
    if target is not None:
        assert int(total[0]) <= target, what


# ---- the solver on crafted tables ---------------------------------------------------
@pytest.mark.parametrize("B", SR.BITS)
@pytest.mark.parametrize("nb", NB)
def test_solver_equals_the_host_loop_and_numpy(cwq, nb, B):
    v = SR.crafted_table(nb, B)
    dv = torch.from_numpy(v).cuda()
    n = 0
    for lo, hi in SR.ranges(B):
        for T in SR.targets(v, lo, hi):
            what = f"nb={nb} B={B} range=({lo}, {hi}) T={T}"
            wb, wl, _ = SR.choose_bits_total(v, T, lo, hi)
            hb, hl = cwq.choose_bits_total(dv, T, min_bits=lo, max_bits=hi)
            assert np.array_equal(_np(hb), wb) and SR.lam_bits(hl) == SR.lam_bits(wl), \
                f"{what}: the host loop against NumPy"
            got = cwq.choose_bits_total_device(dv, T, min_bits=lo, max_bits=hi)
            _assert_solved(got, wb, wl, what, T)
            n += 1
    assert n > 0


def test_a_target_met_exactly(cwq):
    """A walk with ``<`` in place of ``<=`` ends elsewhere on these."""
    v = SR.crafted_table(65, 8)
    dv = torch.from_numpy(v).cuda()
    met = 0
    for T in SR.targets(v, 0, 8):
        wb, wl, wt = SR.choose_bits_total(v, T, 0, 8)
        if wt == T and T > 0 and wl > 0.0:
            _, strict_lam, _ = SR.choose_bits_total(v, T, 0, 8, strict=True)
            assert strict_lam > wl
            _assert_solved(cwq.choose_bits_total_device(dv, T), wb, wl, f"T={T}", T)
            met += 1
    assert met > 0


def test_more_blocks_than_the_sweeps_have_lanes(cwq):
    """2^20 + 65 rows at B = 2 (12.6 MB): every lane strides over several tiles
    and the last tile is short.  Held to choose_bits_total alone (the NumPy
    loop is left out for time)."""
    nb, B = (1 << 20) + 65, 2
    g = torch.Generator(device="cuda").manual_seed(7)
    base = -30.0 * torch.rand((nb, 1), device="cuda", generator=g)
    gain = torch.cumsum(3.0 * torch.rand((nb, B + 1), device="cuda", generator=g), dim=1)
    dv = (base + gain).to(torch.float32).contiguous()
    free = int(cwq.choose_bits(dv, 0.0).sum(dtype=torch.int64).item())
    assert free > nb
    for T, lo in ((free // 2, 0), (free - 1, 0), (nb + nb // 2, 1)):
        hb, hl = cwq.choose_bits_total(dv, T, min_bits=lo)
        _assert_solved(cwq.choose_bits_total_device(dv, T, min_bits=lo), _np(hb), hl,
                       f"T={T} min_bits={lo}", T)


def test_a_total_that_fits_at_no_price_gives_lam_zero(cwq):
    v = SR.crafted_table(257, 8)
    dv = torch.from_numpy(v).cuda()
    free = SR.total_at(v, 0.0, 0, 8)
    for T in (free, free + 5, 1 << 40):
        bits, lam, total = cwq.choose_bits_total_device(dv, T)
        assert float(lam.item()) == 0.0 and SR.lam_bits(lam.item()) == 0
        assert np.array_equal(_np(bits), RR.choose_bits(v, 0.0)) and int(total.item()) == free


@pytest.mark.parametrize("nb,B", [(65, 5), (300, 16)])
def test_clamp_level_table(cwq, nb, B):
    """A -FLT_MAX row and a +FLT_MAX entry: lam_hi starts near 3.4e38 and the
    sixty halvings resolve nothing below about 3e20; the device
    solver equals the host loop there too."""
    v = SR.crafted_table(nb, B, clamp=True)
    dv = torch.from_numpy(v).cuda()
    for lo, hi in SR.ranges(B):
        for T in SR.targets(v, lo, hi):
            wb, wl, _ = SR.choose_bits_total(v, T, lo, hi)
            hb, hl = cwq.choose_bits_total(dv, T, min_bits=lo, max_bits=hi)
            assert np.array_equal(_np(hb), wb) and SR.lam_bits(hl) == SR.lam_bits(wl)
            _assert_solved(cwq.choose_bits_total_device(dv, T, min_bits=lo, max_bits=hi), wb, wl,
                           f"clamp nb={nb} B={B} range=({lo}, {hi}) T={T}", T)
    free = SR.total_at(v, 0.0, 0, B)
    _, lam, total = cwq.choose_bits_total_device(dv, free // 2)
    assert float(lam.item()) > 1e19 and int(total.item()) == B


def test_results_do_not_depend_on_the_workspace(cwq, cwqlib):
    """The same call on a workspace of 0x00 bytes and of 0xFF bytes, outputs
    pre-filled with -1: identical results, and the reference's."""
    nb, B = 257, 16
    v = SR.crafted_table(nb, B)
    dv = torch.from_numpy(v).cuda()
    T = SR.total_at(v, 0.0, 1, B - 1) // 2
    wb, wl, _ = SR.choose_bits_total(v, T, 1, B - 1)
    need = cwqlib.cwq_choose_bits_total_workspace_bytes(B)
    res = []
    for byte in (0x00, 0xFF):
        ws = torch.full((need,), byte, dtype=torch.uint8, device="cuda")
        bits = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
        lam = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
        total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        rc = cwqlib.cwq_choose_bits_total(dv.data_ptr(), nb, B, T, 1, B - 1, bits.data_ptr(),
                                          lam.data_ptr(), total.data_ptr(), ws.data_ptr(), need,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, cwqlib.cwq_last_error()
        _assert_solved((bits, lam, total), wb, wl, f"workspace of {byte:#04x}", T)
        res.append((_np(bits), _np(lam).view(np.uint64), _np(total)))
    assert all(np.array_equal(a, b) for a, b in zip(*res))


def test_python_raises_choose_bits_totals_errors(cwq):
    """nb min_bits > total_bits and a bad range raise choose_bits_total's
    ValueError, in its words, from both wrappers (the library's refusal is
    CWQ_ERR_INVALID: tests/test_rate_total_capi.py)."""
    v = SR.crafted_table(65, 8)
    dv = torch.from_numpy(v).cuda()
    for call in (cwq.choose_bits_total, cwq.choose_bits_total_device):
        with pytest.raises(ValueError, match="65 blocks at min_bits=3 exceed total_bits=194"):
            call(dv, 194, min_bits=3)
        with pytest.raises(ValueError, match="min_bits=9 outside"):
            call(dv, 1000, min_bits=9)
    assert int(cwq.choose_bits_total_device(dv, 195, min_bits=3)[2].item()) == 195
    off, tl, ts, pl, ps = _blocks("uniform")
    with pytest.raises(ValueError, match="257 blocks at min_bits=2 exceed total_bits=513"):
        cwq.encode_blocks_rate_total(tl, ts, pl, ps, SEED, 9, 513, min_bits=2, block_dim=8)
    with pytest.raises(ValueError, match="min_bits=10 outside"):
        cwq.encode_blocks_rate_total(tl, ts, pl, ps, SEED, 9, 5000, min_bits=10, block_dim=8)
    bits = cwq.encode_blocks_rate_total(tl, ts, pl, ps, SEED, 9, 514, min_bits=2, block_dim=8)[2]
    assert (bits == 2).all()


# ---- one call from the distributions to a code --------------------------------------
RAGGED = (0, 1, 7, 255, 256, 300, 8, 0, 33, 64) + (5, 12, 31, 2, 9, 17) * 5  # 40 blocks


@functools.lru_cache(maxsize=None)
def _blocks(kind):
    lens = (8,) * 257 if kind == "uniform" else RAGGED
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(77 + len(lens)))
    return (off,) + RR.inputs(rng, int(off[-1]))


def _assert_code(cwq, got, want, what):
    (gi, gs, gb), (wi, ws, wb) = got[:3], want
    assert gi.shape == wi.shape and gi.dtype == torch.int32, what
    assert np.array_equal(_np(gb), _np(wb)), f"{what}: n_bits"
    assert np.array_equal(_np(gi), _np(wi)), f"{what}: idx"
    assert np.array_equal(_u32(gs), _u32(ws)), f"{what}: sample"


@pytest.mark.parametrize("B", [9, 13])  # 13 crosses the table's split at 12 bits
def test_encode_rate_total_uniform(cwq, B):
    off, tl, ts, pl, ps = _blocks("uniform")
    nb = off.size - 1
    assert nb == 257
    T = nb * B // 2
    want = cwq.encode_blocks_rate(tl, ts, pl, ps, SEED, B, total_bits=T, block_dim=8)
    got = cwq.encode_blocks_rate_total(tl, ts, pl, ps, SEED, B, T, block_dim=8)
    _assert_code(cwq, got, want, f"uniform B={B}")
    idx, sample, bits, lam, total = got
    assert int(total.item()) == int(bits.sum().item()) <= T and float(lam.item()) > 0.0
    assert len(set(_np(bits).tolist())) >= 3
    dec = cwq.decode_blocks_var(idx, bits, pl, ps, 1, SEED, block_dim=8)
    assert np.array_equal(_u32(dec), _u32(sample))


@pytest.mark.parametrize("base,rho,lo", [(0, 1.0, 0), (5, 0.9, 1)])
def test_encode_rate_total_ragged(cwq, base, rho, lo):
    """Block sizes either side of 256 dims, where the table's scorer changes
    from a lane per row to a wave per row, and empty blocks."""
    off, tl, ts, pl, ps = _blocks("ragged")
    nb, B = off.size - 1, 9
    assert nb == 40 and {0, 1, 7, 255, 256, 300} <= set(np.diff(off).tolist())
    T = nb * B // 2
    kw = dict(min_bits=lo, rho=rho, block_off=off, block_id_base=base)
    want = cwq.encode_blocks_rate(tl, ts, pl, ps, SEED, B, total_bits=T, **kw)
    got = cwq.encode_blocks_rate_total(tl, ts, pl, ps, SEED, B, T, **kw)
    _assert_code(cwq, got, want, f"ragged base={base} rho={rho}")
    idx, sample, bits, lam, total = got
    assert int(total.item()) == int(bits.sum().item()) <= T and int(bits.min().item()) >= lo
    dec = cwq.decode_blocks_var(idx, bits, pl, ps, 1, SEED, rho=rho, block_off=off,
                                block_id_base=base)
    assert np.array_equal(_u32(dec), _u32(sample))


# ---- graph replay --------------------------------------------------------------------
def _capture(run):
    """tests/graph_replay.py's way: once eagerly on a side stream, then one capture."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(side)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run(side)
    return graph


def test_solver_replays(cwq, cwqlib):
    """One capture of cwq_choose_bits_total, replayed three times on another
    table each and on outputs and a workspace filled with 0x00, 0xFF and random
    bytes: each replay equals the eager call and the host loop on that table."""
    nb, B = 257, 8
    tables = [SR.crafted_table(nb, B, seed=s) for s in range(4)]
    T = SR.total_at(tables[0], 0.0, 0, B) // 2
    dv = torch.from_numpy(tables[0]).cuda()
    need = cwqlib.cwq_choose_bits_total_workspace_bytes(B)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    bits = torch.empty(nb, dtype=torch.int32, device="cuda")
    lam = torch.empty(1, dtype=torch.float64, device="cuda")
    total = torch.empty(1, dtype=torch.int64, device="cuda")

    def run(stream):
        rc = cwqlib.cwq_choose_bits_total(dv.data_ptr(), nb, B, T, 0, B, bits.data_ptr(),
                                          lam.data_ptr(), total.data_ptr(), ws.data_ptr(), need,
                                          stream.cuda_stream)
        assert rc == 0, cwqlib.cwq_last_error()

    graph = _capture(run)
    rng = np.random.Generator(np.random.PCG64(3))
    lams = set()
    for r, pattern in enumerate(PATTERNS):
        v = tables[r + 1]
        dv.copy_(torch.from_numpy(v))
        for t in (ws, bits, lam, total):
            fill(t, pattern, rng)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = (bits.clone(), lam.clone(), total.clone())
        eager = cwq.choose_bits_total_device(torch.from_numpy(v).cuda(), T)
        assert all(torch.equal(a, b) for a, b in zip(got, eager)), f"replay {r} against eager"
        hb, hl = cwq.choose_bits_total(torch.from_numpy(v).cuda(), T)
        _assert_solved(got, _np(hb), hl, f"replay {r} on buffers filled with {pattern!r}", T)
        lams.add(SR.lam_bits(hl))
    assert len(lams) == 3  # the replays did see different tables


def test_encode_rate_replays(cwq, cwqlib):
    """One capture of cwq_greedy_encode_rate at B = 13 (budgets either side of
    the table's split), replayed three times with the target moved: each replay
    equals the eager calls on the inputs it saw."""
    off, tl, ts, pl, ps = _blocks("uniform")
    nb, d, B = off.size - 1, 8, 13
    D, T = nb * d, nb * B // 2
    ins = [torch.from_numpy(a).cuda() for a in (tl, ts, pl, ps)]
    need = cwqlib.cwq_greedy_encode_rate_workspace_bytes(nb, D, d, B)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx = torch.empty((nb, 1), dtype=torch.int32, device="cuda")
    sample = torch.empty(D, dtype=torch.float32, device="cuda")
    bits = torch.empty(nb, dtype=torch.int32, device="cuda")
    lam = torch.empty(1, dtype=torch.float64, device="cuda")
    total = torch.empty(1, dtype=torch.int64, device="cuda")
    value = torch.empty((nb, B + 1), dtype=torch.float32, device="cuda")

    def run(stream):
        rc = cwqlib.cwq_greedy_encode_rate(
            *(t.data_ptr() for t in ins), None, nb, D, d, B, T, 0, SEED, 1.0, 0,
            idx.data_ptr(), sample.data_ptr(), bits.data_ptr(), lam.data_ptr(), total.data_ptr(),
            value.data_ptr(), ws.data_ptr(), need, None, stream.cuda_stream)
        assert rc == 0, cwqlib.cwq_last_error()

    graph = _capture(run)
    rng = np.random.Generator(np.random.PCG64(4))
    for r, (pattern, shift) in enumerate(zip(PATTERNS, (0.0, 0.25, -0.5))):
        moved = tl + np.float32(shift)
        ins[0].copy_(torch.from_numpy(moved))
        for t in (ws, idx, sample, bits, lam, total, value):
            fill(t, pattern, rng)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        what = f"replay {r} at shift {shift} on buffers filled with {pattern!r}"
        want = cwq.encode_blocks_rate(moved, ts, pl, ps, SEED, B, total_bits=T, block_dim=d)
        _assert_code(cwq, (idx, sample, bits), want, what)
        eager = cwq.encode_blocks_rate_total(moved, ts, pl, ps, SEED, B, T, block_dim=d)
        assert torch.equal(lam, eager[3]) and torch.equal(total, eager[4]), what
        tv = cwq.rate_table(moved, ts, pl, ps, B, SEED, block_dim=d)[1]
        assert np.array_equal(_u32(value), _u32(tv)), f"{what}: out_value"


# ---- the grouped coder ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _latents(D):
    from compression_without_quantization_amd.synthetic import make_latents
    return make_latents(D, bits_per_dim=1.1, off_fraction=0.5, seed=31 + D)


def _standardised_groups(cwq, ql, qs, pl, ps, starts):
    t_loc = torch.from_numpy((ql - pl) / ps).cuda()
    t_scale = torch.from_numpy(qs / ps).cuda()
    zeros, ones = torch.zeros_like(t_loc), torch.ones_like(t_loc)
    return t_loc, t_scale, zeros, ones


@pytest.mark.parametrize("total_bits", [None, "three quarters"])
def test_grouped_rate_coder(cwq, total_bits):
    D, n_bits, mgs = 4096, 8, 6
    ql, qs, pl, ps = _latents(D)
    t, p = cwq.Normal(ql, qs), cwq.Normal(pl, ps)
    var = cwq.code_grouped_greedy_sample_var(t, p, 1, n_bits, SEED, max_group_size_bits=mgs)
    target = var[2] if total_bits is None else 3 * var[2] // 4
    sample, code, total, starts, bits = cwq.code_grouped_greedy_sample_rate(
        t, p, n_bits, SEED, total_bits=None if total_bits is None else target,
        max_group_size_bits=mgs)
    assert starts == var[3] and bits.dtype == np.int32 and len(bits) == len(starts) - 1
    assert total == int(bits.sum()) <= target and isinstance(code, bytes)
    assert len(code) == (total + 7) // 8 and int(bits.max()) <= n_bits
    # the budgets: choose_bits_total on the rate table of the same standardised groups
    # (standardise is one correctly rounded float32 operation per output)
    t_loc, t_scale, zeros, ones = _standardised_groups(cwq, ql, qs, pl, ps, starts)
    tval = cwq.rate_table(t_loc, t_scale, zeros, ones, n_bits, SEED, block_off=starts)[1]
    want_bits, _ = cwq.choose_bits_total(tval, target)
    assert np.array_equal(bits, _np(want_bits))
    dec = cwq.decode_grouped_greedy_sample_var(code, starts, bits, p, 1, SEED)
    assert np.array_equal(_u32(dec), _u32(sample))
