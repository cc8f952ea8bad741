"""GPU: k_encode_prune's screening-only form, k_score_survivors and the launch
over the deferred list (DESIGN.md 4 "Deferral").

cwq_selftest_encode_uniform_defer runs every block as one tile and picks the
mode: 0 the single launch, 1 deferral on, 2 every tile deferred, 3 no slot per
block (Q = 0).  Indices and sample words must be those of prune_mode 0 (the
exact kernel, which alone is the reference here and which the CPU oracle
confirms on the small shapes), and so the same in all four modes.

What a call deferred is read back from the workspace after it
(tests/defer_layout.py, held against the header by tests/test_defer_plan.py),
so that each case is known to have taken the path it is here for: the dense
scoring alone, more than Q rows, a survivor list past its cap, a failed gate.
"""
import functools

import numpy as np
import pytest
import torch

import defer_layout as L

pytestmark = pytest.mark.gpu

SEED, BASE = 42, 3
MODES = (0, 1, 2, 3)
DIMS = (8, 16, 32, 64)
# k_score_survivors takes 8 blocks per wave (4 at d = 64): 1, 3 and 7 fill no
# wave, 70 several and a part of one
BLOCKS = (1, 3, 7, 70)
BITS = (12, 16)
CAP = 1024  # CWQ_SURVIVOR_CAP


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    return C


@functools.lru_cache(maxsize=None)
def _inputs(d, bits, nb, kind="normal"):
    from compression_without_quantization_amd.synthetic import make_blocks
    b = make_blocks(nb, d, bits, seed=900 + d + bits)
    tl, ts, pl, ps = (np.ascontiguousarray(b[k].reshape(-1)).copy() for k in
                      ("post_loc", "post_scale", "prior_loc", "prior_scale"))
    if kind == "tied":          # rows differ far below the rounding of their values
        ts[:] = np.float32(2.0 ** 40)
    elif kind == "flat":        # posterior = prior
        tl[:] = pl
        ts[:] = ps
    elif kind == "gate":        # blocks 1 .. 4 of 7 fail the screening gate, 5 is all NaN
        assert nb == 7
        ts[1 * d + 1] = np.float32("inf")
        ts[2 * d + 2] = np.float32(0.0)
        ts[3 * d + 3] = np.float32("nan")
        tl[4 * d + d // 2] = np.float32("nan")
        tl[5 * d:6 * d] = np.float32("nan")
    else:
        assert kind == "normal"
    return tl, ts, pl, ps


@functools.lru_cache(maxsize=None)
def _reference(cwq, d, bits, nb, n_steps, kind="normal"):
    """prune_mode 0: every row scored exactly by k_encode_eval."""
    dev = [torch.from_numpy(a).cuda() for a in _inputs(d, bits, nb, kind)]
    idx, sample = cwq.encode_blocks(*dev, bits, n_steps, SEED, rho=1.0, block_dim=d,
                                    block_id_base=BASE, prune_mode=0)
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.int64), sample.cpu().numpy().view(np.uint32).copy()


class Call:
    """One cwq_selftest_encode_uniform_defer call's buffers, made once so that a
    graph can replay it."""

    def __init__(self, cwqlib, d, bits, nb, n_steps, host, fill=None):
        self.lib, self.shape = cwqlib, (d, bits, nb, n_steps)
        self.dev = [torch.from_numpy(a).cuda() for a in host]
        self.enc = int(cwqlib.cwq_greedy_encode_uniform_workspace_size(nb, d))
        self.need = int(cwqlib.cwq_greedy_encode_uniform_defer_bytes(nb, d))
        self.regions, total = L.regions(self.enc, nb, d)
        assert total == self.need > self.enc
        mk = (lambda n, dt: torch.empty(n, dtype=dt, device="cuda")) if fill is None else fill
        self.idx = mk(nb * n_steps, torch.int32)
        self.sample = mk(nb * d, torch.float32)
        self.ws = mk(self.need, torch.uint8)

    def run(self, mode, stream=None):
        from compression_without_quantization_amd import _lib
        d, bits, nb, n_steps = self.shape
        st = (stream or torch.cuda.current_stream()).cuda_stream
        rc = self.lib.cwq_selftest_encode_uniform_defer(
            *[t.data_ptr() for t in self.dev], nb, d, bits, n_steps, SEED, 1.0, BASE,
            self.idx.data_ptr(), self.sample.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            _lib.options(2, None), st, mode)
        _lib.check(rc, "cwq_selftest_encode_uniform_defer")

    def result(self):
        torch.cuda.synchronize()
        d, bits, nb, n_steps = self.shape
        return (self.idx.cpu().numpy().astype(np.int64).reshape(nb, n_steps),
                self.sample.cpu().numpy().view(np.uint32).copy())

    def deferred(self):
        """(blocks on the deferred list, count words) of the call's last step."""
        torch.cuda.synchronize()
        w = self.ws.cpu().numpy()
        rd = lambda k: w[self.regions[k][0]:self.regions[k][0] + self.regions[k][1]].view(np.uint32)
        n = int(rd("dcount")[0])
        assert 0 <= n <= self.shape[2]
        return sorted(int(g) for g in rd("dlist")[:n]), rd("count").copy()


def _same(got, want, what):
    for name, g, w in zip(("indices", "sample words"), got, want):
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, f"{what}: {name}: {bad.size} of {w.size} differ, first at {bad[:8]}"


def _all_modes(cwq, cwqlib, d, bits, nb, n_steps, kind="normal"):
    """Every mode against prune_mode 0; {mode: (deferred blocks, count words)}."""
    want = _reference(cwq, d, bits, nb, n_steps, kind)
    call = Call(cwqlib, d, bits, nb, n_steps, _inputs(d, bits, nb, kind))
    seen = {}
    for mode in MODES:
        call.run(mode)
        _same(call.result(), want, f"d={d} bits={bits} nb={nb} steps={n_steps} {kind} mode {mode}")
        if mode:
            seen[mode] = call.deferred()
    return seen


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("nb", BLOCKS)
@pytest.mark.parametrize("d", DIMS)
def test_modes_match_the_exact_kernel(cwq, cwqlib, d, nb, bits):
    seen = _all_modes(cwq, cwqlib, d, bits, nb, 1)
    every = list(range(nb))
    # on: a block is listed with 1 .. Q rows or deferred with count 0
    dl, cnt = seen[1]
    assert all((cnt[g] == 0) == (g in dl) and cnt[g] <= L.Q for g in every), (dl, cnt)
    assert len(dl) < max(nb // 2, 1), f"ordinary blocks deferred: {dl}"
    # every tile deferred; Q = 0: a block always has a row that reaches its tau
    for mode in (2, 3):
        assert seen[mode][0] == every and not seen[mode][1].any(), (mode, seen[mode])


@pytest.mark.parametrize("d", DIMS)
def test_three_steps(cwq, cwqlib, d):
    """Steps 1 and 2 run the STEP0 = false instances of all three kernels."""
    _all_modes(cwq, cwqlib, d, 12, 7, 3)
    _all_modes(cwq, cwqlib, d, 12, 70, 3)


@pytest.mark.parametrize("d,nb", [(8, 7), (32, 3), (64, 1)])
def test_reference_is_the_oracles(cwq, oracle, d, nb):
    """prune_mode 0, the reference above, against the CPU oracle."""
    from oracle import oracle as O
    tl, ts, pl, ps = _inputs(d, 12, nb)
    idx, words = _reference(cwq, d, 12, nb, 1)
    for g in range(nb):
        sl = slice(g * d, (g + 1) * d)
        i, s = O.greedy_encode(tl[sl], ts[sl], pl[sl], ps[sl], [0, d], 12, 1, SEED, 1.0, BASE + g)
        assert np.array_equal(np.asarray(i).reshape(-1), idx[g])
        assert np.array_equal(np.ascontiguousarray(s, dtype=np.float32).view(np.uint32), words[sl])


@pytest.mark.parametrize("d", DIMS)
def test_near_ties(cwq, cwqlib, d):
    """Every row of a block ties (target scale 2^40).  2^8 rows: all reach the
    final tau, more than Q and fewer than the list holds.  2^12 rows: the list
    overflows.  Either way every block is deferred, in mode 1 too, and row 0
    wins."""
    for bits in (8, 12):
        assert (1 << bits > CAP) == (bits == 12)
        seen = _all_modes(cwq, cwqlib, d, bits, 7, 1, "tied")
        assert seen[1][0] == list(range(7)), (bits, seen[1])
        assert (_reference(cwq, d, bits, 7, 1, "tied")[0] == 0).all()


@pytest.mark.parametrize("d", DIMS)
def test_flat_targets(cwq, cwqlib, d):
    _all_modes(cwq, cwqlib, d, 12, 7, 1, "flat")
    _all_modes(cwq, cwqlib, d, 12, 7, 3, "flat")


@pytest.mark.parametrize("d", DIMS)
def test_gate_failures_among_ordinary_blocks(cwq, cwqlib, d):
    """inf, 0 and NaN scales and a NaN mean fail the screening gate: their
    blocks go to the deferred list and the full kernel's exact pass; blocks 0
    and 6 do not.  The all-NaN block ends with index 0."""
    seen = _all_modes(cwq, cwqlib, d, 12, 7, 1, "gate")
    dl, cnt = seen[1]
    assert set(dl) >= {1, 2, 3, 4, 5} and not cnt[1:6].any(), (dl, cnt)
    assert 1 <= cnt[0] <= L.Q and 1 <= cnt[6] <= L.Q, cnt
    assert (_reference(cwq, d, 12, 7, 1, "gate")[0][5] == 0).all()


@pytest.mark.parametrize("pattern", [0x00, 0xFF, "random"])
def test_poisoned_workspace_and_outputs(cwq, cwqlib, pattern):
    """Nothing depends on what the workspace (the new regions, their counter
    included) or the output buffers held: every tile writes its count, the
    launcher zeroes the counter."""
    rng = np.random.Generator(np.random.PCG64(7))

    def fill(n, dt):
        nbytes = n * torch.empty(0, dtype=dt).element_size()
        raw = rng.integers(0, 256, nbytes, dtype=np.uint8) if pattern == "random" else \
            np.full(nbytes, pattern, np.uint8)
        return torch.from_numpy(raw).cuda().view(dt)

    for d, nb, kind in ((32, 7, "normal"), (16, 7, "gate")):
        want = _reference(cwq, d, 12, nb, 3, kind)
        call = Call(cwqlib, d, 12, nb, 3, _inputs(d, 12, nb, kind), fill=fill)
        for mode in (1, 3, 1):  # back to back on the same workspace
            call.run(mode)
            _same(call.result(), want, f"d={d} {kind} mode {mode} pattern {pattern!r}")


def test_graph_capture_and_replay(cwq, cwqlib):
    """The launches of a deferred call are stream work alone, the deferred
    list's length is read on the device: one capture, replayed on poisoned
    outputs and workspace.  Three steps: STEP0 = false is captured too, and two
    key resets with the same arguments lie between the scoring launches."""
    d, bits, nb, n_steps = 32, 12, 70, 3
    want = _reference(cwq, d, bits, nb, n_steps)
    call = Call(cwqlib, d, bits, nb, n_steps, _inputs(d, bits, nb))
    call.run(1)  # (first call outside the capture: module loading)
    _same(call.result(), want, "before the capture")
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        call.run(1, stream=side)
    for _ in range(2):
        call.idx.fill_(-1)
        call.sample.fill_(float("nan"))
        call.ws.fill_(0xFF)
        graph.replay()
        _same(call.result(), want, "graph replay")


def test_mode_and_workspace_are_validated(cwq, cwqlib):
    call = Call(cwqlib, 32, 12, 3, 1, _inputs(32, 12, 3))
    for bad in (-1, 4):
        with pytest.raises(Exception):
            call.run(bad)
    call.ws = call.ws[:call.enc]  # the encoder's own size is too small for this entry
    with pytest.raises(Exception):
        call.run(1)
