"""GPU: the rate table (cwq_rate_table) against the CPU oracle.

Column b of the expected table is ``oracle.greedy_encode`` at b bits and one
step; the expected value is the winning row's log-density in the coder's own
arithmetic (tests/rate_reference.py).  Every comparison is bit for bit: int32
indices, uint32 views of the values; no tolerance anywhere.  The shapes are the
smallest that cross each boundary of the call: 4,096 candidates (the levels
launch hands over to the tuned encoders between columns 11 and 12), rows that do
not start on a Philox block, a first tile that spans levels 0 .. 8, blocks on
either side of the long-row length, and one block spread over many workgroups."""
import functools

import numpy as np
import pytest
import torch

import rate_reference as RR
from graph_replay import replay_check
from poison import poisoned

pytestmark = pytest.mark.gpu

LOWEST = np.float32(-3.4028234663852886e38)
CSR_OFF = (0, 0, 1, 6, 70, 70, 335)

# name -> (block lengths, uniform d or None, B, seed, block_id_base, rho)
CASES = {
    "u32x5_B13": ((32,) * 5, 32, 13, 42, 0, 1.0),
    "u12x9_B9": ((12,) * 9, 12, 9, 43, 0, 1.0),
    "u7x9_B9": ((7,) * 9, 7, 9, 44, 0, 1.0),
    "u12x9_B0": ((12,) * 9, 12, 0, 43, 0, 1.0),
    "u12x9_B1": ((12,) * 9, 12, 1, 43, 0, 1.0),
    "csr_B10": (tuple(np.diff(CSR_OFF).tolist()), None, 10, 45, 0, 1.0),
    "u8x1_B13": ((8,), 8, 13, 46, 0, 1.0),
    # 1000 * seed wraps past 2^31 inside step_seed
    "u12x9_wrap_rho": ((12,) * 9, 12, 9, 2147483, 2, 0.7),
}


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


@functools.lru_cache(maxsize=None)
def _case(name):
    lens, d, B, seed, base, rho = CASES[name]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(sum(map(ord, name))))
    return (off,) + RR.inputs(rng, int(off[-1]))


@functools.lru_cache(maxsize=None)
def _want(name):
    """The oracle's table, once per case."""
    from oracle import oracle as O
    O.build()
    lens, d, B, seed, base, rho = CASES[name]
    off, tl, ts, pl, ps = _case(name)
    idx, value = RR.table(O, tl, ts, pl, ps, off, B, seed, rho=rho, block_id_base=base)
    idx.setflags(write=False)
    value.setflags(write=False)
    return idx, value


def _run(cwq, name, **kw):
    lens, d, B, seed, base, rho = CASES[name]
    off, tl, ts, pl, ps = _case(name)
    blocks = dict(block_dim=d) if d else dict(block_off=off)
    return cwq.rate_table(tl, ts, pl, ps, B, seed, rho=rho, block_id_base=base, **blocks, **kw)


def _assert_table(got, want, what):
    (gi, gv), (wi, wv) = got, want
    gi, gv = _i32(gi), _u32(gv)
    assert gi.shape == wi.shape and gv.shape == wv.shape, what
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: {len(bad)} indices differ, first (block, budget) " \
                          f"{bad[:4].tolist()}: got {gi[tuple(bad[0])]}, want {wi[tuple(bad[0])]}"
    bad = np.argwhere(gv != _u32(wv))
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first (block, budget) " \
                          f"{bad[:4].tolist()}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_is_the_oracles_encode_at_every_budget(cwq, oracle, name):
    _assert_table(_run(cwq, name), _want(name), name)


@pytest.mark.parametrize("name", ["u32x5_B13", "csr_B10"])
def test_prune_mode_never_changes_the_table(cwq, oracle, name):
    _assert_table(_run(cwq, name, prune_mode=0), _want(name), f"{name}, prune_mode 0")


@pytest.mark.parametrize("B", [9, 13])
def test_block_of_nan_targets_is_index_0_at_lowest(cwq, oracle, B):
    off, tl, ts, pl, ps = _case("u32x5_B13")
    tl = tl.copy()
    tl[64:96] = np.nan  # block 2
    idx, value = cwq.rate_table(tl, ts, pl, ps, B, 42, block_dim=32)
    assert (_i32(idx)[2] == 0).all()
    assert (_u32(value)[2] == _u32(np.full(B + 1, LOWEST))).all()
    wi, wv = _want("u32x5_B13")
    keep = [0, 1, 3, 4]
    _assert_table((_i32(idx)[keep], value[keep]), (wi[keep, :B + 1], wv[keep, :B + 1]),
                  "the other blocks")


@functools.lru_cache(maxsize=None)
def _props():
    rng = np.random.Generator(np.random.PCG64(300))
    return RR.inputs(rng, 300 * 32)


def test_properties_of_a_table_and_encode_blocks_columns(cwq):
    tl, ts, pl, ps = _props()
    B = 12
    idx, value = cwq.rate_table(tl, ts, pl, ps, B, 7, block_dim=32)
    idx, value = _i32(idx), value.cpu().numpy()
    assert (np.diff(value, axis=1) >= 0).all(), "value[:, b] decreases somewhere"
    assert (idx >= 0).all() and (idx < (1 << np.arange(B + 1))[None, :]).all()
    for b in range(1, B + 1):
        new = (idx[:, b] >= (1 << (b - 1))) & (idx[:, b] < (1 << b))
        assert (new | (idx[:, b] == idx[:, b - 1])).all(), f"budget {b}"
    for b in (0, 5, 11, 12):
        ei, _ = cwq.encode_blocks(tl, ts, pl, ps, b, 1, 7, block_dim=32)
        assert np.array_equal(_i32(ei)[:, 0], idx[:, b]), f"encode_blocks at {b} bits"


@pytest.mark.parametrize("pattern", [0xFF, "random"])
@pytest.mark.parametrize("name", ["u32x5_B13", "csr_B10"])
def test_table_does_not_depend_on_buffer_contents(cwq, oracle, name, pattern):
    lens, d, B, _, _, _ = CASES[name]
    nb, D = len(lens), int(sum(lens))
    with poisoned(pattern) as filled:
        got = _run(cwq, name)
        torch.cuda.synchronize()
    from compression_without_quantization_amd.ratetable import rate_table_workspace_bytes
    filled.assert_workspace(rate_table_workspace_bytes(nb, D, max(lens), B), name)
    _assert_table(got, _want(name), f"{name} on buffers filled with {pattern!r}")


def test_graph_replay_equals_the_eager_call(cwq, oracle):
    """One capture on one stream, replayed with the inputs changed between
    replays: each replay is the eager call on the inputs it saw."""
    from compression_without_quantization_amd import _lib
    from compression_without_quantization_amd.ratetable import rate_table_workspace_bytes
    name = "u32x5_B13"
    lens, d, B, seed, base, rho = CASES[name]
    off, tl, ts, pl, ps = _case(name)
    nb, D = len(lens), int(off[-1])
    lib = _lib.load()
    dev = torch.device("cuda")
    ins = [torch.from_numpy(a).to(dev) for a in (tl, ts, pl, ps)]
    idx = torch.empty((nb, B + 1), dtype=torch.int32, device=dev)
    value = torch.empty((nb, B + 1), dtype=torch.float32, device=dev)
    ws = torch.empty(rate_table_workspace_bytes(nb, D, d, B), dtype=torch.uint8, device=dev)

    def run(stream):
        rc = lib.cwq_rate_table(*(t.data_ptr() for t in ins), None, nb, D, d, B, seed, rho, base,
                                idx.data_ptr(), value.data_ptr(), ws.data_ptr(), ws.numel(), None,
                                stream.cuda_stream)
        assert rc == 0, lib.cwq_last_error()

    wi, wv = _want(name)
    replay_check(run, {"idx": idx, "value": value}, [ws], {"idx": wi, "value": wv}, name)

    # the inputs changed between replays of one capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(side)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run(side)
    for shift in (0.25, -0.5):
        ins[0].copy_(torch.from_numpy(tl + np.float32(shift)))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = (idx.clone(), value.clone())
        eager = cwq.rate_table(tl + np.float32(shift), ts, pl, ps, B, seed, rho=rho,
                               block_id_base=base, block_dim=d)
        _assert_table(got, (_i32(eager[0]), eager[1].cpu().numpy()), f"replay at shift {shift}")
