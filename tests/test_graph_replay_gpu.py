"""GPU: every capturable entry point captured into a graph and replayed.

include/cwq.h: calls are stream-ordered, allocate nothing and do not
synchronise, and so can be captured, except those it names.  Each case here is
one call through the C ABI on tensors made beforehand, at the smallest shape
at which its path exists (tests/encode_shapes.py's GRAPH_CASES;
tests/test_encode_plan.py checks the paths on the CPU), held by
tests/graph_replay.py to a reference: run eagerly, captured once, replayed
three times on outputs and workspaces filled with 0x00, 0xFF and random bytes.
The reference is the CPU oracle (encoders, decoders, RNG), the NumPy
restatements of the beam encoder and of backfitting, or NumPy itself.

Encoders run at 1, 2, 3 and 4 steps: from three steps on one capture holds two
key resets with the same arguments between its scoring launches, which is where
replays went wrong while those were memset nodes (DESIGN.md 4 "Graph replay").
"""
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import encode_shapes as S
from graph_replay import Steps, replay_check

pytestmark = pytest.mark.gpu
RHO, SEED, BASE = S.GRAPH_RHO, S.GRAPH_SEED, S.GRAPH_BASE


def _wrap32(x):
    return int(np.int32(np.uint32(int(x) & 0xFFFFFFFF)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _empty(n, dtype):
    return torch.empty(int(n), dtype=dtype, device="cuda")


def _values(rng, D):
    tl = rng.standard_normal(D).astype(np.float32)
    ts = rng.uniform(0.3, 0.9, D).astype(np.float32)
    pl = (0.25 * rng.standard_normal(D)).astype(np.float32)
    ps = rng.uniform(0.8, 1.3, D).astype(np.float32)
    return tl, ts, pl, ps


@pytest.fixture(scope="module")
def lib(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return cwqlib


def _ok(rc, what):
    from compression_without_quantization_amd import _lib
    _lib.check(rc, what)


# ---------------------------------------------------------------------------
# the encoders
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _enc_inputs(name):
    """(block offsets, the four host arrays) of a GRAPH_CASES entry."""
    from compression_without_quantization_amd.synthetic import make_blocks
    c = S.GRAPH_CASES[name]
    off = np.concatenate([[0], np.cumsum(c["sizes"])]).astype(np.int64)
    if c["d"] is not None:
        b = make_blocks(len(c["sizes"]), c["d"], c["bits"], seed=300 + c["d"] + c["bits"])
        host = tuple(np.ascontiguousarray(b[k].reshape(-1)) for k in
                     ("post_loc", "post_scale", "prior_loc", "prior_scale"))
    else:
        host = _values(np.random.Generator(np.random.PCG64(2000 + int(off[-1]) + c["bits"])),
                       int(off[-1]))
    return off, host


@functools.lru_cache(maxsize=None)
def _enc_oracle(name, n_steps):
    """(blocks, idx of those blocks, sample of their dims) from the CPU oracle:
    every block, or every oracle_stride-th and the last."""
    from oracle import oracle as O
    O.build()
    c = S.GRAPH_CASES[name]
    off, (tl, ts, pl, ps) = _enc_inputs(name)
    nb, stride = len(c["sizes"]), c.get("oracle_stride", 1)
    if stride == 1:
        wi, ws = O.greedy_encode(tl, ts, pl, ps, off, c["bits"], n_steps, _wrap32(SEED), RHO, BASE)
        return np.arange(nb), wi, ws
    blocks = np.unique(np.concatenate([np.arange(0, nb, stride), [nb - 1]]))
    d = c["d"]

    def one(g):  # block g alone, numbered g: the same seed as inside the whole call
        sl = slice(g * d, (g + 1) * d)
        i, s = O.greedy_encode(tl[sl], ts[sl], pl[sl], ps[sl], [0, d], c["bits"], n_steps,
                               _wrap32(SEED), RHO, BASE + int(g))
        return i[0], s

    with ThreadPoolExecutor(16) as pool:  # (the oracle's C code runs without the GIL)
        res = list(pool.map(one, blocks))
    return blocks, np.stack([r[0] for r in res]), np.concatenate([r[1] for r in res])


class EncodeCall:
    """One encoder call's tensors, made once, and the call on a stream."""

    def __init__(self, lib, name, n_steps, prune=None):
        c = S.GRAPH_CASES[name]
        self.lib, self.c, self.n_steps = lib, c, n_steps
        self.prune = c["prune"] if prune is None else prune
        off, host = _enc_inputs(name)
        self.off, self.nb, self.D = off, len(c["sizes"]), int(off[-1])
        self.dev = [_dev(a) for a in host]
        self.off_dev = _dev(off)
        self.longest = max(c["sizes"])
        if c["entry"] == "defer":
            need = lib.cwq_greedy_encode_uniform_defer_bytes(self.nb, c["d"])
        elif c["entry"] == "uniform":
            need = lib.cwq_greedy_encode_uniform_workspace_size(self.nb, c["d"])
        else:
            need = lib.cwq_greedy_encode_workspace_size(self.nb, self.D, self.longest)
        assert need > 0
        self.ws = _empty(need, torch.uint8)
        self.idx = _empty(self.nb * n_steps, torch.int32)
        self.sample = _empty(self.D, torch.float32)

    def run(self, stream):
        from compression_without_quantization_amd import _lib
        c, st = self.c, stream.cuda_stream
        ptrs = [t.data_ptr() for t in self.dev]
        tail = (c["bits"], self.n_steps, _wrap32(SEED), RHO, BASE, self.idx.data_ptr(),
                self.sample.data_ptr(), self.ws.data_ptr(), self.ws.numel())
        opts = _lib.options(self.prune)
        if c["entry"] == "uniform":
            rc = self.lib.cwq_greedy_encode_uniform(*ptrs, self.nb, c["d"], *tail, opts, st)
        elif c["entry"] == "defer":
            rc = self.lib.cwq_selftest_encode_uniform_defer(*ptrs, self.nb, c["d"], *tail, opts,
                                                            st, c["defer"])
        elif c["entry"] == "csr":
            rc = self.lib.cwq_greedy_encode(*ptrs, self.off_dev.data_ptr(), self.nb, self.D,
                                            self.longest, *tail, opts, st)
        else:
            rc = self.lib.cwq_selftest_encode_rows_wave(*ptrs, self.off_dev.data_ptr(), self.nb,
                                                        self.D, self.longest, *tail, st)
        _ok(rc, c["entry"])

    def outputs(self):
        return {"idx": self.idx, "sample": self.sample}

    def layouts(self):
        return {"idx": Steps("idx", self.n_steps, self.off),
                "sample": Steps("sample", self.n_steps, self.off)}


def _enc_want(lib, name, n_steps):
    """The whole call's (idx, sample).  With an oracle stride: the exact
    kernel's eager result, after the oracle has confirmed it on its blocks."""
    blocks, wi, ws = _enc_oracle(name, n_steps)
    c = S.GRAPH_CASES[name]
    if blocks.size == len(c["sizes"]):
        return wi, ws
    exact = EncodeCall(lib, name, n_steps, prune=0)
    exact.run(torch.cuda.current_stream())
    torch.cuda.synchronize()
    idx = exact.idx.cpu().numpy().reshape(-1, n_steps)
    sample = exact.sample.cpu().numpy()
    d = c["d"]
    dims = (blocks[:, None] * d + np.arange(d)[None, :]).reshape(-1)
    assert np.array_equal(idx[blocks], wi), "the exact kernel against the oracle: indices"
    assert np.array_equal(sample[dims].view(np.uint32), ws.view(np.uint32)), \
        "the exact kernel against the oracle: sample"
    return idx, sample


@pytest.mark.parametrize("n_steps", S.GRAPH_STEPS)
@pytest.mark.parametrize("name", list(S.GRAPH_CASES))
def test_encoder_replays(lib, oracle, name, n_steps):
    wi, ws = _enc_want(lib, name, n_steps)
    call = EncodeCall(lib, name, n_steps)
    replay_check(call.run, call.outputs(), [call.ws], {"idx": wi, "sample": ws},
                 f"{name}, {n_steps} steps", call.layouts())


# ---------------------------------------------------------------------------
# the decoders: each decodes the oracle's indices of an encoder case
# ---------------------------------------------------------------------------
# (tests/test_decode_plan.py checks on the CPU which kernel each case takes)
@pytest.mark.parametrize("n_steps", S.GRAPH_DECODE_STEPS)
@pytest.mark.parametrize("case", list(S.GRAPH_DECODE_CASES))
def test_decoder_replays(lib, oracle, case, n_steps):
    name, entry, _ = S.GRAPH_DECODE_CASES[case]
    c = S.GRAPH_CASES[name]
    off, (_, _, pl, ps) = _enc_inputs(name)
    _, wi, _ = _enc_oracle(name, n_steps)
    want = oracle.greedy_decode(wi, pl, ps, off, c["bits"], n_steps, _wrap32(SEED), RHO, BASE)
    idx, dpl, dps, doff = _dev(wi.astype(np.int32)), _dev(pl), _dev(ps), _dev(off)
    nb, D = len(c["sizes"]), int(off[-1])
    out = _empty(D, torch.float32)

    def run(stream):
        if entry == "uniform":
            rc = lib.cwq_greedy_decode_uniform(idx.data_ptr(), dpl.data_ptr(), dps.data_ptr(), nb,
                                               c["d"], c["bits"], n_steps, _wrap32(SEED), RHO,
                                               BASE, out.data_ptr(), stream.cuda_stream)
        else:
            rc = lib.cwq_greedy_decode(idx.data_ptr(), dpl.data_ptr(), dps.data_ptr(),
                                       doff.data_ptr(), nb, D, max(c["sizes"]), c["bits"],
                                       n_steps, _wrap32(SEED), RHO, BASE, out.data_ptr(),
                                       stream.cuda_stream)
        _ok(rc, "decode")

    replay_check(run, {"sample": out}, [], {"sample": want}, f"decode {case}, {n_steps} steps",
                 {"sample": Steps("sample", n_steps, off)})


def test_variable_bits_decoder_replays(lib, oracle):
    """Blocks coded at a bit count each are decoded by cwq_greedy_decode_uniform
    with CWQ_MAX_BITS_PER_STEP as the indices' range."""
    d, nb, n_steps = 32, 40, 2
    tl, ts, pl, ps = _values(np.random.Generator(np.random.PCG64(31)), nb * d)
    bits = [4 + g % 9 for g in range(nb)]
    wi = np.zeros((nb, n_steps), np.int32)
    for g in range(nb):
        sl = slice(g * d, (g + 1) * d)
        wi[g] = oracle.greedy_encode(tl[sl], ts[sl], pl[sl], ps[sl], [0, d], bits[g], n_steps,
                                     _wrap32(SEED), RHO, BASE + g)[0][0]
    assert wi.max() >= 1 << 11
    off = np.arange(nb + 1, dtype=np.int64) * d
    want = oracle.greedy_decode(wi, pl, ps, off, 30, n_steps, _wrap32(SEED), RHO, BASE)
    idx, dpl, dps, out = _dev(wi), _dev(pl), _dev(ps), _empty(nb * d, torch.float32)

    def run(stream):
        _ok(lib.cwq_greedy_decode_uniform(idx.data_ptr(), dpl.data_ptr(), dps.data_ptr(), nb, d, 30,
                                          n_steps, _wrap32(SEED), RHO, BASE, out.data_ptr(),
                                          stream.cuda_stream), "decode")

    replay_check(run, {"sample": out}, [], {"sample": want}, "variable-bits decode",
                 {"sample": Steps("sample", n_steps, off)})


# ---------------------------------------------------------------------------
# beam search, beam search under budgets, backfitting: four steps, on the
# layouts of their own graph tests
# ---------------------------------------------------------------------------
def test_beam_encode_replays(lib, oracle):
    import test_beam_gpu as TB
    n_bits, n_steps, beam = 5, 4, 4
    t = TB._tensors(lib, TB._ragged(), n_steps, beam)
    wi, ws, wv = TB._reference(TB._ragged, n_bits, n_steps, beam, 1.0, TB.SEED, TB.BASE)

    def run(stream):
        assert TB._raw(lib, t, n_bits, n_steps, beam, stream=stream.cuda_stream) == 0

    off = TB._ragged()[0]
    replay_check(run, {"idx": t["idx"], "sample": t["sample"], "value": t["value"]}, [t["ws"]],
                 {"idx": wi.astype(np.int32), "sample": ws, "value": wv}, "cwq_beam_encode, 4 steps",
                 {"idx": Steps("idx", n_steps, off), "sample": Steps("sample", n_steps, off)})


def test_beam_encode_var_replays(lib, oracle):
    import test_beam_var_gpu as TV
    n_steps, beam = 4, 8
    bits = TV.ragged_bits()
    t = TV._tensors(lib, TV._ragged(), bits, n_steps, beam)
    wi, ws, wv = TV._reference(TV._ragged, bits, n_steps, beam, 0.7, TV.SEED, TV.BASE)

    def run(stream):
        with torch.cuda.stream(stream):  # (the helper enqueues on the current stream)
            assert TV._raw(lib, t, 7, n_steps, beam, rho=0.7) == 0

    off = TV._ragged()[0]
    replay_check(run, {"idx": t["idx"], "sample": t["sample"], "value": t["value"]}, [t["ws"]],
                 {"idx": wi.astype(np.int32), "sample": ws, "value": wv},
                 "cwq_beam_encode_var, 4 steps",
                 {"idx": Steps("idx", n_steps, off), "sample": Steps("sample", n_steps, off)})


@functools.lru_cache(maxsize=None)
def _oracle_table(n_bits, n_steps, rho):
    """The greedy coder's table of test_backfit_gpu's ragged layout, from the oracle."""
    import test_backfit_gpu as TF
    from oracle import oracle as O
    off, tl, ts, pl, ps = TF._ragged()
    return O.greedy_encode(tl, ts, pl, ps, off, n_bits, n_steps, _wrap32(TF.SEED), rho,
                           TF.BASE)[0].astype(np.int32)


def test_backfit_replays(lib, oracle):
    """The table is refined in place, so every run starts from a copy of it made
    by a launch of the captured sequence itself."""
    import test_backfit_gpu as TF
    n_bits, n_steps, sweeps = 5, 4, 2
    table = _oracle_table(n_bits, n_steps, 0.7)
    t = TF._tensors(lib, TF._ragged(), table, n_steps)
    start = t["idx"].clone()
    wi, ws, wvals, wacc, _ = TF._reference(TF._ragged, TF._Fn(_oracle_table, n_bits, n_steps, 0.7),
                                           n_bits, n_steps, sweeps, 0.7, TF.SEED, TF.BASE)

    def run(stream):
        with torch.cuda.stream(stream):
            t["idx"].copy_(start)
            assert TF._raw(lib, t, n_bits, n_steps, sweeps) == 0

    off = TF._ragged()[0]
    replay_check(run, {"idx": t["idx"], "sample": t["sample"], "value": t["value"], "acc": t["acc"]},
                 [t["ws"]],
                 {"idx": wi.astype(np.int32), "sample": ws,
                  "value": np.ascontiguousarray(wvals[:, -1], dtype=np.float32),
                  "acc": np.asarray(wacc, np.int32)}, "cwq_greedy_backfit, 4 steps",
                 {"idx": Steps("idx", n_steps, off), "sample": Steps("sample", n_steps, off)})


# ---------------------------------------------------------------------------
# single calls
# ---------------------------------------------------------------------------
def test_stateless_normal_sample_replays(lib, oracle):
    d, n = 37, 129
    rng = np.random.Generator(np.random.PCG64(5))
    loc, scale = rng.standard_normal(d).astype(np.float32), rng.uniform(0.5, 2, d).astype(np.float32)
    want = oracle.stateless_normal_sample(loc, scale, n, _wrap32(SEED))
    dl, dsc, out = _dev(loc), _dev(scale), _empty(n * d, torch.float32)

    def run(stream):
        _ok(lib.cwq_stateless_normal_sample(dl.data_ptr(), dsc.data_ptr(), d, n, _wrap32(SEED),
                                            out.data_ptr(), stream.cuda_stream), "normal_sample")

    replay_check(run, {"out": out}, [], {"out": np.asarray(want, np.float32)},
                 "cwq_stateless_normal_sample")


def test_elementwise_replays(lib, oracle):
    """standardise and destandardise are one or two correctly rounded float32
    operations per element, which NumPy repeats exactly; the KL takes a
    logarithm, whose float32 rounding is the oracle's to state."""
    n = 1027
    ql, qs, pl, ps = _values(np.random.Generator(np.random.PCG64(6)), n)
    d = [_dev(a) for a in (ql, qs, pl, ps)]
    tl, ts, kl, ds = (_empty(n, torch.float32) for _ in range(4))
    want_tl, want_ts = (ql - pl) / ps, qs / ps
    assert want_tl.dtype == np.float32
    want_ds = (ps * ql).astype(np.float32) + pl

    def run(stream):
        st = stream.cuda_stream
        p = [t.data_ptr() for t in d]
        _ok(lib.cwq_standardise(*p, n, tl.data_ptr(), ts.data_ptr(), st), "standardise")
        _ok(lib.cwq_kl_normal_normal(*p, n, kl.data_ptr(), st), "kl")
        _ok(lib.cwq_destandardise(p[0], p[2], p[3], n, ds.data_ptr(), st), "destandardise")

    replay_check(run, {"t_loc": tl, "t_scale": ts, "kl": kl, "destandardised": ds}, [],
                 {"t_loc": want_tl, "t_scale": want_ts,
                  "kl": oracle.kl_normal_normal(ql, qs, pl, ps), "destandardised": want_ds},
                 "standardise, kl_normal_normal, destandardise")


def _bits_inputs(lens):
    rng = np.random.Generator(np.random.PCG64(2024 + len(lens)))
    D = int(sum(lens))
    ql = (0.6 * rng.standard_normal(D)).astype(np.float32)
    qs = rng.uniform(0.4, 1.2, D).astype(np.float32)
    return ql, qs, np.zeros(D, np.float32), np.ones(D, np.float32)


def _bits_want(oracle, arrays, off, extra, n_steps):
    kl = oracle.kl_normal_normal(*arrays).astype(np.float64)
    S_g = np.array([np.cumsum(kl[a:b])[-1] if b > a else 0.0 for a, b in zip(off[:-1], off[1:])])
    x = (S_g / np.log(2.0) + extra) / n_steps
    assert np.abs(x - np.round(x)).min() > 1e-6  # no block on an integer boundary
    return np.clip(np.ceil(x), 0, 30).astype(np.int32), (S_g / np.log(2.0)).astype(np.float32)


def test_block_bits_replays(lib, oracle):
    extra = 1.0 / math.log(2.0)
    nb, d = 96, 32
    uni = _bits_inputs([d] * nb)
    lens = S.ROWS_WAVE_LENGTHS[:12]
    rag = _bits_inputs(lens)
    off_u = np.arange(nb + 1) * d
    off_r = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    want_u = _bits_want(oracle, uni, off_u, extra, 1)
    want_r = _bits_want(oracle, rag, off_r, extra, 2)
    du, dr, doff = [_dev(a) for a in uni], [_dev(a) for a in rag], _dev(off_r)
    bu, ku = _empty(nb, torch.int32), _empty(nb, torch.float32)
    br, kr = _empty(len(lens), torch.int32), _empty(len(lens), torch.float32)

    def run(stream):
        st = stream.cuda_stream
        _ok(lib.cwq_block_bits(*[t.data_ptr() for t in du], nb, d, extra, 0, 30, bu.data_ptr(),
                               ku.data_ptr(), st), "block_bits")
        _ok(lib.cwq_block_bits_csr(*[t.data_ptr() for t in dr], doff.data_ptr(), len(lens),
                                   int(off_r[-1]), extra, 2, 0, 30, br.data_ptr(), kr.data_ptr(),
                                   st), "block_bits_csr")

    replay_check(run, {"bits": bu, "kl_bits": ku, "bits_csr": br, "kl_bits_csr": kr}, [],
                 {"bits": want_u[0], "kl_bits": want_u[1], "bits_csr": want_r[0],
                  "kl_bits_csr": want_r[1]}, "cwq_block_bits, cwq_block_bits_csr")


def test_pack_and_unpack_replay(lib):
    """The packed stream against NumPy's packbits of the fields' bits, LSB
    first (test_varbits_gpu.py holds that to binary_io.py), and back."""
    nb, n_steps = 301, 3
    rng = np.random.Generator(np.random.PCG64(9))
    bits = rng.integers(0, 31, nb).astype(np.int32)
    bits[0] = bits[-1] = 0
    idx = (rng.integers(0, 1 << 30, (nb, n_steps)) & ((1 << bits.astype(np.int64)) - 1)[:, None]) \
        .astype(np.int32)
    w = np.repeat(bits.astype(np.int64), n_steps)
    total = int(w.sum())
    field = np.repeat(np.arange(w.size), w)
    pos = np.arange(total) - (np.cumsum(w) - w)[field]
    stream_bits = ((idx.reshape(-1).astype(np.int64)[field] >> pos) & 1).astype(np.uint8)
    packed = np.packbits(stream_bits)
    didx, dbits = _dev(idx), _dev(bits)
    out, tot = _empty(packed.size, torch.uint8), _empty(1, torch.int64)
    back = _empty(nb * n_steps, torch.int32)
    ws = _empty(lib.cwq_pack_indices_var_workspace_size(nb), torch.uint8)

    def run(stream):
        st = stream.cuda_stream
        _ok(lib.cwq_pack_indices_var(didx.data_ptr(), dbits.data_ptr(), nb, n_steps, out.data_ptr(),
                                     packed.size, tot.data_ptr(), ws.data_ptr(), ws.numel(), st),
            "pack")
        _ok(lib.cwq_unpack_indices_var(out.data_ptr(), packed.size, dbits.data_ptr(), nb, n_steps,
                                       back.data_ptr(), ws.data_ptr(), ws.numel(), st), "unpack")

    replay_check(run, {"bytes": out, "total_bits": tot, "unpacked": back}, [ws],
                 {"bytes": packed, "total_bits": np.array([total], np.int64), "unpacked": idx},
                 "cwq_pack_indices_var, cwq_unpack_indices_var")


@pytest.mark.parametrize("name", ["nt_small", "nt_short"])
def test_importance_replays(lib, oracle, name):
    """importance_shapes.py's smallest k_imp_small case and its smallest
    screened one: the encoder with its screening pass on, and the decoder of
    the oracle's indices, in one capture."""
    import importance_shapes as IS
    case = IS.near_tie_case(name)
    tl, ts, pl, ps = case.inputs()
    wi, ws = oracle.importance_encode(tl, ts, pl, ps, case.off, case.oracle_counts, case.seed,
                                      case.base)
    nb, D = case.sizes.size, int(case.off[-1])
    d = [_dev(a) for a in (tl, ts, pl, ps)]
    off, counts, widx = _dev(case.off), _dev(case.counts), _dev(np.asarray(wi, np.int64))
    index, sample, decoded = _empty(nb, torch.int64), _empty(D, torch.float32), \
        _empty(D, torch.float32)
    ws_dev = _empty(lib.cwq_importance_workspace_size(nb, D), torch.uint8)

    def run(stream):
        from compression_without_quantization_amd import _lib
        st = stream.cuda_stream
        _ok(lib.cwq_importance_encode(*[t.data_ptr() for t in d], off.data_ptr(), counts.data_ptr(),
                                      nb, D, _wrap32(case.seed), case.base, index.data_ptr(),
                                      sample.data_ptr(), ws_dev.data_ptr(), ws_dev.numel(),
                                      _lib.options(2), st), "importance_encode")
        _ok(lib.cwq_importance_decode(widx.data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                      off.data_ptr(), nb, D, _wrap32(case.seed), case.base,
                                      decoded.data_ptr(), st), "importance_decode")

    replay_check(run, {"index": index, "sample": sample, "decoded": decoded}, [ws_dev],
                 {"index": np.asarray(wi, np.int64), "sample": ws, "decoded": ws},
                 f"cwq_importance_encode / _decode, {name}")


def test_pln_calls_replay(lib):
    """The PLN posterior (float32 in the header's order, each operation
    correctly rounded, so NumPy repeats it) and the two permutations."""
    C, HW, eps = 5, 77, np.float32(1e-12)
    n = C * HW
    rng = np.random.Generator(np.random.PCG64(12))
    ll, ls, pl, ps = _values(rng, n)
    one = np.float32(1.0)
    lp, pp = one / (ls * ls + eps), one / (ps * ps + eps)
    var = one / (lp + pp)
    want_scale, want_loc = np.sqrt(var), (ll * pp + pl * lp) * var
    assert want_loc.dtype == np.float32 and want_scale.dtype == np.float32
    perm = rng.permutation(n).astype(np.int32)
    nhwc = ll.reshape(C, HW).T.reshape(-1)  # f = hw C + c of the NCHW tensor ll
    want_gather = nhwc[perm]
    back = np.zeros(n, np.float32)          # out_nchw[c HW + hw] = src[i], perm[i] = hw C + c
    back[(perm % C) * HW + perm // C] = ls
    d = [_dev(a) for a in (ll, ls, pl, ps)]
    dperm = _dev(perm)
    loc, scale, gathered, scattered = (_empty(n, torch.float32) for _ in range(4))

    def run(stream):
        st = stream.cuda_stream
        _ok(lib.cwq_pln_posterior(*[t.data_ptr() for t in d], n, float(eps), loc.data_ptr(),
                                  scale.data_ptr(), st), "pln_posterior")
        _ok(lib.cwq_permute_gather(d[0].data_ptr(), C, HW, dperm.data_ptr(), gathered.data_ptr(),
                                   st), "permute_gather")
        _ok(lib.cwq_permute_scatter(d[1].data_ptr(), C, HW, dperm.data_ptr(),
                                    scattered.data_ptr(), st), "permute_scatter")

    replay_check(run, {"loc": loc, "scale": scale, "gathered": gathered, "scattered": scattered},
                 [], {"loc": want_loc, "scale": want_scale, "gathered": want_gather,
                      "scattered": back},
                 "cwq_pln_posterior, cwq_permute_gather, cwq_permute_scatter")
