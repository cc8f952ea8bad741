"""GPU: every scoring path of the greedy family against the CPU references on
near-tie inputs, bit for bit: int32 indices, uint32 views of samples and values.

The inputs are tests/near_ties.py's family on the cases of
tests/encode_shapes.py (NEAR_TIE_CASES): targets so wide that a block's best
rows differ by a rounding or not at all.  tests/test_near_ties.py certifies on
the CPU, from the oracle alone and with the seed, block_id_base and rho used
here, that on each case every applicable neighbouring arithmetic (the row sum
in the sse4, avx8x2, avx512, seq or tree order, log sigma one ulp up or down)
changes the index row of at least 4 of the first 64 blocks, that at least 4
exact ties are won by an index other than 0, and that the winners are spread
over the index range.  So, for each case, swapping the reference for any
applicable variant's index table makes the comparison below fail: a kernel
that sums in another order, folds the d % 8 tail elsewhere, takes another log
sigma or breaks ties another way cannot pass.  tests/test_encode_plan.py checks
that each case takes the path it names.

The coder's seed is 2^31 - 4 with block_id_base 5, so the block seeds wrap;
rho is 0.8 on the multi-step cases.  References: oracle.greedy_encode for the
encoders and for a beam of 1, tests/beam_reference.py for a beam of 4,
tests/backfit_reference.py for backfitting.
"""
import functools

import numpy as np
import pytest
import torch

import backfit_reference as B
import beam_reference as R
import encode_shapes as S
import near_ties as NT

pytestmark = pytest.mark.gpu

SEED, BASE = NT.SEED, NT.BASE
GROUPS = {}
for _name, _c in S.NEAR_TIE_CASES.items():
    GROUPS.setdefault(_c["group"], []).append(_name)


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
    """The case with its inputs on the host and on the device."""
    c = dict(S.NEAR_TIE_CASES[name], name=name)
    c["off"] = NT.offsets(c["sizes"])
    c["nb"], c["D"] = len(c["sizes"]), int(c["off"][-1])
    c["rho"] = 0.8 if c["n_steps"] > 1 else 1.0
    c["host"] = NT.inputs(c["off"], c["input_seed"], c["level"])
    c["dev"] = tuple(torch.from_numpy(a).cuda() for a in c["host"])
    c["layout"] = dict(block_dim=c["d"]) if c["d"] is not None else dict(block_off=c["off"])
    c["kw"] = dict(rho=c["rho"], block_id_base=BASE, **c["layout"])
    if np.ndim(c["bits"]):
        c["bits"] = np.asarray(c["bits"], np.int32)
    assert SEED + BASE + c["nb"] > 2147483647 and BASE != 0
    return c


@functools.lru_cache(maxsize=None)
def _declared(name):
    """(blocks checked, idx, sample) from oracle.greedy_encode, once per case:
    every block, or every ``oracle_stride``-th one, the last and the first 64
    (the blocks the certificate covers)."""
    c = _case(name)
    blocks = None
    if "oracle_stride" in c:
        blocks = np.unique(np.concatenate([np.arange(0, c["nb"], c["oracle_stride"]),
                                           np.arange(NT.certified_blocks(c["off"])),
                                           [c["nb"] - 1]]))
    idx, sample = NT.declared(c["host"], c["off"], c["bits"], c["n_steps"], SEED, c["rho"], BASE,
                              blocks)
    return (np.arange(c["nb"]) if blocks is None else blocks), idx, sample


def _dims(c, blocks):
    off = c["off"]
    return np.concatenate([np.arange(off[g], off[g + 1]) for g in blocks] +
                          [np.zeros(0, np.int64)]).astype(np.int64)


def _check_encoder(name, got, what):
    """got = (idx, sample) of an encoder against the oracle."""
    c = _case(name)
    blocks, want_idx, want_sample = _declared(name)
    idx, words = _i32(got[0]), _u32(got[1])
    assert idx.shape == (c["nb"], c["n_steps"]) and words.shape == (c["D"],)
    bad = blocks[(idx[blocks] != want_idx[blocks]).any(axis=1)]
    assert bad.size == 0, (f"{name} {what}: {bad.size} of {blocks.size} blocks differ, first "
                           f"{bad[:8]}: {idx[bad[:8]].tolist()} != {want_idx[bad[:8]].tolist()}")
    dims = _dims(c, blocks)
    assert np.array_equal(words[dims], _u32(want_sample)[dims]), f"{name} {what}: sample"
    empty = np.flatnonzero(np.diff(c["off"]) == 0)
    assert (idx[empty] == 0).all(), f"{name} {what}: empty blocks"
    assert idx.min() >= 0 and (idx < (1 << np.asarray(c["bits"], np.int64).reshape(-1, 1))).all()


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what


# ---------------------------------------------------------------------------
# encode_blocks: the exact kernel, k_encode_prune (also its tile queue), the
# general pruned kernel on uniform and ragged blocks, the small-candidate paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GROUPS["encode"])
def test_encode_blocks(cwq, oracle, name):
    c = _case(name)
    for prune in c["prune"]:
        got = cwq.encode_blocks(*c["dev"], c["bits"], c["n_steps"], SEED, prune_mode=prune,
                                **c["kw"])
        _check_encoder(name, got, f"prune_mode {prune}")
    if "oracle_stride" in c:  # every block, against the exact kernel
        ref = cwq.encode_blocks(*c["dev"], c["bits"], c["n_steps"], SEED, prune_mode=0, **c["kw"])
        _check_encoder(name, ref, "prune_mode 0")
        _same_bits(got, ref, f"{name}: the whole against the exact kernel")


@pytest.mark.parametrize("name", GROUPS["tau_guess"])
def test_tau_guess_modes(cwq, cwqlib, oracle, name):
    """k_encode_prune started from a guessed threshold: off, on, and every
    screened tile retried (cwq_selftest_encode_uniform_tau_guess)."""
    from compression_without_quantization_amd import _lib
    c = _case(name)
    tl, ts, pl, ps = c["dev"]
    need = int(cwqlib.cwq_greedy_encode_uniform_workspace_size(c["nb"], c["d"]))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    for mode in c["guess"]:
        idx = torch.full((c["nb"], c["n_steps"]), -77, dtype=torch.int32, device="cuda")
        sample = torch.full((c["D"],), float("nan"), dtype=torch.float32, device="cuda")
        rc = cwqlib.cwq_selftest_encode_uniform_tau_guess(
            tl.data_ptr(), ts.data_ptr(), pl.data_ptr(), ps.data_ptr(), c["nb"], c["d"],
            c["bits"], c["n_steps"], SEED, c["rho"], BASE, idx.data_ptr(), sample.data_ptr(),
            ws.data_ptr(), ws.numel(), _lib.options(2, None),
            torch.cuda.current_stream().cuda_stream, mode)
        _lib.check(rc, "cwq_selftest_encode_uniform_tau_guess")
        torch.cuda.synchronize()
        _check_encoder(name, (idx, sample), f"guess mode {mode}")


# ---------------------------------------------------------------------------
# k_encode_rows_wave, every block forced onto it
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GROUPS["rows_wave"])
def test_rows_wave(cwq, cwqlib, oracle, name):
    from test_rows_wave_gpu import _rows_wave
    c = _case(name)
    idx, sample, _keep = _rows_wave(cwqlib, *c["host"], c["off"], c["bits"], c["n_steps"], SEED,
                                    c["rho"], BASE)
    torch.cuda.synchronize()
    _check_encoder(name, (idx, sample), "forced wave per row")


# ---------------------------------------------------------------------------
# encode_blocks_var: block g against the oracle at n_bits[g]
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GROUPS["var"])
def test_encode_blocks_var(cwq, oracle, name):
    c = _case(name)
    runs = {}
    for prune in (None, 0):
        runs[prune] = cwq.encode_blocks_var(*c["dev"], c["bits"], c["n_steps"], SEED,
                                            prune_mode=prune, **c["kw"])
        _check_encoder(name, runs[prune], f"prune_mode {prune}")
    assert (_i32(runs[None][0])[c["bits"] == 0] == 0).all()


# ---------------------------------------------------------------------------
# the beam encoder
# ---------------------------------------------------------------------------
def _values_of(oracle, c, sample, blocks=None):
    """The value a block's key holds for ``sample``: tests/beam_reference.py's
    log-density, Eigen row sum and keyed value; +0 for an empty block."""
    tl, ts = c["host"][:2]
    out = np.zeros(c["nb"], np.float32)
    for g in (range(c["nb"]) if blocks is None else blocks):
        sl = slice(int(c["off"][g]), int(c["off"][g + 1]))
        if sl.stop > sl.start:
            with np.errstate(all="ignore"):
                z = (sample[sl] - tl[sl]) / ts[sl]
                lp = (np.float32(-0.5) * (z * z)) - R.lognorms(oracle, ts[sl])
                out[g] = R.keyed_values(R.eigen_rowsums(lp[None, :]))[0]
    return out


def _check_beam_one(oracle, name, got, what):
    c = _case(name)
    _check_encoder(name, got[:2], what)
    want = _values_of(oracle, c, _declared(name)[2])
    assert np.array_equal(_u32(got[2]), _u32(want)), \
        f"{name} {what}: values differ at {np.flatnonzero(_u32(got[2]) != _u32(want))[:8]}"


def _check_beam(got, want, what):
    assert np.array_equal(_i32(got[0]), want[0]), \
        f"{what}: blocks {np.flatnonzero((_i32(got[0]) != want[0]).any(axis=1))[:8]}"
    assert np.array_equal(_u32(got[1]), _u32(want[1])), f"{what}: sample"
    assert np.array_equal(_u32(got[2]), _u32(want[2])), f"{what}: value"


@pytest.mark.parametrize("name", GROUPS["beam"])
def test_beam(cwq, oracle, name):
    """A beam of 1 is the greedy coder, on the plan's kernel and on each of
    cwq_selftest_beam_encode's paths (a lane per row, a wave per row, both with
    quarter tiles); a beam of 4 against the restatement."""
    c = _case(name)
    for path in (None, 0, 1, 2, 3):
        got = cwq.encode_blocks_beam(*c["dev"], c["bits"], c["n_steps"], SEED, 1,
                                     return_value=True, _path=path, **c["kw"])
        _check_beam_one(oracle, name, got, f"beam 1, path {path}")
    want = R.beam_encode(oracle, *c["host"], c["off"], c["bits"], c["n_steps"], SEED, 4, c["rho"],
                         BASE)
    assert not np.array_equal(want[0], _declared(name)[1])  # the beam finds another code
    for path in (None, 1):
        got = cwq.encode_blocks_beam(*c["dev"], c["bits"], c["n_steps"], SEED, 4,
                                     return_value=True, _path=path, **c["kw"])
        _check_beam(got, want, f"{name}: beam 4, path {path}")


@pytest.mark.parametrize("name", GROUPS["beam_var"])
def test_beam_var(cwq, oracle, name):
    import beam_var_reference as RV
    c = _case(name)
    got = cwq.encode_blocks_var_beam(*c["dev"], c["bits"], c["n_steps"], SEED, 1,
                                     return_value=True, **c["kw"])
    _check_beam_one(oracle, name, got, "encode_blocks_var_beam, beam 1")
    want = RV.beam_encode_var(oracle, *c["host"], c["off"], c["bits"], c["n_steps"], SEED, 4,
                              c["rho"], BASE)
    got = cwq.encode_blocks_var_beam(*c["dev"], c["bits"], c["n_steps"], SEED, 4,
                                     return_value=True, **c["kw"])
    _check_beam(got, want, f"{name}: encode_blocks_var_beam, beam 4")


# ---------------------------------------------------------------------------
# backfitting, from the oracle's greedy table
# ---------------------------------------------------------------------------
def _backfit_reference(oracle, c, table, sweeps, blocks):
    """tests/backfit_reference.py per budget on ``blocks``: (idx, sample,
    values [nb, sweeps + 1], accepted)."""
    bits = np.broadcast_to(np.asarray(c["bits"], np.int64), (c["nb"],))
    idx = np.zeros((c["nb"], c["n_steps"]), np.int32)
    sample = np.zeros(c["D"], np.float32)
    values = np.zeros((c["nb"], sweeps + 1), np.float32)
    accepted = np.zeros(c["nb"], np.int32)
    for b in sorted(set(bits[blocks].tolist())):
        rows = [int(g) for g in blocks if bits[g] == b]
        i, s, v, a, _ = B.backfit(oracle, table, *c["host"], c["off"], int(b), c["n_steps"], SEED,
                                  sweeps, c["rho"], BASE, rows)
        idx[rows], values[rows], accepted[rows] = i[rows], v[rows], a[rows]
        dims = _dims(c, rows)
        sample[dims] = s[dims]
    return idx, sample, values, accepted


def _check_backfit(c, got, want, blocks, what):
    gi, gs, gv, ga = _i32(got[0]), _u32(got[1]), _u32(got[2]), _i32(got[3])
    bad = blocks[(gi[blocks] != want[0][blocks]).any(axis=1)]
    assert bad.size == 0, f"{what}: indices of blocks {bad[:8]}"
    dims = _dims(c, blocks)
    assert np.array_equal(gs[dims], _u32(want[1])[dims]), f"{what}: sample"
    wv = _u32(want[2][:, -1])
    assert np.array_equal(gv[blocks], wv[blocks]), \
        f"{what}: values of blocks {blocks[gv[blocks] != wv[blocks]][:8]}"
    assert np.array_equal(ga[blocks], want[3][blocks]), \
        f"{what}: accepted counts of blocks {blocks[ga[blocks] != want[3][blocks]][:8]}"


@pytest.mark.parametrize("name,sweeps", [(n, 1 if n == "backfit_short" else 2)
                                         for n in GROUPS["backfit"] + GROUPS["backfit_var"]])
def test_backfit(cwq, oracle, name, sweeps):
    """One sweep on a greedy table; a wave per block on ragged blocks; a lane
    per block (the restatement on every ``ref_stride``-th block); under
    budgets.  The table is the oracle's."""
    c = _case(name)
    table = NT.declared(c["host"], c["off"], c["bits"], c["n_steps"], SEED, c["rho"], BASE)[0]
    blocks = np.unique(np.concatenate([np.arange(0, c["nb"], c.get("ref_stride", 1)),
                                       [c["nb"] - 1]]))
    want = _backfit_reference(oracle, c, table, sweeps, blocks)
    assert want[3][blocks].sum() > 0  # some replacement is accepted
    call = cwq.backfit_blocks_var if c["group"] == "backfit_var" else cwq.backfit_blocks
    runs = [call(table, *c["dev"], c["bits"], c["n_steps"], SEED, sweeps, return_value=True,
                 return_accepted=True, prune_mode=m, **c["kw"]) for m in (None, 0)]
    for got, m in zip(runs, (None, 0)):
        _check_backfit(c, got, want, blocks, f"{name}: prune_mode {m}")
    _same_bits(runs[0], runs[1], f"{name}: every block, prune_mode 0 against the default")
    # the table itself: the encoder's, and sweeps=0 returns it with its value
    start = call(table, *c["dev"], c["bits"], c["n_steps"], SEED, 0, return_value=True,
                 return_accepted=True, **c["kw"])
    assert np.array_equal(_i32(start[0]), table) and not _i32(start[3]).any()
    assert np.array_equal(_u32(start[2])[blocks], _u32(want[2][:, 0])[blocks])
    assert (runs[0][2] >= start[2]).all()
