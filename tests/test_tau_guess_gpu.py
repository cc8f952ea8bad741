"""GPU: k_encode_prune's screening pass started from a guessed threshold.

With the tau guess on, a tile's threshold starts at the lower bound of a row at
the level q_m that csrc/cwq_tau_guess.h predicts m of its candidates to fall
below; after the pass the kernel checks that a real row passed the guess and
otherwise runs the tile again without it.  None of that may change a result.
cwq_selftest_encode_uniform_tau_guess picks the mode: 0 off, 1 on, 2 every
screened tile's guess replaced by FLT_MAX, so that every tile takes the retry
(no counter is read here: mode 2 forces the retry by construction).

Shapes and inputs are those of tests/test_prune_tau_gpu.py
(tests/prune_tau_shapes.py), and so are the CPU oracle's blocks, computed once
for both files.
"""
import numpy as np
import pytest
import torch

import prune_tau_shapes as P
from test_prune_tau_gpu import BASE, SEED, _check_oracle, _inputs, _oracle, _same

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    return C


def _encode(cwqlib, shape, host, guess_mode, workspace=None):
    """cwq_selftest_encode_uniform_tau_guess at prune_mode 2: (indices, sample words)."""
    from compression_without_quantization_amd import _lib
    d, bits, nb, n_steps = shape
    tl, ts, pl, ps = (torch.from_numpy(a).cuda() for a in host)
    idx = torch.empty((nb, n_steps), dtype=torch.int32, device="cuda")
    sample = torch.empty(nb * d, dtype=torch.float32, device="cuda")
    need = int(cwqlib.cwq_greedy_encode_uniform_workspace_size(nb, d))
    ws = workspace if workspace is not None else \
        torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    assert ws.numel() >= need
    rc = cwqlib.cwq_selftest_encode_uniform_tau_guess(
        tl.data_ptr(), ts.data_ptr(), pl.data_ptr(), ps.data_ptr(), nb, d, bits, n_steps, SEED,
        1.0, BASE, idx.data_ptr(), sample.data_ptr(), ws.data_ptr(), ws.numel(),
        _lib.options(2, None), torch.cuda.current_stream().cuda_stream, guess_mode)
    _lib.check(rc, "cwq_selftest_encode_uniform_tau_guess")
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.int64), sample.cpu().numpy().view(np.uint32).copy()


def _three_modes(cwqlib, shape, kind="normal"):
    host = _inputs(shape, kind)
    out = [_encode(cwqlib, shape, host, g) for g in MODES]
    _same(out[1], out[0], f"{shape} {kind}: guess on against off")
    _same(out[2], out[0], f"{shape} {kind}: every tile retried against off")
    return out


@pytest.mark.parametrize("shape", P.MODES_CASES, ids=lambda s: "d%d_b%d_nb%d_s%d" % s)
def test_modes_agree_and_match_oracle(cwq, cwqlib, oracle, shape):
    """Tiles of 2^4, 2^8 (no guess: m / N > 2^-9) and 2^12 candidates at d in
    {8, 32, 64}, the workload's own tile, two steps, and INTER tiles (2 and
    4,096 per block; the later ones start from keys[g])."""
    out = _three_modes(cwqlib, shape)
    _check_oracle(out[1], shape, f"{shape}: guess on")


@pytest.mark.parametrize("kind", ["tied_zero_scale", "tied_wide_target"])
@pytest.mark.parametrize("shape", P.TIED, ids=lambda s: "d%d_b%d" % s[:2])
def test_all_rows_tied(cwq, cwqlib, shape, kind):
    """Every candidate has the same value: index 0 in every mode.  Zero
    proposal scale gives no guess (sum w = 0); the wide target gives one that
    every row passes or none does."""
    for idx, _ in _three_modes(cwqlib, shape, kind):
        assert (idx == 0).all(), f"{shape} {kind}: {idx.reshape(-1)}"


def test_nan_block(cwq, cwqlib, oracle):
    """A block whose rows are all NaN: as with the guess off (index 0); the
    other blocks are the oracle's."""
    shape = P.NAN_BLOCK
    d = shape[0]
    out = _three_modes(cwqlib, shape, "nan_block")
    _, want_i, want_w = _oracle(shape)
    for idx, words in out:
        assert (idx[1] == 0).all()
        for g in (0, 2):
            assert np.array_equal(idx[g], want_i[g])
            assert np.array_equal(words[g * d:(g + 1) * d], want_w[g])


def test_retry_then_guess_on_one_workspace(cwq, cwqlib, oracle):
    """Mode 2, then mode 1, back to back on one workspace filled with 0xA5 that
    nothing clears: the retry resets what it reads, and leaves nothing behind
    that the next call reads."""
    need = max(int(cwqlib.cwq_greedy_encode_uniform_workspace_size(nb, d))
               for d, _, nb, _ in P.WORKSPACE)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    for shape in P.WORKSPACE:
        for g in (2, 1):
            got = _encode(cwqlib, shape, _inputs(shape), g, workspace=ws)
            _check_oracle(got, shape, f"{shape} guess mode {g} on a used workspace")


def test_mode_is_validated(cwq, cwqlib):
    shape = P.WORKSPACE[0]
    from compression_without_quantization_amd import _lib
    for bad in (-1, 3):
        with pytest.raises(Exception):
            _encode(cwqlib, shape, _inputs(shape), bad)
    assert _lib.ABI_VERSION >= 14
