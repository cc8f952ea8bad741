"""CPU: the C ABI of budgets under a total (cwq_choose_bits_total,
cwq_greedy_encode_rate, include/cwq.h 0.18): the symbols, and every refusal that
happens on the host before a launch (no GPU compute is called)."""
import pytest

from compression_without_quantization_amd import _lib

INVALID, WORKSPACE = -1, -3  # CWQ_ERR_INVALID, CWQ_ERR_WORKSPACE
NAMES = ("cwq_choose_bits_total", "cwq_choose_bits_total_workspace_bytes",
         "cwq_greedy_encode_rate", "cwq_greedy_encode_rate_workspace_bytes")


def test_symbols_and_version(cwqlib):
    assert _lib.ABI_VERSION >= 18 and cwqlib.cwq_version() == _lib.ABI_VERSION
    for name in NAMES:
        assert hasattr(cwqlib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["cwq_choose_bits_total"][1]) == 12
    assert len(_lib.SIGNATURES["cwq_greedy_encode_rate"][1]) == 24
    # the existing calls keep their argument lists
    assert len(_lib.SIGNATURES["cwq_choose_bits"][1]) == 9
    assert len(_lib.SIGNATURES["cwq_rate_table"][1]) == 18


def test_python_exports():
    import compression_without_quantization_amd as C
    for name in ("choose_bits_total_device", "encode_blocks_rate_total",
                 "code_grouped_greedy_sample_rate"):
        assert callable(getattr(C, name)) and name in C.__all__


def _solve(lib, nb=4, B=8, total=16, lo=0, hi=8, value=1, bits=1, lam=1, tot=1, ws=1, ws_bytes=None):
    need = lib.cwq_choose_bits_total_workspace_bytes(max(min(B, 30), 0))
    return lib.cwq_choose_bits_total(value, nb, B, total, lo, hi, bits, lam, tot, ws,
                                     need if ws_bytes is None else ws_bytes, None)


def test_solver_refuses_bad_ranges_as_choose_bits_does(cwqlib):
    assert _solve(cwqlib, lo=5, hi=4) == INVALID and b"min_bits" in cwqlib.cwq_last_error()
    assert _solve(cwqlib, lo=9, hi=30, total=100) == INVALID  # min > B
    assert b"min_bits" in cwqlib.cwq_last_error()
    assert _solve(cwqlib, lo=-1) == INVALID and b"min_bits" in cwqlib.cwq_last_error()
    assert _solve(cwqlib, B=31) == INVALID and b"max_bits_table" in cwqlib.cwq_last_error()
    assert _solve(cwqlib, B=-1) == INVALID and b"max_bits_table" in cwqlib.cwq_last_error()
    assert _solve(cwqlib, nb=-1) == INVALID and b"nb" in cwqlib.cwq_last_error()
    for null in ("value", "bits", "lam", "tot"):
        assert _solve(cwqlib, **{null: None}) == INVALID, null
        assert b"null" in cwqlib.cwq_last_error()


def test_solver_refuses_a_total_below_min_bits_everywhere(cwqlib):
    assert _solve(cwqlib, nb=4, lo=3, total=11) == INVALID
    assert b"total_bits" in cwqlib.cwq_last_error()
    assert _solve(cwqlib, nb=4, lo=0, total=-1) == INVALID and b"total_bits" in cwqlib.cwq_last_error()
    assert _solve(cwqlib, nb=1 << 62, lo=30, hi=30, B=30, total=1 << 62) == INVALID
    assert b"total_bits" in cwqlib.cwq_last_error()


def test_solver_refuses_a_short_workspace(cwqlib):
    for B in (0, 8, 30):
        need = cwqlib.cwq_choose_bits_total_workspace_bytes(B)
        assert need >= 40 + 8 * 8 * (B + 1) + 8 * 8  # the state, a tree of >= 8 slots, its totals
        assert _solve(cwqlib, B=B, hi=B, ws_bytes=need - 1) == WORKSPACE
    assert _solve(cwqlib, ws=None, ws_bytes=1 << 20) == WORKSPACE


def test_no_block_is_no_launch(cwqlib):
    assert cwqlib.cwq_choose_bits_total(None, 0, 8, 0, 0, 8, None, None, None, None, 0, None) == 0
    assert cwqlib.cwq_greedy_encode_rate(None, None, None, None, None, 0, 0, 0, 16, 0, 0, 42, 1.0,
                                         0, None, None, None, None, None, None, None, 0, None,
                                         None) == 0


def _encode(lib, nb=10, d=4, B=8, total=40, lo=0, ws=1, ws_bytes=None, total_dims=None, idx=1,
            sample=1, bits=1, lam=1, tot=1, t_loc=1, opts=None):
    need = lib.cwq_greedy_encode_rate_workspace_bytes(nb, nb * d, d, max(min(B, 30), 0))
    return lib.cwq_greedy_encode_rate(t_loc, 1, 1, 1, None, nb, nb * d if total_dims is None
                                      else total_dims, d, B, total, lo, 42, 1.0, 0, idx, sample,
                                      bits, lam, tot, None, ws,
                                      need if ws_bytes is None else ws_bytes, opts, None)


def test_encode_rate_refusals(cwqlib):
    for B in (-1, 31):
        assert _encode(cwqlib, B=B) == INVALID and b"max_bits" in cwqlib.cwq_last_error()
    assert _encode(cwqlib, lo=9) == INVALID and b"min_bits" in cwqlib.cwq_last_error()
    assert _encode(cwqlib, lo=-1) == INVALID and b"min_bits" in cwqlib.cwq_last_error()
    assert _encode(cwqlib, lo=5, total=49) == INVALID and b"total_bits" in cwqlib.cwq_last_error()
    assert _encode(cwqlib, total_dims=41) == INVALID and b"total_dims" in cwqlib.cwq_last_error()
    for null in ("idx", "sample", "bits", "lam", "tot", "t_loc"):
        assert _encode(cwqlib, **{null: None}) == INVALID, null
    bad = _lib.options(prune_mode=3)
    assert _encode(cwqlib, opts=bad) == INVALID and b"prune_mode" in cwqlib.cwq_last_error()
    for B in (0, 11, 12, 30):
        need = cwqlib.cwq_greedy_encode_rate_workspace_bytes(10, 40, 4, B)
        table = cwqlib.cwq_rate_table_workspace_bytes(10, 40, 4, B)
        assert need >= table + 8 * 10 * (B + 1) + cwqlib.cwq_choose_bits_total_workspace_bytes(B)
        assert _encode(cwqlib, B=B, ws_bytes=need - 1) == WORKSPACE
    assert _encode(cwqlib, ws=None, ws_bytes=1 << 30) == WORKSPACE


def test_python_wants_exactly_one_of_block_dim_and_block_off():
    """(The wrappers' ValueError for a total below min_bits everywhere needs a
    device tensor: tests/test_rate_total_gpu.py.)"""
    import numpy as np
    from compression_without_quantization_amd import encode_blocks_rate_total
    x = np.ones(8, np.float32)
    for kw in (dict(), dict(block_dim=4, block_off=[0, 4, 8])):
        with pytest.raises(ValueError, match="exactly one of block_dim / block_off"):
            encode_blocks_rate_total(x, x, x, x, 1, 4, 8, **kw)
