"""CPU: the rate table's C ABI (cwq_rate_table, cwq_choose_bits, include/cwq.h
0.17): the symbols, and every refusal that happens on the host before a launch
(no GPU compute is called)."""
import math

import pytest

from compression_without_quantization_amd import _lib

INVALID, WORKSPACE = -1, -3  # CWQ_ERR_INVALID, CWQ_ERR_WORKSPACE


def test_symbols_and_version(cwqlib):
    assert _lib.ABI_VERSION >= 17 and cwqlib.cwq_version() == _lib.ABI_VERSION
    for name in ("cwq_rate_table", "cwq_choose_bits", "cwq_rate_table_workspace_bytes"):
        assert hasattr(cwqlib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["cwq_rate_table"][1]) == 18
    assert len(_lib.SIGNATURES["cwq_choose_bits"][1]) == 9


def _table(lib, B, nb=10, d=4, ws=None, block_off=None, total=None):
    need = lib.cwq_rate_table_workspace_bytes(nb, nb * d, d, max(min(B, 30), 0))
    return lib.cwq_rate_table(1, 1, 1, 1, block_off, nb, nb * d if total is None else total, d, B,
                              42, 1.0, 0, 1, 1, 1, need if ws is None else ws, None, None)


@pytest.mark.parametrize("B", [-1, 31])
def test_max_bits_outside_0_30_is_refused(cwqlib, B):
    assert _table(cwqlib, B) == INVALID and b"max_bits" in cwqlib.cwq_last_error()


def test_short_workspace_is_refused(cwqlib):
    for B in (0, 11, 12, 30):
        need = cwqlib.cwq_rate_table_workspace_bytes(10, 40, 4, B)
        assert need >= 10 * 12 * 8 + 10 * max(B - 11, 0) * 8 + 4 * 40
        assert _table(cwqlib, B, ws=need - 1) == WORKSPACE
    assert cwqlib.cwq_rate_table(1, 1, 1, 1, None, 10, 40, 4, 8, 42, 1.0, 0, 1, 1, None, 1 << 30,
                                 None, None) == WORKSPACE


def test_uniform_blocks_must_fill_total_dims(cwqlib):
    assert _table(cwqlib, 8, total=41) == INVALID and b"total_dims" in cwqlib.cwq_last_error()


def test_null_outputs_and_bad_options_are_refused(cwqlib):
    need = cwqlib.cwq_rate_table_workspace_bytes(10, 40, 4, 8)
    assert cwqlib.cwq_rate_table(1, 1, 1, 1, None, 10, 40, 4, 8, 42, 1.0, 0, None, 1, 1, need,
                                 None, None) == INVALID
    assert cwqlib.cwq_rate_table(None, 1, 1, 1, None, 10, 40, 4, 8, 42, 1.0, 0, 1, 1, 1, need,
                                 None, None) == INVALID
    bad = _lib.options(prune_mode=3)
    assert cwqlib.cwq_rate_table(1, 1, 1, 1, None, 10, 40, 4, 8, 42, 1.0, 0, 1, 1, 1, need, bad,
                                 None) == INVALID and b"prune_mode" in cwqlib.cwq_last_error()


def test_no_block_is_no_launch(cwqlib):
    assert cwqlib.cwq_rate_table(None, None, None, None, None, 0, 0, 0, 16, 42, 1.0, 0, None, None,
                                 None, 0, None, None) == 0
    assert cwqlib.cwq_choose_bits(None, 0, 8, 0.5, 0, 8, None, None, None) == 0


def test_python_wants_exactly_one_of_block_dim_and_block_off():
    import numpy as np
    from compression_without_quantization_amd import encode_blocks_rate, rate_table
    x = np.ones(8, np.float32)
    for kw in (dict(), dict(block_dim=4, block_off=[0, 4, 8])):
        with pytest.raises(ValueError, match="exactly one of block_dim / block_off"):
            rate_table(x, x, x, x, 4, 1, **kw)
    for kw in (dict(), dict(lam=0.5, total_bits=8)):
        with pytest.raises(ValueError, match="exactly one of lam / total_bits"):
            encode_blocks_rate(x, x, x, x, 1, 4, block_dim=4, **kw)


@pytest.mark.parametrize("lam", [-1e-300, -1.0, math.nan, math.inf])
def test_choose_bits_refuses_a_bad_lam(cwqlib, lam):
    assert cwqlib.cwq_choose_bits(1, 4, 8, lam, 0, 8, 1, None, None) == INVALID
    assert b"lam" in cwqlib.cwq_last_error()


def test_choose_bits_refuses_bad_ranges(cwqlib):
    assert cwqlib.cwq_choose_bits(1, 4, 8, 0.5, 5, 4, 1, None, None) == INVALID  # min > max
    assert b"min_bits" in cwqlib.cwq_last_error()
    assert cwqlib.cwq_choose_bits(1, 4, 8, 0.5, 9, 30, 1, None, None) == INVALID  # min > B
    assert cwqlib.cwq_choose_bits(1, 4, 8, 0.5, -1, 8, 1, None, None) == INVALID
    assert cwqlib.cwq_choose_bits(1, 4, 31, 0.5, 0, 8, 1, None, None) == INVALID
    assert cwqlib.cwq_choose_bits(1, 4, -1, 0.5, 0, 8, 1, None, None) == INVALID
    assert cwqlib.cwq_choose_bits(None, 4, 8, 0.5, 0, 8, 1, None, None) == INVALID
    assert cwqlib.cwq_choose_bits(1, -1, 8, 0.5, 0, 8, 1, None, None) == INVALID
