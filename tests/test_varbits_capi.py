"""CPU: the per-block bit budget entry points of libcwq.so (ABI 0.8) are
exported and bound, and their host-side validation runs before any HIP call
(no device work is started here)."""
import pytest

from compression_without_quantization_amd import _lib

NEW = ["cwq_block_bits", "cwq_greedy_encode_uniform_var_workspace_size",
       "cwq_greedy_encode_uniform_var", "cwq_pack_indices_var_workspace_size",
       "cwq_pack_indices_var", "cwq_unpack_indices_var"]


def test_symbols_exported_and_bound(cwqlib):
    for name in NEW:
        assert hasattr(cwqlib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION >= 8 and cwqlib.cwq_version() == _lib.ABI_VERSION
    import compression_without_quantization_amd as C
    for name in ("block_bits", "encode_blocks_var", "decode_blocks_var", "pack_indices",
                 "unpack_indices"):
        assert name in C.__all__ and callable(getattr(C, name))


def _poison(cwqlib):
    """Leave a message behind, so that a later success is seen to clear it."""
    assert cwqlib.cwq_block_bits(None, None, None, None, -1, 4, 0.0, 0, 30, None, None,
                                 None) == -1
    assert cwqlib.cwq_last_error() != b""


def test_empty_calls_succeed_and_clear_the_error(cwqlib):
    calls = [
        lambda: cwqlib.cwq_block_bits(None, None, None, None, 0, 32, 1.44, 0, 30, None, None,
                                      None),
        lambda: cwqlib.cwq_greedy_encode_uniform_var(None, None, None, None, 0, 32, None, 1, 42,
                                                     1.0, 0, None, None, None, 0, None, None),
        lambda: cwqlib.cwq_pack_indices_var(None, None, 0, 1, None, 0, None, None, 0, None),
        lambda: cwqlib.cwq_unpack_indices_var(None, 0, None, 0, 1, None, None, 0, None),
    ]
    for call in calls:
        _poison(cwqlib)
        assert call() == 0
        assert cwqlib.cwq_last_error() == b""


def test_bad_arguments_refused_before_any_launch(cwqlib):
    enc = cwqlib.cwq_greedy_encode_uniform_var
    need = cwqlib.cwq_greedy_encode_uniform_var_workspace_size(10, 4)
    # negative sizes
    assert enc(1, 1, 1, 1, -1, 4, 1, 1, 42, 1.0, 0, 1, 1, 1, need, None, None) == -1
    assert enc(1, 1, 1, 1, 10, -4, 1, 1, 42, 1.0, 0, 1, 1, 1, need, None, None) == -1
    assert enc(1, 1, 1, 1, 10, 4, 1, 0, 42, 1.0, 0, 1, 1, 1, need, None, None) == -1
    assert b"n_steps" in cwqlib.cwq_last_error()
    assert enc(1, 1, 1, 1, 1 << 31, 4, 1, 1, 42, 1.0, 0, 1, 1, 1, need, None, None) == -1
    # null pointers: n_bits, out_idx, an input, the sample
    assert enc(1, 1, 1, 1, 10, 4, None, 1, 42, 1.0, 0, 1, 1, 1, need, None, None) == -1
    assert enc(1, 1, 1, 1, 10, 4, 1, 1, 42, 1.0, 0, None, 1, 1, need, None, None) == -1
    assert enc(1, None, 1, 1, 10, 4, 1, 1, 42, 1.0, 0, 1, 1, 1, need, None, None) == -1
    assert enc(1, 1, 1, 1, 10, 4, 1, 1, 42, 1.0, 0, 1, None, 1, need, None, None) == -1
    # options are validated as in the plain call
    assert enc(1, 1, 1, 1, 10, 4, 1, 1, 42, 1.0, 0, 1, 1, 1, need, _lib.options(prune_mode=3),
               None) == -1
    assert b"cwq_options" in cwqlib.cwq_last_error()
    # a workspace one byte short, or absent
    assert enc(1, 1, 1, 1, 10, 4, 1, 1, 42, 1.0, 0, 1, 1, 1, need - 1, None, None) == -3
    assert b"workspace" in cwqlib.cwq_last_error()
    assert enc(1, 1, 1, 1, 10, 4, 1, 1, 42, 1.0, 0, 1, 1, None, need, None, None) == -3
    # more steps than the sorted inputs can stage need the tail on top
    assert enc(1, 1, 1, 1, 10, 4, 1, 17, 42, 1.0, 0, 1, 1, 1, need, None, None) == -3

    bb = cwqlib.cwq_block_bits
    assert bb(1, 1, 1, 1, -1, 4, 0.0, 0, 30, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 10, -4, 0.0, 0, 30, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 10, 4, 0.0, 0, 31, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 10, 4, 0.0, -1, 30, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 10, 4, 0.0, 9, 8, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 10, 4, float("nan"), 0, 30, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 10, 4, 0.0, 0, 30, None, None, None) == -1
    assert bb(None, 1, 1, 1, 10, 4, 0.0, 0, 30, 1, None, None) == -1

    pack, unpack = cwqlib.cwq_pack_indices_var, cwqlib.cwq_unpack_indices_var
    pneed = cwqlib.cwq_pack_indices_var_workspace_size(10)
    assert pack(1, 1, -1, 1, 1, 8, 1, 1, pneed, None) == -1
    assert pack(1, 1, 10, 0, 1, 8, 1, 1, pneed, None) == -1
    assert pack(1, 1, 10, 1, 1, -8, 1, 1, pneed, None) == -1
    assert pack(None, 1, 10, 1, 1, 8, 1, 1, pneed, None) == -1
    assert pack(1, None, 10, 1, 1, 8, 1, 1, pneed, None) == -1
    assert pack(1, 1, 10, 1, None, 8, 1, 1, pneed, None) == -1
    assert pack(1, 1, 10, 1, 1, 8, None, 1, pneed, None) == -1
    assert pack(1, 1, 10, 1, 1, 8, 1, 1, pneed - 1, None) == -3
    assert unpack(1, -1, 1, 10, 1, 1, 1, pneed, None) == -1
    assert unpack(1, 8, 1, -1, 1, 1, 1, pneed, None) == -1
    assert unpack(1, 8, 1, 10, 0, 1, 1, pneed, None) == -1
    assert unpack(None, 8, 1, 10, 1, 1, 1, pneed, None) == -1
    assert unpack(1, 8, None, 10, 1, 1, 1, pneed, None) == -1
    assert unpack(1, 8, 1, 10, 1, None, 1, pneed, None) == -1
    assert unpack(1, 8, 1, 10, 1, 1, 1, pneed - 1, None) == -3


@pytest.mark.parametrize("d", [32, 12, 7])
def test_workspace_sizes(cwqlib, d):
    var = cwqlib.cwq_greedy_encode_uniform_var_workspace_size
    uni = cwqlib.cwq_greedy_encode_uniform_workspace_size
    pack = cwqlib.cwq_pack_indices_var_workspace_size
    sizes = [0, 1, 2, 63, 64, 2047, 2048, 2049, 20011, 1000000]
    v = [var(nb, d) for nb in sizes]
    p = [pack(nb) for nb in sizes]
    assert v == sorted(v) and p == sorted(p)  # monotone in nb
    assert v[-1] > v[0] and p[-1] > p[0]
    for nb, size in zip(sizes, v):
        # the sorted copies of the four inputs on top of one encoder workspace
        assert size >= uni(nb, d) + 16 * nb * d
    for nb, size in zip(sizes, p):
        assert size >= 8 * (nb + 1)
    assert var(-1, d) == 0 and var(1 << 31, d) == 0 and pack(-1) == 0
