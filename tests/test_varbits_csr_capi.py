"""CPU: the per-block bit budget entry points for CSR blocks (ABI 0.9) are
exported and bound, and their host-side validation runs before any HIP call
(no device work is started here)."""
from compression_without_quantization_amd import _lib

NEW = ["cwq_block_bits_csr", "cwq_greedy_encode_var_workspace_size", "cwq_greedy_encode_var"]


def test_symbols_exported_and_bound(cwqlib):
    for name in NEW:
        assert hasattr(cwqlib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION >= 9 and cwqlib.cwq_version() == _lib.ABI_VERSION
    import compression_without_quantization_amd as C
    for name in ("code_grouped_greedy_sample_var", "decode_grouped_greedy_sample_var",
                 "block_bits", "encode_blocks_var", "decode_blocks_var"):
        assert name in C.__all__ and callable(getattr(C, name))


def test_workspace_size(cwqlib):
    size = cwqlib.cwq_greedy_encode_var_workspace_size
    plain = cwqlib.cwq_greedy_encode_workspace_size
    for nb, D, mbd in [(0, 0, 0), (1, 8, 8), (97, 2672, 130), (4, 1145, 1100), (49, 196608, 4095),
                       (20011, 90000, 9)]:
        by_steps = [size(nb, D, mbd, s) for s in (1, 2, 30)]
        assert by_steps == sorted(by_steps)
        if nb >= 64:  # the staged indices (4 nb n_steps bytes, rounded up to 256)
            assert by_steps[0] < by_steps[1] < by_steps[2]
        elif nb >= 4:
            assert by_steps[0] < by_steps[2]
        # five sorted arrays and the staged indices on top of one encoder workspace
        assert by_steps[2] >= plain(nb, D, mbd) + 20 * D + 4 * nb * 30
    assert size(97, 2672, 1100, 2) > size(97, 2672, 130, 2)  # the long blocks' records
    # negative or overflowing arguments
    assert size(-1, 8, 8, 1) == 0 and size(1, -8, 8, 1) == 0 and size(1, 8, -8, 1) == 0
    assert size(1, 8, 8, 0) == 0 and size(1 << 31, 8, 8, 1) == 0
    assert size(1, 1 << 62, 8, 1) == 0
    assert size((1 << 31) - 1, 8, 8, (1 << 31) - 1) == 0


def test_bad_arguments_refused_before_any_launch(cwqlib):
    enc = cwqlib.cwq_greedy_encode_var
    need = cwqlib.cwq_greedy_encode_var_workspace_size(100, 400, 4, 1)

    def call(nb=100, D=400, mbd=4, n_steps=1, ws_bytes=need, opts=None, t_scale=1, off=1, bits=1,
             out_idx=1, out_sample=1, ws=1):
        return enc(1, t_scale, 1, 1, off, nb, D, mbd, bits, n_steps, 42, 1.0, 0, out_idx,
                   out_sample, ws, ws_bytes, opts, None)

    assert call(nb=-1) == -1 and call(nb=1 << 31) == -1
    assert call(D=-40) == -1 and call(mbd=-4) == -1
    assert call(n_steps=0) == -1
    assert b"n_steps" in cwqlib.cwq_last_error()
    assert call(off=None) == -1 and call(bits=None) == -1 and call(out_idx=None) == -1
    assert call(t_scale=None) == -1 and call(out_sample=None) == -1
    assert call(opts=_lib.options(prune_mode=3)) == -1
    assert b"cwq_options" in cwqlib.cwq_last_error()
    assert call(ws_bytes=need - 1) == -3
    assert b"workspace" in cwqlib.cwq_last_error()
    assert call(ws=None) == -3
    assert call(n_steps=2) == -3  # more steps stage more indices
    # no blocks: accepted without touching the device, and the error is cleared
    assert enc(None, None, None, None, None, 0, 0, 0, None, 1, 42, 1.0, 0, None, None, None, 0,
               None, None) == 0
    assert cwqlib.cwq_last_error() == b""

    bb = cwqlib.cwq_block_bits_csr
    assert bb(1, 1, 1, 1, 1, -1, 40, 0.0, 1, 0, 30, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 1, 10, -40, 0.0, 1, 0, 30, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 1, 10, 40, 0.0, 0, 0, 30, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 1, 10, 40, 0.0, 1, 0, 31, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 1, 10, 40, 0.0, 1, -1, 30, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 1, 10, 40, 0.0, 1, 9, 8, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 1, 10, 40, float("nan"), 1, 0, 30, 1, None, None) == -1
    assert bb(1, 1, 1, 1, None, 10, 40, 0.0, 1, 0, 30, 1, None, None) == -1
    assert bb(1, 1, 1, 1, 1, 10, 40, 0.0, 1, 0, 30, None, None, None) == -1
    assert bb(None, 1, 1, 1, 1, 10, 40, 0.0, 1, 0, 30, 1, None, None) == -1
    assert bb(None, None, None, None, None, 0, 0, 1.44, 1, 0, 30, None, None, None) == 0
    assert cwqlib.cwq_last_error() == b""
