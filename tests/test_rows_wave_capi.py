"""CPU: the wave-per-row encoder's test entry (ABI 0.10) is exported and bound,
and it validates like cwq_greedy_encode before any HIP call (no device work is
started here)."""
from compression_without_quantization_amd import _lib

NAME = "cwq_selftest_encode_rows_wave"


def test_symbol_exported_and_bound(cwqlib):
    assert hasattr(cwqlib, NAME)
    assert NAME in _lib.SIGNATURES
    # cwq_greedy_encode's argument list without opts
    plain = list(_lib.SIGNATURES["cwq_greedy_encode"][1])
    plain.remove(_lib.c_opts)
    assert _lib.SIGNATURES[NAME] == (_lib.c_int, plain)
    assert _lib.ABI_VERSION >= 10 and cwqlib.cwq_version() == _lib.ABI_VERSION
    import compression_without_quantization_amd as C
    assert NAME not in C.__all__ and "selftest_encode_rows_wave" not in C.__all__


def test_bad_arguments_refused_before_any_launch(cwqlib):
    enc = getattr(cwqlib, NAME)
    need = cwqlib.cwq_greedy_encode_workspace_size(100, 400, 4)
    assert need > 0

    def call(nb=100, D=400, mbd=4, n_bits=9, n_steps=1, ws_bytes=need, t_loc=1, t_scale=1,
             p_loc=1, p_scale=1, off=1, out_idx=1, out_sample=1, ws=1):
        return enc(t_loc, t_scale, p_loc, p_scale, off, nb, D, mbd, n_bits, n_steps, 42, 1.0, 0,
                   out_idx, out_sample, ws, ws_bytes, None)

    assert call(n_bits=31) == -1
    assert b"n_bits_per_step=31" in cwqlib.cwq_last_error()
    assert call(n_bits=-1) == -1
    assert call(n_steps=0) == -1
    assert b"n_steps" in cwqlib.cwq_last_error()
    assert call(nb=-1) == -1 and call(D=-40) == -1 and call(mbd=-4) == -1
    assert call(off=None) == -1
    assert b"block_off" in cwqlib.cwq_last_error()
    assert call(out_idx=None) == -1
    assert b"out_idx" in cwqlib.cwq_last_error()
    for name in ("t_loc", "t_scale", "p_loc", "p_scale", "out_sample"):
        assert call(**{name: None}) == -1, name
        assert b"null" in cwqlib.cwq_last_error()
    assert call(ws_bytes=need - 1) == -3
    assert b"workspace" in cwqlib.cwq_last_error()
    assert call(ws=None) == -3
    # no blocks: accepted without touching the device (the workspace is checked
    # as cwq_greedy_encode checks it, and never used), and the error is cleared
    need0 = cwqlib.cwq_greedy_encode_workspace_size(0, 0, 0)
    assert enc(None, None, None, None, None, 0, 0, 0, 9, 1, 42, 1.0, 0, None, None, 1, need0,
               None) == 0
    assert cwqlib.cwq_last_error() == b""
