"""CPU: the C ABI of the beam encoder under per-block bit budgets (0.15) is
exported and bound, and its host-side validation answers before any launch."""
from compression_without_quantization_amd import _lib

NAMES = ("cwq_beam_encode_var", "cwq_selftest_beam_encode_var")


def test_abi_version_and_symbols(cwqlib):
    assert _lib.ABI_VERSION >= 15 and cwqlib.cwq_version() == _lib.ABI_VERSION
    for name in NAMES:
        assert hasattr(cwqlib, name) and name in _lib.SIGNATURES, name
    import compression_without_quantization_amd as C
    for name in ("encode_blocks_var_beam", "code_grouped_greedy_sample_var_beam"):
        assert callable(getattr(C, name)) and name in C.__all__, name


def _call(cwqlib, nb=2, d=4, max_bits=3, n_steps=2, beam=2, ws=None, path=None, bits=1,
          opts=None):
    """Non-null dummy pointers: validation must answer before anything is read."""
    need = cwqlib.cwq_beam_encode_workspace_size(nb, nb * d, d, max(n_steps, 1),
                                                 min(max(beam, 1), 16))
    args = (1, 1, 1, 1, None, nb, nb * d, d, bits, max_bits, n_steps, beam, 42, 1.0, 0, 1, 1, None,
            1, need if ws is None else ws, opts, None)
    if path is None:
        return cwqlib.cwq_beam_encode_var(*args)
    return cwqlib.cwq_selftest_beam_encode_var(*args, path)


def test_invalid_arguments_rejected_before_launch(cwqlib):
    err = cwqlib.cwq_last_error
    for beam in (0, 17, -3):
        assert _call(cwqlib, beam=beam) == -1 and b"beam" in err()
    for mb in (-1, 31):
        assert _call(cwqlib, max_bits=mb) == -1 and b"max_bits" in err()
    # beam * 2^max_bits may not exceed 2^31: 2 * 2^30 is the limit
    for beam, mb in ((3, 30), (9, 28)):
        assert _call(cwqlib, beam=beam, max_bits=mb) == -1
        assert b"2^31" in err() and b"max_bits" in err()
    # (2, 30) passes every argument check: only the workspace, the last one, refuses
    assert _call(cwqlib, beam=2, max_bits=30, ws=1) == -3 and b"workspace" in err()
    assert _call(cwqlib, n_steps=0) == -1 and b"n_steps" in err()
    assert _call(cwqlib, bits=None) == -1 and b"n_bits" in err()
    # the lane-per-row kernel holds a row of at most 64 dims
    assert _call(cwqlib, d=65, path=0) == -1 and b"lane" in err()
    assert _call(cwqlib, path=4) == -1 and b"path" in err()
    assert _call(cwqlib, path=-1) == -1 and b"path" in err()
    assert _call(cwqlib, opts=_lib.options(prune_mode=3)) == -1 and b"cwq_options" in err()


def test_workspace_is_the_fixed_calls(cwqlib):
    need = cwqlib.cwq_beam_encode_workspace_size(2, 8, 4, 2, 2)
    assert need > 0
    assert _call(cwqlib, ws=need - 1) == -3 and b"workspace" in cwqlib.cwq_last_error()


def test_empty_call(cwqlib):
    """nb = 0 succeeds without touching the device and clears the message."""
    assert _call(cwqlib, beam=0) == -1 and cwqlib.cwq_last_error() != b""
    assert cwqlib.cwq_beam_encode_var(None, None, None, None, None, 0, 0, 0, None, 3, 1, 2, 42,
                                      1.0, 0, None, None, None, None, 0, None, None) == 0
    assert cwqlib.cwq_last_error() == b""
