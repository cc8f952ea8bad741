"""CPU: the beam encoder's C ABI (0.11) is exported and bound, and its
host-side validation answers before any launch."""
import numpy as np

from compression_without_quantization_amd import _lib

NAMES = ("cwq_beam_encode_workspace_size", "cwq_beam_encode", "cwq_selftest_beam_encode")


def test_abi_version_and_symbols(cwqlib):
    assert _lib.ABI_VERSION >= 11 and cwqlib.cwq_version() == _lib.ABI_VERSION
    for name in NAMES:
        assert hasattr(cwqlib, name) and name in _lib.SIGNATURES, name
    import compression_without_quantization_amd as C
    assert callable(C.encode_blocks_beam) and callable(C.code_grouped_greedy_sample_beam)
    assert "encode_blocks_beam" in C.__all__ and "code_grouped_greedy_sample_beam" in C.__all__


def test_workspace_formula(cwqlib):
    """include/cwq.h: 3 + 2 beam floats per dim, a key list per tile, the selected keys."""
    up = lambda v: (v + 255) // 256 * 256
    for nb, D, steps, beam in [(18, 8711, 3, 4), (300, 9600, 4, 16), (1, 4095, 30, 3),
                               (5000, 25000, 2, 1)]:
        want = -(-2048 // nb)
        t = 1
        while t < want:
            t *= 2
        need = 3 * up(4 * D) + up(8 * beam * D) + up(8 * beam * nb * 4 * t) + \
            up(8 * beam * nb * steps)
        assert cwqlib.cwq_beam_encode_workspace_size(nb, D, 64, steps, beam) == need
    assert cwqlib.cwq_beam_encode_workspace_size(0, 0, 0, 1, 1) == 0
    for bad in [(-1, 0, 0, 1, 1), (1, 4, 4, 0, 1), (1, 4, 4, 1, 0), (1, 4, 4, 1, 17)]:
        assert cwqlib.cwq_beam_encode_workspace_size(*bad) == 0


def _call(cwqlib, nb=2, d=4, n_bits=3, n_steps=2, beam=2, ws=None, path=None, off=None):
    """Non-null dummy pointers: validation must answer before anything is read."""
    need = cwqlib.cwq_beam_encode_workspace_size(nb, nb * d, d, max(n_steps, 1),
                                                 min(max(beam, 1), 16))
    args = (1, 1, 1, 1, off, nb, nb * d, d, n_bits, n_steps, beam, 42, 1.0, 0, 1, 1, None, 1,
            need if ws is None else ws, None, None)
    if path is None:
        return cwqlib.cwq_beam_encode(*args)
    return cwqlib.cwq_selftest_beam_encode(*args, path)


def test_invalid_arguments_rejected_before_launch(cwqlib):
    for beam in (0, 17, -3):
        assert _call(cwqlib, beam=beam) == -1 and b"beam" in cwqlib.cwq_last_error()
    # beam * 2^b may not exceed 2^31: 2 * 2^30 is the limit, 3 * 2^30 is past it
    assert _call(cwqlib, n_bits=30, beam=3) == -1 and b"2^31" in cwqlib.cwq_last_error()
    assert _call(cwqlib, n_bits=28, beam=9) == -1 and b"2^31" in cwqlib.cwq_last_error()
    assert _call(cwqlib, n_bits=31) == -1 and b"n_bits_per_step" in cwqlib.cwq_last_error()
    assert _call(cwqlib, n_steps=0) == -1 and b"n_steps" in cwqlib.cwq_last_error()
    need = cwqlib.cwq_beam_encode_workspace_size(2, 8, 4, 2, 2)
    assert need > 0
    assert _call(cwqlib, ws=need - 1) == -3 and b"workspace" in cwqlib.cwq_last_error()
    # the lane-per-row kernel holds a row of at most 64 dims
    assert _call(cwqlib, d=65, path=0) == -1 and b"lane" in cwqlib.cwq_last_error()
    assert _call(cwqlib, path=4) == -1 and _call(cwqlib, path=-1) == -1
    # an empty call succeeds without touching the device and clears the message
    assert cwqlib.cwq_beam_encode(None, None, None, None, None, 0, 0, 0, 3, 1, 2, 42, 1.0, 0,
                                  None, None, None, None, 0, None, None) == 0
    assert cwqlib.cwq_last_error() == b""
    o = _lib.options(prune_mode=3)
    assert cwqlib.cwq_beam_encode(1, 1, 1, 1, None, 2, 8, 4, 3, 2, 2, 42, 1.0, 0, 1, 1, None, 1,
                                  need, o, None) == -1
    assert b"cwq_options" in cwqlib.cwq_last_error()


def test_plan_rule_on_the_host(tmp_path):
    """csrc/cwq_dispatch.h beam_plan / beam_tiles_per_block compiled for the
    host: the lane kernel up to 64 dims, the wave kernel above and for an
    unknown length; tiles per block are a power of two that divides 2^b and
    never exceeds the cap the workspace is sized with."""
    import ctypes
    import os
    import subprocess
    from conftest import REPO
    so = tmp_path / "libbeam_plan.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(REPO, "tests", "native", "beam_plan.cpp")])
    L = ctypes.CDLL(str(so))
    i64 = ctypes.c_int64
    L.bp_path.argtypes, L.bp_path.restype = [i64], ctypes.c_int
    L.bp_tiles_cap.argtypes, L.bp_tiles_cap.restype = [i64], i64
    L.bp_tiles_per_block.argtypes = [ctypes.c_int, i64, i64, ctypes.c_int]
    L.bp_tiles_per_block.restype = i64
    assert [L.bp_path(d) for d in (0, 1, 63, 64, 65, 4095, -1)] == [0, 0, 0, 0, 1, 1, 1]
    for nb in (1, 3, 18, 300, 2047, 2048, 2049, 65536):
        cap = L.bp_tiles_cap(nb)
        assert cap >= 4 and cap & (cap - 1) == 0
        assert nb * (cap // 4) >= 2048 or cap == 4
        for bits in (0, 1, 3, 6, 8, 14, 30):
            n = 1 << bits
            for path, rows in ((0, 128), (1, 4)):
                t = L.bp_tiles_per_block(path, nb, n, 0)
                q = L.bp_tiles_per_block(path, nb, n, 1)
                assert 1 <= t <= cap // 4 and n % t == 0 and t & (t - 1) == 0
                assert t == 1 or n // t >= rows        # no tile below a row per lane / wave
                assert q == min(4 * t, n) and q <= cap
    # the benchmark's shapes: one tile of 256 rows per block; 30 x 14 bits on a few long groups
    assert L.bp_tiles_per_block(0, 65536, 256, 0) == 1
    assert L.bp_tiles_per_block(1, 18, 1 << 14, 0) == 128
