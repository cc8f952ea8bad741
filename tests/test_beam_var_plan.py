"""CPU: the counts the beam kernels take per block under per-block bit budgets
(csrc/cwq_beam_plan.h), compiled for the host next to the tiling rule and the
workspace layout they must fit."""
import ctypes
import os
import subprocess

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = tmp_path_factory.mktemp("beam_var_plan") / "libbeam_var_plan.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(REPO, "tests", "native", "beam_var_plan.cpp")])
    L = ctypes.CDLL(str(so))
    i64, ci = ctypes.c_int64, ctypes.c_int
    for name in ("bvp_live", "bvp_keep"):
        getattr(L, name).argtypes, getattr(L, name).restype = [ci, ci, ci], ci
    L.bvp_clamp.argtypes, L.bvp_clamp.restype = [ctypes.c_int32, ci], ci
    L.bvp_tiles_cap.argtypes, L.bvp_tiles_cap.restype = [i64], i64
    L.bvp_tiles_per_block.argtypes, L.bvp_tiles_per_block.restype = [ci, i64, i64, ci], i64
    L.bvp_tiles_bytes.argtypes, L.bvp_tiles_bytes.restype = [i64, i64, ci, ci], i64
    return L


def test_live_counts_closed_form(plan):
    """beam_live(b, i, B) = min(B, 2^(b i)), which is the recursion L_0 = 1,
    L_{i+1} = min(B, L_i 2^b) of include/cwq.h; b * i reaches 1,920 and
    16 << 30 does not fit 32 bits."""
    for b in range(31):
        for B in range(1, 17):
            L = 1
            for i in range(65):
                assert plan.bvp_live(b, i, B) == min(B, 1 << (b * i)) == L, (b, B, i)
                assert plan.bvp_keep(b, i, B) == min(B, L << b), (b, B, i)
                L = min(B, L << b)


def test_counts_are_read_clamped(plan):
    assert plan.bvp_tab_len() == 31
    for mb in (0, 6, 30):
        for b in (-2147483648, -3, -1, 0, 1, mb, mb + 1, 11, 31, 2147483647):
            assert plan.bvp_clamp(b, mb) == min(max(b, 0), mb)


@pytest.mark.parametrize("nb", [1, 3, 18, 300, 2047, 2048, 2049, 65536])
def test_tile_table_fits_the_workspace(plan, nb):
    """tpb[b] <= stride = tpb[max_bits] <= beam_tiles_cap(nb) on both paths and
    both tile sizes, every tpb[b] a power of two dividing 2^b, and the slots
    [nb][stride][beam] of u64 keys fit beam_ws's tiles region."""
    cap = plan.bvp_tiles_cap(nb)
    for path in (0, 1):
        for quarter in (0, 1):
            tpb = [plan.bvp_tiles_per_block(path, nb, 1 << b, quarter) for b in range(31)]
            assert all(x <= y for x, y in zip(tpb, tpb[1:]))  # monotone in 2^b
            for max_bits in range(31):
                stride = tpb[max_bits]
                assert 1 <= stride <= cap
                for b in range(max_bits + 1):
                    assert 1 <= tpb[b] <= stride and (1 << b) % tpb[b] == 0
                    assert tpb[b] & (tpb[b] - 1) == 0
            for beam in (1, 5, 16):
                assert nb * tpb[30] * beam * 8 <= plan.bvp_tiles_bytes(nb, 32 * nb, 4, beam)
