"""CPU: the rate table's plan (csrc/cwq_rate_plan.h) and workspace layout
(rate_ws, csrc/cwq_workspace.h), compiled for the host from the headers
themselves (tests/native/rate_plan.cpp).

Every path of the call is bit-exact by design, so the GPU tests cannot see a
shape rerouted between the lane-per-row and the wave-per-row scorer, or a budget
moved between the levels launch and the tuned encoders.  These can: the plan is
held to a Python restatement over a table of shapes, and the layout to the
checks tests/test_workspace_layout.py applies to the others."""
import ctypes
import itertools
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = ctypes.c_int64

BITS = (0, 1, 8, 11, 12, 16, 30)
UNIFORM_D = (7, 8, 32, 64, 100)
CSR_MAX_D = (1, 64, 65, 255, 256, 4095, -1)
NB = (0, 1, 2048, 10 ** 6)


@pytest.fixture(scope="module")
def rp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rate_plan") / "librate_plan.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-o", so,
                           os.path.join(REPO, "tests", "native", "rate_plan.cpp")])
    lib = ctypes.CDLL(so)
    lib.rp_plan.restype = None
    lib.rp_plan.argtypes = [ctypes.c_int, I64, I64, I64, ctypes.c_int, ctypes.POINTER(I64)]
    lib.rp_level.restype = ctypes.c_int
    lib.rp_level.argtypes = [ctypes.c_uint32]
    lib.rp_consts.restype = None
    lib.rp_consts.argtypes = [ctypes.POINTER(I64)]
    lib.rp_ws.restype = None
    lib.rp_ws.argtypes = [ctypes.c_int, I64, I64, I64, ctypes.c_int, ctypes.POINTER(I64)]
    return lib


def plan(rp, csr, ud, max_d, nb, B):
    out = (I64 * 8)()
    rp.rp_plan(int(csr), ud, max_d, nb, B, out)
    keys = ("levels", "long_rows", "tiles_per_block", "rows_per_tile", "tiles", "workgroups",
            "high_first", "high_count")
    return dict(zip(keys, out))


def restated(csr, ud, max_d, nb, B, target_tiles=16384, grid_cap=1 << 16, long_d=256):
    """The plan as DESIGN.md 4j states it."""
    L = min(B, 11)
    rows = 1 << L
    want = -(-target_tiles // nb) if nb > 0 else 1
    want = max(1, min(want, -(-rows // 256)))
    per_tile = max(256, -(-(-(-rows // want)) // 256) * 256)
    tiles_per_block = -(-rows // per_tile)
    tiles = nb * tiles_per_block
    return dict(levels=L, long_rows=int(max_d < 0 or max_d >= long_d),
                tiles_per_block=tiles_per_block, rows_per_tile=per_tile, tiles=tiles,
                workgroups=min(tiles, grid_cap), high_first=12, high_count=max(B - 11, 0))


def shapes():
    for B, nb in itertools.product(BITS, NB):
        for d in UNIFORM_D:
            yield False, d, d, nb, B
        for max_d in CSR_MAX_D:
            yield True, 0, max_d, nb, B


def test_constants(rp):
    c = (I64 * 6)()
    rp.rp_consts(c)
    assert list(c) == [11, 12, 4096, 256, 1 << 16, 16384]
    assert 1 << c[1] == c[2], "the levels launch ends where the screened encoders begin"


def test_plan_over_the_table_of_shapes(rp):
    n = 0
    for shape in shapes():
        assert plan(rp, *shape) == restated(*shape), shape
        n += 1
    assert n == len(BITS) * len(NB) * (len(UNIFORM_D) + len(CSR_MAX_D))


def test_plan_by_hand(rp):
    # one block: its 2,048 rows go to eight workgroups of 256 rows
    p = plan(rp, False, 8, 8, 1, 13)
    assert (p["levels"], p["tiles_per_block"], p["rows_per_tile"], p["workgroups"]) == (11, 8, 256, 8)
    assert (p["high_first"], p["high_count"]) == (12, 2)
    # B = 11 is the last budget without an encoder launch, B = 12 the first with one
    assert plan(rp, False, 32, 32, 5, 11)["high_count"] == 0
    assert plan(rp, False, 32, 32, 5, 12)["high_count"] == 1
    # many blocks: one tile each, the grid capped and strided
    p = plan(rp, False, 32, 32, 10 ** 6, 8)
    assert (p["tiles_per_block"], p["rows_per_tile"], p["tiles"], p["workgroups"]) == \
        (1, 256, 10 ** 6, 1 << 16)
    # no block: nothing is launched
    assert plan(rp, True, 0, 64, 0, 16)["workgroups"] == 0
    # rows are long from 256 dims on, and when the longest block is unknown
    assert [plan(rp, True, 0, m, 4, 9)["long_rows"] for m in (255, 256, -1)] == [0, 1, 1]
    assert plan(rp, False, 100, 100, 4, 9)["long_rows"] == 0


def test_tiles_are_256_aligned_and_cover_the_rows(rp):
    for shape in shapes():
        p = plan(rp, *shape)
        rows = 1 << p["levels"]
        assert p["rows_per_tile"] % 256 == 0
        assert (p["tiles_per_block"] - 1) * p["rows_per_tile"] < rows <= \
            p["tiles_per_block"] * p["rows_per_tile"], shape


def test_levels(rp):
    assert [rp.rp_level(n) for n in (0, 1, 2, 3, 4, 255, 256, 2047, 2048)] == \
        [0, 1, 2, 2, 3, 8, 9, 11, 12]
    for r in range(1, 12):  # level r >= 1 is rows [2^(r-1), 2^r): budget b holds levels 0 .. b
        assert rp.rp_level((1 << (r - 1))) == r == rp.rp_level((1 << r) - 1)


# ---- the layout ---------------------------------------------------------------
NAMES = ("enc", "lkeys", "hkeys", "sample", "idx")


def layout(rp, csr, nb, D, max_d, B):
    out = (I64 * 13)()
    rp.rp_ws(int(csr), nb, D, max_d, B, out)
    regions = [(NAMES[i], out[2 * i], out[2 * i + 1]) for i in range(5)]
    return regions, out[10], out[11], out[12]


def layout_shapes():
    for B in BITS:
        for nb in (0, 1, 9, 2048):
            for d in (7, 8, 32, 100):
                yield False, nb, nb * d, d, B
            for d in (1, 64, 300, 4095):
                yield True, nb, nb * d // 2 + (d if nb else 0), d, B


def test_layout_regions_aligned_disjoint_and_inside_the_total(rp):
    for shape in layout_shapes():
        regions, total, enc_total, enc_with_defer = layout(rp, *shape)
        end = 0
        for name, off, nbytes in regions:
            assert off % 256 == 0 and off >= end, (shape, name)  # in order: disjoint
            end = off + nbytes
        assert end <= total and total % 256 == 0, shape
        by = {n: (o, b) for n, o, b in regions}
        csr, nb, D, max_d, B = shape
        assert by["enc"][1] == enc_with_defer >= enc_total, shape
        assert by["lkeys"][1] == nb * 12 * 8
        assert by["hkeys"][1] == nb * max(B - 11, 0) * 8
        assert by["sample"][1] == 4 * D
        assert by["idx"][1] == (4 * nb if B > 11 else 0)


def test_size_function_is_the_ragged_layouts_total(rp, cwqlib):
    """cwq_rate_table_workspace_bytes answers for ragged blocks; the uniform
    layout of the same blocks, which the call uses, is never larger."""
    for csr, nb, D, max_d, B in layout_shapes():
        need = int(cwqlib.cwq_rate_table_workspace_bytes(nb, D, max_d, B))
        assert need == layout(rp, True, nb, D, max_d, B)[1]
        assert layout(rp, csr, nb, D, max_d, B)[1] <= need, (csr, nb, D, max_d, B)
    assert cwqlib.cwq_rate_table_workspace_bytes(-1, 0, 0, 4) == 0
    assert cwqlib.cwq_rate_table_workspace_bytes(4, 32, 8, 31) == 0
