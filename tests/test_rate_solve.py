"""CPU: the total solver's plan (csrc/cwq_rate_solve.h) and its workspace
layouts, compiled for the host from the headers themselves
(tests/native/rate_solve.cpp).

cwq_choose_bits_total is defined as equal to ratetable.choose_bits_total: sixty
halvings of the price, taken several at a time from a tree of intervals.  The
tree, the walk and the products are the header's; here a plain C++ choose rule
drives them through the launch sequence of cwq_ratetable.hip and the result is
held to the NumPy restatement of the 60-step loop
(tests/rate_solve_reference.py): the final price as a float64 bit pattern, the
bits and the total, over crafted tables, targets and ranges."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rate_solve_reference as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = ctypes.c_int64
F64 = ctypes.c_double


@pytest.fixture(scope="module")
def rs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rate_solve") / "librate_solve.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared",
                           "-o", so, os.path.join(REPO, "tests", "native", "rate_solve.cpp")])
    lib = ctypes.CDLL(so)
    lib.rs_consts.restype = None
    lib.rs_consts.argtypes = [ctypes.POINTER(I64)]
    lib.rs_node.restype = None
    lib.rs_node.argtypes = [F64, F64, ctypes.c_int, ctypes.POINTER(F64)]
    lib.rs_span_round_trip.restype = F64
    lib.rs_span_round_trip.argtypes = [F64]
    lib.rs_span_key.restype = ctypes.c_uint64
    lib.rs_span_key.argtypes = [F64]
    lib.rs_solve.restype = None
    lib.rs_solve.argtypes = [ctypes.c_void_p, I64, ctypes.c_int, I64, ctypes.c_int, ctypes.c_int,
                             ctypes.c_void_p, ctypes.POINTER(F64), ctypes.POINTER(I64)]
    lib.rs_solve_ws.restype = None
    lib.rs_solve_ws.argtypes = [I64, ctypes.c_int, ctypes.POINTER(I64)]
    lib.rs_enc_rate_ws.restype = None
    lib.rs_enc_rate_ws.argtypes = [I64, I64, I64, ctypes.c_int, ctypes.POINTER(I64)]
    return lib


def consts(rs):
    c = (I64 * 6)()
    rs.rs_consts(c)
    return dict(zip(("levels", "rounds", "slots", "halvings", "launches", "state_bytes"), c))


def solve(rs, value, lo, hi, target):
    v = np.ascontiguousarray(value, np.float32)
    bits = np.full(v.shape[0], -1, np.int32)
    lam, total = F64(-1.0), I64(-1)
    rs.rs_solve(v.ctypes.data, v.shape[0], v.shape[1], target, lo, hi, bits.ctypes.data,
                ctypes.byref(lam), ctypes.byref(total))
    return bits, lam.value, total.value


def test_constants(rs):
    c = consts(rs)
    assert c["halvings"] == 60 and c["levels"] * c["rounds"] == 60
    assert 3 <= c["levels"] <= 6 and c["slots"] == 1 << c["levels"] <= 64
    # a reset, the first sweep, a step and a sweep per round, the last step, the last pass
    assert c["launches"] == 2 + 2 * c["rounds"] + 2
    assert c["state_bytes"] == 40


def test_tree_is_the_loops_recurrence(rs):
    """Node k's interval is the one the 60-step loop holds after the halvings
    that k's bits spell, for intervals whose mids round."""
    levels = consts(rs)["levels"]
    out = (F64 * 3)()
    for lo, hi in ((0.0, 1.0), (0.0, 3.4028234663852886e38), (0.1, 0.7000000000000001),
                   (1e-300, 3e-300), (0.0, 0.0), (5e-324, 1.5e-323)):
        for k in range(1, 1 << levels):
            a, b = lo, hi
            for bit in bin(k)[3:]:
                mid = 0.5 * (a + b)
                a, b = (mid, b) if bit == "1" else (a, mid)
            rs.rs_node(lo, hi, k, out)
            assert [SR.lam_bits(x) for x in out] == \
                [SR.lam_bits(x) for x in (a, b, 0.5 * (a + b))], (lo, hi, k)


def test_span_key_orders_as_the_doubles_do(rs):
    xs = [0.0, 5e-324, 1e-300, 0.3, 1.0, 1.0000000000000002, 3.4e38, 6.8056469327705772e38]
    keys = [rs.rs_span_key(x) for x in xs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(rs.rs_span_round_trip(x) == x for x in xs)
    # what cannot be a maximum (the span at b = lo is +0) is +0
    assert rs.rs_span_key(-1.0) == rs.rs_span_key(-0.0) == rs.rs_span_key(float("nan")) == 0


@pytest.mark.parametrize("nb", SR.NB)
def test_solver_equals_the_sixty_step_loop(rs, nb):
    n = exact = zero = 0
    for v, lo, hi, T in SR.cases(nbs=(nb,)):
        wb, wl, wt = SR.choose_bits_total(v, T, lo, hi)
        gb, gl, gt = solve(rs, v, lo, hi, T)
        what = (v.shape, lo, hi, T)
        assert SR.lam_bits(gl) == SR.lam_bits(wl), what
        assert np.array_equal(gb, wb) and gt == wt, what
        assert gt <= T, what
        n += 1
        exact += gt == T
        zero += wl == 0.0
    assert n >= 7 * 5 * 2 and exact > 0 and zero > 0


def test_a_target_met_exactly_tells_the_walks_apart(rs):
    """Some targets are met exactly by some price; there the walk's ``<=``
    matters: with ``<`` the loop ends at another, higher price (and, above the
    floor of min_bits everywhere, at a smaller total)."""
    v = SR.crafted_table(65, 8)
    met = []
    for T in SR.targets(v, 0, 8):
        bits, lam, total = SR.choose_bits_total(v, T, 0, 8)
        if total == T and lam > 0.0:
            met.append(T)
            _, lam_strict, total_strict = SR.choose_bits_total(v, T, 0, 8, strict=True)
            assert lam_strict > lam and (total_strict < T or T == 0)
            gb, gl, gt = solve(rs, v, 0, 8, T)
            assert SR.lam_bits(gl) == SR.lam_bits(lam) and gt == T
    assert any(T > 0 for T in met), "no target of this table is met exactly: choose another table"


def test_clamp_level_table_resolves_nothing_below_the_span(rs):
    """with a -FLT_MAX row and a +FLT_MAX entry lam_hi starts near
    3.4e38 and sixty halvings end near 3e20, where every other block sits at
    min_bits.  The device solver is defined as equal, so it inherits this."""
    v = SR.crafted_table(65, 5, clamp=True)
    free = SR.total_at(v, 0.0, 0, 5)
    bits, lam, total = solve(rs, v, 0, 5, free // 2)
    wb, wl, wt = SR.choose_bits_total(v, free // 2, 0, 5)
    assert SR.lam_bits(lam) == SR.lam_bits(wl) and np.array_equal(bits, wb)
    assert lam > 1e19 and total == 5 and bits[2] == 5


# ---- the layouts ----------------------------------------------------------------
def _regions(out, names):
    return [(n, out[2 * i], out[2 * i + 1]) for i, n in enumerate(names)]


def _sound(regions, total, start=0):
    end = start
    for name, off, nbytes in regions:
        assert off % 256 == 0 and off >= end, name  # in order: disjoint
        end = off + nbytes
    assert end <= total and total % 256 == 0


def test_solver_layout(rs, cwqlib):
    c = consts(rs)
    for B in (0, 5, 8, 16, 30):
        out = (I64 * 7)()
        rs.rs_solve_ws(0, B, out)
        regions = _regions(out, ("state", "prod", "totals"))
        _sound(regions, out[6])
        by = {n: b for n, _, b in regions}
        assert by == {"state": c["state_bytes"], "prod": (B + 1) * c["slots"] * 8,
                      "totals": c["slots"] * 8}
        assert cwqlib.cwq_choose_bits_total_workspace_bytes(B) == out[6]
    assert cwqlib.cwq_choose_bits_total_workspace_bytes(-1) == 0
    assert cwqlib.cwq_choose_bits_total_workspace_bytes(31) == 0


def test_encode_rate_layout(rs, cwqlib):
    names = ("rate", "tidx", "tvalue", "state", "prod", "totals")
    for B in (0, 8, 11, 12, 16, 30):
        for nb, D, max_d in ((0, 0, 0), (1, 8, 8), (9, 72, 8), (40, 3000, 300), (2048, 65536, 32)):
            out = (I64 * 14)()
            rs.rs_enc_rate_ws(nb, D, max_d, B, out)
            regions = _regions(out, names)
            _sound(regions, out[12])
            by = {n: b for n, _, b in regions}
            assert by["rate"] == out[13] == cwqlib.cwq_rate_table_workspace_bytes(nb, D, max_d, B)
            assert by["tidx"] == by["tvalue"] == 4 * nb * (B + 1)
            assert cwqlib.cwq_greedy_encode_rate_workspace_bytes(nb, D, max_d, B) == out[12]
    assert cwqlib.cwq_greedy_encode_rate_workspace_bytes(-1, 0, 0, 4) == 0
    assert cwqlib.cwq_greedy_encode_rate_workspace_bytes(4, 32, 8, 31) == 0
