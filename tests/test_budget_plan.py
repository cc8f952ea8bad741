"""CPU: the plan of the calls whose blocks carry a bit count each
(csrc/cwq_budget_plan.h: cwq_greedy_encode_uniform_var, cwq_greedy_encode_var,
cwq_greedy_backfit_var), compiled for the host next to the tiling and the
rows-wave rule it reads (csrc/cwq_dispatch.h), against a restatement here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

i64, ci = ctypes.c_int64, ctypes.c_int
NONE, BITS, BAD_LEN, SUM_DIMS, LONGEST = range(5)  # BudgetRefusal, in the order of the checks


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = tmp_path_factory.mktemp("budget_plan") / "libbudget_plan.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o",
                           str(so), os.path.join(REPO, "tests", "native", "budget_plan.cpp")])
    L = ctypes.CDLL(str(so))
    p64 = ctypes.POINTER(i64)
    L.bp_fact_words.restype = ci
    L.bp_uniform_facts.argtypes, L.bp_uniform_facts.restype = \
        [ctypes.POINTER(ctypes.c_uint32), i64, p64], None
    L.bp_plan.argtypes, L.bp_plan.restype = [p64, ci, i64, i64, i64, ci, ci, p64, p64], ci
    L.bp_choose_tiling.argtypes, L.bp_choose_tiling.restype = [i64, i64, p64], None
    L.bp_rows_wave.argtypes, L.bp_rows_wave.restype = [ci, i64, i64, ci], ci
    assert L.bp_fact_words() == 161
    return L


class Facts:
    """VbcFacts: dims, maxd, pre, counts, start [32] and bad_len."""

    def __init__(self, counts, dims, maxd, bad_len=0):
        self.counts, self.dims, self.maxd = (np.asarray(a, np.int64) for a in (counts, dims, maxd))
        # bucket b's first row and first dim: exclusive scans in ascending bit order
        self.start = np.concatenate([[0], np.cumsum(self.counts)[:-1]])
        self.pre = np.concatenate([[0], np.cumsum(self.dims)[:-1]])
        self.bad_len = bad_len

    def words(self):
        return np.concatenate([self.dims, self.maxd, self.pre, self.counts, self.start,
                               [self.bad_len]]).astype(np.int64)


def _uniform_facts(counts, d):
    counts = np.asarray(counts, np.int64)
    return Facts(counts, counts * d, np.where(counts > 0, d, 0))


def _run(plan, f, csr, nb, total_dims, max_block_dim, n_steps=3, prune=2):
    w = np.ascontiguousarray(f.words())
    head, buckets = (i64 * 7)(), (i64 * 310)()
    rc = plan.bp_plan(w.ctypes.data_as(ctypes.POINTER(i64)), int(csr), nb, total_dims,
                      max_block_dim, n_steps, prune, head, buckets)
    assert rc == head[0]
    keys = ("bits", "r0", "d0", "count", "dims", "maxd", "block_off", "tiles_per_block",
            "cand_per_tile", "rows_wave")
    got = dict(zip(("refusal", "got", "limit", "n_buckets", "top", "sum_dims", "longest"), head))
    got["buckets"] = [dict(zip(keys, buckets[10 * i:10 * i + 10])) for i in range(head[3])]
    return got


COUNTS = {
    "one bin": [0] * 7 + [41] + [0] * 24,
    "every bin": list(range(1, 32)) + [0],
    "empty": [0] * 32,
    "bin 31": [3, 0, 5] + [0] * 28 + [2],
}


@pytest.mark.parametrize("d", [0, 1, 13, 32])
@pytest.mark.parametrize("name", list(COUNTS))
def test_uniform_facts(plan, name, d):
    counts = COUNTS[name]
    out = (i64 * 161)()
    plan.bp_uniform_facts((ctypes.c_uint32 * 32)(*counts), d, out)
    want = _uniform_facts(counts, d)
    assert np.array_equal(np.asarray(out[:]), want.words())
    assert want.bad_len == 0 and out[160] == 0
    # what the restatement says, spelled out once
    row = 0
    for b in range(32):
        assert out[96 + b] == counts[b] and out[128 + b] == row and out[64 + b] == row * d
        assert out[b] == counts[b] * d and out[32 + b] == (d if counts[b] else 0)
        row += counts[b]


def _random_facts(rng, csr):
    """Facts with some buckets empty, some of 0 dims, some long enough for the
    rows-wave rule; nb <= 2^16."""
    counts = np.where(rng.random(32) < 0.45, 0, rng.integers(1, 2000, 32))
    counts[31] = 0
    if not csr:
        return _uniform_facts(counts, int(rng.choice([0, 1, 13, 32, 300])))
    mean = rng.choice([0, 1, 7, 255, 256, 257, 900], 32)
    dims = np.where(rng.random(32) < 0.5, counts * mean, (counts * mean * rng.random(32)).astype(
        np.int64))
    maxd = np.where(dims > 0, np.minimum(dims, np.maximum(-(-dims // np.maximum(counts, 1)),
                                                          rng.integers(1, 4096, 32))), 0)
    return Facts(counts, dims, maxd)


@pytest.mark.parametrize("csr", [False, True])
def test_plan_on_random_facts(plan, csr):
    rng = np.random.Generator(np.random.PCG64(20 + csr))
    seen_wave = seen_zero_bucket = 0
    for trial in range(200):
        f = _random_facts(rng, csr)
        nb = int(f.counts.sum())
        sum_dims, longest = int(f.dims[:31].sum()), int(f.maxd[:31].max())
        prune = int(rng.integers(0, 3))
        got = _run(plan, f, csr, nb, sum_dims, longest, prune=prune)
        assert got["refusal"] == NONE and (got["got"], got["limit"]) == (0, 0)
        bk = got["buckets"]
        bits = [k["bits"] for k in bk]
        assert bits == sorted((b for b in range(31) if f.counts[b]), reverse=True)
        assert got["n_buckets"] == len(bits) and all(k["count"] > 0 for k in bk)
        assert got["top"] == (max(bits) if bits else 0)
        assert got["sum_dims"] == sum_dims and got["longest"] == longest
        # from the top down the rows and the dims are walked backwards without gap or overlap
        row_end, dim_end = nb - int(f.counts[31]), sum_dims
        for k in bk:
            b = k["bits"]
            assert k["r0"] == f.start[b] and k["d0"] == f.pre[b]
            assert k["count"] == f.counts[b] and k["dims"] == f.dims[b] and k["maxd"] == f.maxd[b]
            assert k["r0"] + k["count"] == row_end and k["d0"] + k["dims"] == dim_end
            row_end, dim_end = k["r0"], k["d0"]
            assert k["block_off"] == (k["r0"] + b if csr else -1)
            tiling = (i64 * 2)()
            plan.bp_choose_tiling(k["count"], 1 << b, tiling)
            assert (k["tiles_per_block"], k["cand_per_tile"]) == tuple(tiling)
            wave = bool(plan.bp_rows_wave(b, k["dims"], k["count"], prune))
            assert wave == ((1 << b) < 4096 and k["dims"] >= 256 * k["count"] and prune != 0)
            assert k["rows_wave"] == (csr and wave)
            seen_wave += k["rows_wave"]
            seen_zero_bucket += b == 0
        assert row_end == 0 and dim_end == 0
    assert seen_zero_bucket > 20 and (seen_wave > 50 if csr else seen_wave == 0)


def _refusable():
    """39 ragged blocks, 2,547 dims, the longest 300: valid at (39, 2547, 300)."""
    counts = [7, 6, 0, 7, 0, 0, 6, 0, 7, 0, 0, 0, 6] + [0] * 19
    dims = [400, 300, 0, 547, 0, 0, 500, 0, 450, 0, 0, 0, 350] + [0] * 19
    maxd = [257, 64, 0, 300, 0, 0, 257, 0, 300, 0, 0, 0, 64] + [0] * 19
    return counts, dims, maxd


def test_each_refusal_alone_and_their_order(plan):
    counts, dims, maxd = _refusable()
    ok = Facts(counts, dims, maxd)
    assert _run(plan, ok, True, 39, 2547, 300)["refusal"] == NONE
    wide = list(counts)
    wide[31], wide[0] = 2, wide[0] - 2
    cases = {
        BITS: (Facts(wide, dims, maxd), 2547, 300, (2, 39)),
        BAD_LEN: (Facts(counts, dims, maxd, bad_len=3), 2547, 300, (3, 0)),
        SUM_DIMS: (ok, 2546, 300, (2547, 2546)),
        LONGEST: (ok, 2547, 299, (300, 299)),
    }
    for code, (f, D, m, numbers) in cases.items():
        got = _run(plan, f, True, 39, D, m)
        assert got["refusal"] == code and (got["got"], got["limit"]) == numbers, code
    # all four at once, then without the first, the first two, ...: the order
    # counts in bin 31, bad_len, the dims' sum, the longest block
    for first in (BITS, BAD_LEN, SUM_DIMS, LONGEST):
        f = Facts(wide if first <= BITS else counts, dims, maxd,
                  bad_len=3 if first <= BAD_LEN else 0)
        D = 2546 if first <= SUM_DIMS else 2547
        got = _run(plan, f, True, 39, D, 299)
        assert got["refusal"] == first, first
        assert (got["got"], got["limit"]) == cases[first][3]
    # uniform blocks are refused for bin 31 alone: their dims follow from the counts
    u = _uniform_facts(COUNTS["bin 31"], 13)
    got = _run(plan, u, False, 10, 130, 13)
    assert got["refusal"] == BITS and (got["got"], got["limit"]) == (2, 10)
    assert _run(plan, _uniform_facts(COUNTS["one bin"], 13), False, 41, 533, 13)["refusal"] == NONE
