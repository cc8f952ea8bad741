"""The encode dispatch (csrc/cwq_dispatch.h, DESIGN.md "Encode dispatch") on the
host: which path a launch_encode call of a given shape takes.

Every path is bit-exact by design, so the GPU tests, which compare outputs with
the oracle, cannot see a shape being rerouted.  These tests can: a table of
shapes to paths, the thresholds, and every shape for which a GPU test names a
path in its docstring."""
import ctypes

import pytest

import encode_shapes as S

ROWS_WAVE, UNIFORM_PRUNED, CSR_PRUNED, SMALL_PIPE, SMALL_THREE, EVAL = range(6)
I64 = ctypes.c_int64


@pytest.fixture(scope="module")
def mc(mathcheck):
    mathcheck.mc_encode_plan.argtypes = [ctypes.c_int, I64, I64, I64, I64, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_int)]
    mathcheck.mc_encode_plan.restype = None
    mathcheck.mc_has_screen_arrays.argtypes = [ctypes.c_int, I64, I64]
    mathcheck.mc_has_long_block_records.argtypes = [ctypes.c_int, I64, I64]
    mathcheck.mc_few_rows.argtypes = [I64, I64]
    mathcheck.mc_bucket_takes_rows_wave.argtypes = [ctypes.c_int, I64, I64, ctypes.c_int]
    mathcheck.mc_dispatch_consts.argtypes = [ctypes.POINTER(I64)]
    mathcheck.mc_dispatch_consts.restype = None
    return mathcheck


def plan(mc, *, csr, bits, prune, nb=4, ud=0, max_d=None, rows_wave=False, n_steps=1):
    """(path, coop, self_finalizing, fork parts) of one block range, as
    encode_impl fills the shape: uniform blocks have max_d == ud."""
    if max_d is None:
        assert not csr
        max_d = ud
    out = (ctypes.c_int * 4)()
    mc.mc_encode_plan(int(csr), ud, max_d, nb, 1 << bits, prune, int(rows_wave), n_steps, out)
    return out[0], bool(out[1]), bool(out[2]), out[3]


def part_sizes(nb, k):
    """launch_encode's split of nb blocks in k parts."""
    return [nb * (i + 1) // k - nb * i // k for i in range(k)]


def csr_paths(mc, sizes, bits, n_steps, prune=2):
    """Plans of a ragged call as launch_encode runs it: the whole call's plan
    (prep, destandardise, fork) and the plan of every block range that
    encode_steps is given (the parts of a forked call, else the whole)."""
    nb, max_d = len(sizes), max(sizes)
    whole = plan(mc, csr=True, bits=bits, prune=prune, nb=nb, max_d=max_d, n_steps=n_steps)
    k = whole[3]
    ranges = [plan(mc, csr=True, bits=bits, prune=prune, nb=n, max_d=max_d, n_steps=n_steps)
              for n in (part_sizes(nb, k) if k > 1 else [nb])]
    return whole, ranges


TABLE = [
    # uniform blocks: (ud, bits, prune, nb) -> path
    (dict(csr=False, ud=32, bits=16, prune=1), UNIFORM_PRUNED),
    (dict(csr=False, ud=32, bits=16, prune=2), UNIFORM_PRUNED),
    (dict(csr=False, ud=32, bits=16, prune=0), EVAL),
    # n_cand * 16 > 2^32 and no screening arrays for d = 64
    (dict(csr=False, ud=64, bits=30, prune=2), EVAL),
    (dict(csr=False, ud=64, bits=28, prune=2), UNIFORM_PRUNED),  # n_cand * 16 == 2^32
    (dict(csr=False, ud=5, bits=13, prune=2), CSR_PRUNED),
    (dict(csr=False, ud=5, bits=13, prune=1), EVAL),
    (dict(csr=False, ud=12, bits=8, prune=2), SMALL_PIPE),
    (dict(csr=False, ud=72, bits=8, prune=2), SMALL_THREE),
    # ragged blocks
    (dict(csr=True, max_d=64, bits=6, prune=2), SMALL_PIPE),
    (dict(csr=True, max_d=64, bits=11, prune=2), SMALL_PIPE),
    (dict(csr=True, max_d=64, bits=5, prune=2), EVAL),
    (dict(csr=True, max_d=64, bits=12, prune=2), CSR_PRUNED),
    (dict(csr=True, max_d=64, bits=8, prune=1), EVAL),
    (dict(csr=True, max_d=64, bits=12, prune=1), EVAL),
    (dict(csr=True, max_d=0, bits=8, prune=2), SMALL_PIPE),
    (dict(csr=True, max_d=65, bits=8, prune=2), SMALL_THREE),
    (dict(csr=True, max_d=130, bits=8, prune=2), SMALL_THREE),
    (dict(csr=True, max_d=-1, bits=8, prune=2), SMALL_THREE),
    (dict(csr=True, max_d=8, bits=8, prune=2, nb=(1 << 32) - 1), SMALL_PIPE),
    (dict(csr=True, max_d=8, bits=8, prune=2, nb=1 << 32), SMALL_THREE),
    # block lengths do not matter from 4,096 candidates on
    (dict(csr=True, max_d=-1, bits=12, prune=2), CSR_PRUNED),
    (dict(csr=True, max_d=4095, bits=30, prune=2), CSR_PRUNED),
]


@pytest.mark.parametrize("shape,path", TABLE)
def test_shape_takes_path(mc, shape, path):
    got, coop, self_finalizing, _ = plan(mc, **shape)
    assert got == path, shape
    assert self_finalizing == (path == SMALL_PIPE)
    assert not coop or path == CSR_PRUNED


@pytest.mark.parametrize("shape,path", TABLE)
def test_rows_wave_overrides_every_path(mc, shape, path):
    got, coop, self_finalizing, _ = plan(mc, rows_wave=True, **shape)
    assert (got, coop, self_finalizing) == (ROWS_WAVE, False, False), shape


def test_coop_threshold(mc):
    """Cooperative rows below 8 candidate rows per lane of the chip."""
    c = (I64 * 3)()
    mc.mc_dispatch_consts(c)
    limit = c[0]
    assert limit == 8 * 1536 * 256
    for nb, n_cand in ((limit - 1, 1), (1, limit - 1)):
        assert nb * n_cand == limit - 1 and mc.mc_few_rows(nb, n_cand)
    for nb, n_cand in ((limit, 1), (768, 1 << 12), (3, 1 << 20)):
        assert nb * n_cand == limit and not mc.mc_few_rows(nb, n_cand)
    n_cand = 1 << 12
    assert limit % n_cand == 0
    nb = limit // n_cand
    below = plan(mc, csr=True, bits=12, prune=2, nb=nb - 1, max_d=300)
    at = plan(mc, csr=True, bits=12, prune=2, nb=nb, max_d=300)
    assert below[:2] == (CSR_PRUNED, True) and at[:2] == (CSR_PRUNED, False)
    # nb * n_cand == limit - 1 has no power-of-two n_cand but 1: the flag is the
    # general pruned path's alone, the fork's part count reads the same product
    assert plan(mc, csr=True, bits=0, prune=2, nb=limit - 1, max_d=300, n_steps=2)[::3] == (EVAL, 3)
    assert plan(mc, csr=True, bits=0, prune=2, nb=limit, max_d=300, n_steps=2)[::3] == (EVAL, 2)
    # a small-candidate launch of few rows is not cooperative
    assert plan(mc, csr=True, bits=8, prune=2, nb=2, max_d=300)[:2] == (SMALL_THREE, False)


def test_fork_parts_and_per_part_coop(mc):
    c = (I64 * 3)()
    mc.mc_dispatch_consts(c)
    nb = c[0] >> 12  # nb * 4,096 candidates: exactly at the few-rows limit
    # the whole is not a few-rows launch, so it forks in two; each half is
    whole, ranges = csr_paths(mc, [300] * nb, 12, 2)
    assert whole[:2] == (CSR_PRUNED, False) and whole[3] == 2
    assert [r[:2] for r in ranges] == [(CSR_PRUNED, True)] * 2
    # few rows: three parts, never more parts than blocks
    assert plan(mc, csr=True, bits=12, prune=2, nb=nb - 1, max_d=300, n_steps=2)[3] == 3
    assert plan(mc, csr=True, bits=12, prune=2, nb=2, max_d=300, n_steps=2)[3] == 2
    # no fork: one step, one block, uniform blocks
    assert plan(mc, csr=True, bits=12, prune=2, nb=nb, max_d=300, n_steps=1)[3] == 1
    assert plan(mc, csr=True, bits=12, prune=2, nb=1, max_d=300, n_steps=2)[3] == 1
    assert plan(mc, csr=False, ud=5, bits=12, prune=2, nb=nb, n_steps=2)[3] == 1
    # the fork does not depend on the path
    assert plan(mc, csr=True, bits=8, prune=0, nb=9, max_d=64, n_steps=3)[3] == 3


def test_has_screen_arrays(mc):
    fast = set(range(8, 65, 8))
    for d in list(range(0, 140)) + [1024, 1025, 4095]:
        assert bool(mc.mc_has_screen_arrays(0, d, 3)) == (d not in fast), d
        assert not mc.mc_has_screen_arrays(0, d, 0)  # no uniform block at all
        for nb in (0, 3):
            assert mc.mc_has_screen_arrays(1, 0, nb)  # ragged blocks: always
            assert mc.mc_has_screen_arrays(1, d, nb)


def test_has_long_block_records(mc):
    c = (I64 * 3)()
    mc.mc_dispatch_consts(c)
    lds = c[2]
    assert lds == 1024
    for csr in (0, 1):
        assert not mc.mc_has_long_block_records(csr, lds, 3)
        assert mc.mc_has_long_block_records(csr, lds + 1, 3)
    assert mc.mc_has_long_block_records(1, lds + 1, 0)
    assert not mc.mc_has_long_block_records(0, lds + 1, 0)
    assert not mc.mc_has_long_block_records(1, -1, 3) and not mc.mc_has_long_block_records(1, 0, 3)


def test_bucket_rule(mc):
    """cwq_greedy_encode_var: a bucket below 4,096 candidates whose mean block
    reaches 256 dims takes the wave-per-row kernel, unless prune_mode is 0."""
    c = (I64 * 3)()
    mc.mc_dispatch_consts(c)
    assert c[1] == 256
    for count in (1, 3, 1000):
        for prune in (1, 2):
            assert mc.mc_bucket_takes_rows_wave(11, 256 * count, count, prune)
            assert not mc.mc_bucket_takes_rows_wave(12, 256 * count, count, prune)
            assert not mc.mc_bucket_takes_rows_wave(11, 256 * count - 1, count, prune)
            assert mc.mc_bucket_takes_rows_wave(0, 256 * count, count, prune)
            assert not mc.mc_bucket_takes_rows_wave(30, 4095 * count, count, prune)
        assert not mc.mc_bucket_takes_rows_wave(11, 256 * count, count, 0)
        assert not mc.mc_bucket_takes_rows_wave(0, 4095 * count, count, 0)


# ---------------------------------------------------------------------------
# the shapes for which a GPU test names a path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits,n_steps", S.SMALL_PATH_BITS_STEPS)
@pytest.mark.parametrize("name,path", [("pipeline", SMALL_PIPE), ("three_kernel", SMALL_THREE)])
def test_small_path_adversarial_shapes(mc, name, path, bits, n_steps):
    """test_gpu.py::test_small_path_adversarial: mode 2 takes the named
    small-candidate path, in the whole call and in every part of a forked one;
    mode 0 the exact kernel."""
    sizes = S.SMALL_PATH_SIZES[name]
    whole, ranges = csr_paths(mc, sizes, bits, n_steps)
    assert whole[0] == path and whole[2] == (path == SMALL_PIPE)
    assert whole[3] == (1 if n_steps == 1 else 3) and len(ranges) == whole[3]
    for r in ranges:
        assert r[:3] == (path, False, path == SMALL_PIPE)
    whole, ranges = csr_paths(mc, sizes, bits, n_steps, prune=0)
    assert {r[0] for r in ranges + [whole]} == {EVAL}


@pytest.mark.parametrize("d,bits,nb", S.UNIFORM_GENERAL_PRUNED)
def test_uniform_odd_d_general_pruned_shapes(mc, d, bits, nb):
    """test_gpu.py::test_uniform_odd_d_general_pruned: no d of it is one the
    uniform pruned kernel takes, so mode 2 runs the general pruned kernel
    (cooperatively: few rows), unforked, and mode 0 the exact kernel."""
    n_steps = S.UNIFORM_GENERAL_PRUNED_STEPS
    assert plan(mc, csr=False, ud=d, bits=bits, prune=2, nb=nb, n_steps=n_steps) == \
        (CSR_PRUNED, True, False, 1)
    assert plan(mc, csr=False, ud=d, bits=bits, prune=0, nb=nb, n_steps=n_steps)[0] == EVAL
    assert mc.mc_has_screen_arrays(0, d, nb)


@pytest.mark.parametrize("sizes,bits,n_steps,kind", S.CSR_COOP)
def test_csr_cooperative_rows_shapes(mc, sizes, bits, n_steps, kind):
    """test_gpu.py::test_csr_cooperative_rows_vs_oracle: mode 2 runs the general
    pruned kernel with cooperative rows in every block range, and its blocks
    reach the length from which a row is walked cooperatively."""
    c = (I64 * 3)()
    mc.mc_dispatch_consts(c)
    assert max(sizes) >= c[1]
    whole, ranges = csr_paths(mc, sizes, bits, n_steps)
    assert whole[:3] == (CSR_PRUNED, True, False)
    assert whole[3] == (1 if n_steps == 1 else min(3, len(sizes)))
    for r in ranges:
        assert r[:3] == (CSR_PRUNED, True, False)
    assert bool(mc.mc_has_long_block_records(1, max(sizes), len(sizes))) == (max(sizes) > c[2])
    assert {r[0] for r in csr_paths(mc, sizes, bits, n_steps, prune=0)[1]} == {EVAL}


@pytest.mark.parametrize("bits", S.ROWS_WAVE_BITS)
@pytest.mark.parametrize("n_steps", [1, 3])
def test_forced_rows_wave_shapes(mc, bits, n_steps):
    """test_rows_wave_gpu.py: cwq_selftest_encode_rows_wave forces the
    wave-per-row kernel (default options: prune_mode 2) in every block range."""
    sizes = S.ROWS_WAVE_LENGTHS
    nb, max_d = len(sizes), max(sizes)
    whole = plan(mc, csr=True, bits=bits, prune=2, nb=nb, max_d=max_d, rows_wave=True,
                 n_steps=n_steps)
    assert whole[:3] == (ROWS_WAVE, False, False)
    for n in part_sizes(nb, whole[3]):
        assert plan(mc, csr=True, bits=bits, prune=2, nb=n, max_d=max_d, rows_wave=True,
                    n_steps=n_steps)[:3] == (ROWS_WAVE, False, False)
    # without the flag these bit counts would leave every long row to one lane
    assert plan(mc, csr=True, bits=bits, prune=2, nb=nb, max_d=max_d)[0] in (EVAL, SMALL_THREE)


@pytest.mark.parametrize("n_short", [0, 40])
def test_encode_var_long_bucket_shapes(mc, n_short):
    """test_rows_wave_gpu.py::test_encode_var_long_buckets: with no short block
    every bucket takes the wave-per-row kernel; 40 blocks of 3 dims keep the
    9-bit bucket off it; prune_mode 0 keeps every bucket off it."""
    lens = S.LONG_LENS + [3] * n_short
    bits = S.LONG_BITS + [9] * n_short
    for b in set(bits):
        mine = [n for n, bb in zip(lens, bits) if bb == b]
        assert bool(mc.mc_bucket_takes_rows_wave(b, sum(mine), len(mine), 2)) == \
            (not (n_short and b == 9)), b
        assert not mc.mc_bucket_takes_rows_wave(b, sum(mine), len(mine), 0)


# ---------------------------------------------------------------------------
# test_workspace_state_gpu.py: each case's shape takes the path its name says
# ---------------------------------------------------------------------------
def test_workspace_state_uniform_shapes(mc):
    for d, bits, nb, n_steps in (S.WS_UNIFORM_PRUNED, S.WS_TILE_QUEUE):
        for prune in (1, 2):
            assert plan(mc, csr=False, ud=d, bits=bits, prune=prune, nb=nb, n_steps=n_steps) == \
                (UNIFORM_PRUNED, False, False, 1)
        assert plan(mc, csr=False, ud=d, bits=bits, prune=0, nb=nb, n_steps=n_steps) == \
            (EVAL, False, False, 1)
        assert not mc.mc_has_screen_arrays(0, d, nb)  # keys, tile queue, shard constants only
    # the tile queue's own conditions (launch_prune_t): one tile of >= 4,096
    # candidates per block, more tiles than the 1,536 resident workgroups
    d, bits, nb, _ = S.WS_TILE_QUEUE
    assert (1 << bits) >= 4096 and nb > 1536 and nb >= 16384
    d, bits, nb, _ = S.WS_UNIFORM_PRUNED
    assert nb <= 1536
    for d, bits, nb, n_steps in S.WS_UNIFORM_GENERAL:
        assert (d, bits, nb) in S.UNIFORM_GENERAL_PRUNED
        assert n_steps == S.UNIFORM_GENERAL_PRUNED_STEPS


def test_workspace_state_ragged_shapes(mc):
    c = (I64 * 3)()
    mc.mc_dispatch_consts(c)
    coop_min_d, lds = c[1], c[2]
    # the exact kernel: too few candidates for any screened path; forked (two steps)
    sizes, bits, n_steps = S.WS_EVAL_RAGGED
    whole, ranges = csr_paths(mc, sizes, bits, n_steps)
    assert whole[0] == EVAL and whole[3] == 3 and {r[0] for r in ranges} == {EVAL}
    assert 0 in sizes
    # per-lane rows: the general pruned kernel, no block long enough for a
    # cooperative row or a record, forked in three
    sizes, bits, n_steps = S.WS_CSR_LANE
    whole, ranges = csr_paths(mc, sizes, bits, n_steps)
    assert whole[0] == CSR_PRUNED and whole[3] == 3 and len(ranges) == 3
    assert {r[0] for r in ranges} == {CSR_PRUNED}
    assert max(sizes) < coop_min_d and 0 in sizes
    assert not mc.mc_has_long_block_records(1, max(sizes), len(sizes))
    # every sub-case in one call: cooperative rows, blocks on both sides of the
    # LDS / record boundary
    sizes, bits, n_steps = S.WS_CSR_ALL
    whole, ranges = csr_paths(mc, sizes, bits, n_steps)
    assert whole[:3] == (CSR_PRUNED, True, False) and whole[3] == 3
    assert [r[:2] for r in ranges] == [(CSR_PRUNED, True)] * 3
    assert min(sizes) < coop_min_d <= sorted(sizes)[1] and lds in sizes
    assert any(s > lds for s in sizes) and mc.mc_has_long_block_records(1, max(sizes), len(sizes))
    for name, path in (("pipeline", SMALL_PIPE), ("three_kernel", SMALL_THREE)):
        sizes, bits, n_steps = S.WS_SMALL[name]
        whole, ranges = csr_paths(mc, sizes, bits, n_steps)
        assert whole[0] == path and whole[2] == (path == SMALL_PIPE) and whole[3] == 3
        assert {r[:3] for r in ranges} == {(path, False, path == SMALL_PIPE)}


# ---------------------------------------------------------------------------
# test_near_ties_gpu.py: each near-tie case takes the path it names
# ---------------------------------------------------------------------------
ENCODE_PATHS = {"rows_wave": ROWS_WAVE, "uniform_pruned": UNIFORM_PRUNED, "csr_pruned": CSR_PRUNED,
                "small_pipe": SMALL_PIPE, "small_three": SMALL_THREE, "eval": EVAL}


@pytest.fixture(scope="module")
def search_plans(tmp_path_factory):
    """beam_plan and backfit_plan (csrc/cwq_dispatch.h) compiled for the host."""
    import os
    import subprocess
    from conftest import REPO
    out = []
    for name in ("beam_plan", "backfit_plan"):
        so = tmp_path_factory.mktemp(name) / f"lib{name}.so"
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-o", str(so),
                               os.path.join(REPO, "tests", "native", name + ".cpp")])
        out.append(ctypes.CDLL(str(so)))
    out[0].bp_path.argtypes, out[0].bp_path.restype = [I64], ctypes.c_int
    out[1].bf_path.argtypes, out[1].bf_path.restype = [I64, I64], ctypes.c_int
    return out


def _bucket_plans(mc, c):
    """A budget call's buckets as cwq_greedy_encode_var and
    cwq_greedy_encode_uniform_var run them: the blocks of one bit count as a
    call of their own, with their own longest block; {bits: (path, rows_wave rule)}."""
    out = {}
    for b in sorted(set(c["bits"])):
        mine = [n for n, bb in zip(c["sizes"], c["bits"]) if bb == b]
        if c["d"] is not None:
            out[b] = (plan(mc, csr=False, ud=c["d"], bits=b, prune=2, nb=len(mine),
                           n_steps=c["n_steps"])[0], False)
        else:
            rule = bool(mc.mc_bucket_takes_rows_wave(b, sum(mine), len(mine), 2))
            out[b] = (plan(mc, csr=True, bits=b, prune=2, nb=len(mine), max_d=max(mine),
                           rows_wave=rule, n_steps=c["n_steps"])[0], rule)
    return out


@pytest.mark.parametrize("name", list(S.NEAR_TIE_CASES))
def test_near_tie_case_takes_its_path(mc, search_plans, name):
    c = S.NEAR_TIE_CASES[name]
    sizes, n_steps, nb = c["sizes"], c["n_steps"], len(c["sizes"])
    assert sum(1 for n in sizes if n > 0) >= S.NEAR_TIE_MIN_BLOCKS
    consts = (I64 * 3)()
    mc.mc_dispatch_consts(consts)
    coop_min_d, lds = consts[1], consts[2]
    if c["group"] in ("encode", "tau_guess"):
        want = ENCODE_PATHS[c["path"]]
        for prune in c.get("prune", (2,)):
            p = 2 if prune is None else prune
            if c["d"] is not None:
                whole = plan(mc, csr=False, ud=c["d"], bits=c["bits"], prune=p, nb=nb,
                             n_steps=n_steps)
                ranges = [whole]
                assert whole[3] == 1
            else:
                whole, ranges = csr_paths(mc, sizes, c["bits"], n_steps, prune=p)
            # prune_mode 0 is the exact kernel whatever the shape
            assert {r[0] for r in ranges + [whole]} == {EVAL if p == 0 else want}, (name, prune)
    if name == "tile_queue":
        assert (1 << c["bits"]) >= 4096 and nb > 1536 and c["oracle_stride"] == 16
    elif c["path"] == "uniform_pruned" and c["group"] != "var":
        assert nb <= 1536  # no tile queue
    if name == "csr_lane":
        assert max(sizes) < coop_min_d and 0 in sizes
        assert csr_paths(mc, sizes, c["bits"], n_steps)[0][3] == 3  # forked
    if name == "csr_coop":
        whole, ranges = csr_paths(mc, sizes, c["bits"], n_steps)
        assert whole[1] and all(r[1] for r in ranges)
        assert lds in sizes and any(n > lds for n in sizes) and any(n < coop_min_d for n in sizes)
        assert mc.mc_has_long_block_records(1, max(sizes), nb)
    if name.startswith("general"):
        assert mc.mc_has_screen_arrays(0, c["d"], nb)
    if c["group"] == "rows_wave":  # forced by the selftest entry, in every part
        whole = plan(mc, csr=True, bits=c["bits"], prune=2, nb=nb, max_d=max(sizes),
                     rows_wave=True, n_steps=n_steps)
        assert whole[0] == ROWS_WAVE
        for n in part_sizes(nb, whole[3]):
            assert plan(mc, csr=True, bits=c["bits"], prune=2, nb=n, max_d=max(sizes),
                        rows_wave=True, n_steps=n_steps)[0] == ROWS_WAVE
        assert 0 in sizes and max(sizes) == 4095
    if c["group"] == "var":
        assert len(c["bits"]) == nb
        buckets = _bucket_plans(mc, c)
        if c["path"] == "mixed":  # one call, every other path, no long bucket
            assert not any(rule for _, rule in buckets.values())
            assert {p for p, _ in buckets.values()} >= {EVAL, SMALL_PIPE, SMALL_THREE, CSR_PRUNED}
            assert 0 in c["bits"] and 0 in sizes
        else:
            assert {p for p, _ in buckets.values()} == {ENCODE_PATHS[c["path"]]}
            assert len(buckets) >= 4
        if c["path"] == "rows_wave":
            assert all(rule for _, rule in buckets.values())
    beam, backfit = search_plans
    if c["group"] in ("beam", "beam_var"):
        assert c["path"] == "beam_lane" and beam.bp_path(max(sizes)) == 0 and max(sizes) == 64
    if c["group"] in ("backfit", "backfit_var"):
        assert n_steps >= 2  # a code of one step is returned as given
        assert backfit.bf_path(max(sizes), nb) == (1 if c["path"] == "backfit_lane" else 0)


# ---------------------------------------------------------------------------
# test_graph_replay_gpu.py: each captured case takes the path it names, at
# every step count it runs with
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.GRAPH_CASES))
def test_graph_case_takes_its_path(mc, name):
    mc.mc_choose_tiling.argtypes = [I64, I64, ctypes.POINTER(I64)]
    mc.mc_choose_tiling.restype = None
    mc.mc_takes_tile_queue.argtypes = [I64, I64, I64]
    c = S.GRAPH_CASES[name]
    sizes, nb, bits = c["sizes"], len(c["sizes"]), c["bits"]
    want = ENCODE_PATHS[c["path"]]
    assert (want == EVAL) == (c["prune"] == 0 or c["path"] == "eval")
    assert S.GRAPH_STEPS == (1, 2, 3, 4)
    for n_steps in S.GRAPH_STEPS:
        if c["d"] is not None:
            whole = plan(mc, csr=False, ud=c["d"], bits=bits, prune=c["prune"], nb=nb,
                         n_steps=n_steps)
            assert whole == (want, c["path"] == "csr_pruned", False, 1), (name, n_steps)
        else:
            rw = c["entry"] == "rows_wave"
            whole = plan(mc, csr=True, bits=bits, prune=c["prune"], nb=nb, max_d=max(sizes),
                         rows_wave=rw, n_steps=n_steps)
            # a ragged call of several steps forks, a one-step call does not
            assert whole[3] == (1 if n_steps == 1 else min(3, nb)), (name, n_steps)
            for n in part_sizes(nb, whole[3]):
                part = plan(mc, csr=True, bits=bits, prune=c["prune"], nb=n, max_d=max(sizes),
                            rows_wave=rw, n_steps=n_steps)
                assert part[0] == want and part[2] == (want == SMALL_PIPE), (name, n_steps, n)
    consts = (I64 * 3)()
    mc.mc_dispatch_consts(consts)
    coop_min_d, lds = consts[1], consts[2]
    if name == "csr_lane":
        assert max(sizes) < coop_min_d and 0 in sizes
    if name == "csr_all":
        assert lds in sizes and any(n > lds for n in sizes) and any(n < coop_min_d for n in sizes)
        assert mc.mc_has_long_block_records(1, max(sizes), nb)
    if name.startswith("general"):
        assert mc.mc_has_screen_arrays(0, c["d"], nb)
    if "_x" in name:  # a few-block case's layout repeated
        base = S.GRAPH_CASES[name[:name.rindex("_x")]]
        k = int(name[name.rindex("_x") + 2:])
        assert sizes == base["sizes"] * k and nb >= S.GRAPH_MIN_BLOCKS > len(base["sizes"])
        assert {q: c[q] for q in c if q != "sizes"} == {q: base[q] for q in base if q != "sizes"}
    if c["entry"] == "rows_wave":
        assert sizes == S.ROWS_WAVE_LENGTHS[:8] and 0 in sizes and bits == 9
    if c["tiles"] is None:
        return
    # k_encode_prune's tiling (choose_tiling) and its queue (takes_tile_queue)
    assert c["d"] % 8 == 0 and 8 <= c["d"] <= 64 and not mc.mc_has_screen_arrays(0, c["d"], nb)
    t = (I64 * 4)()
    mc.mc_choose_tiling(nb, 1 << bits, t)
    tpb, cpt, min_cpt, grid = t[0], t[1], t[2], t[3]
    assert (min_cpt, grid) == (4096, 1536)
    if c["entry"] == "defer":
        # the selftest runs every block as one tile of its whole row count; the
        # screening-only form's queue grid is its 8 waves per SIMD: 2,048 slots
        # (deferral needs the screening pass: prune_mode 2; mode 0 is the single
        # launch, with the screening pass and, prune_mode 1, without it)
        assert c["defer"] in (0, 1, 2, 3) and c["prune"] in ((1, 2) if c["defer"] == 0 else (2,))
        assert (c["defer"] == 0) == name.startswith("prune_one_tile")
        tpb, cpt = 1, ((1 << bits) + 255) // 256 * 256
        grid = 256 * 8 if c["defer"] else t[3]
        assert (c["d"], bits, nb) == S.GRAPH_FAILURE_SHAPE
    queue = bool(mc.mc_takes_tile_queue(nb * tpb, cpt, grid))
    if c["tiles"] == "one":
        assert tpb == 1 and cpt >= 1 << bits and not queue
    elif c["tiles"] == "many":
        assert tpb > 1 and tpb * cpt == 1 << bits and not queue
    else:
        assert c["tiles"] == "queue"
        assert tpb == 1 and cpt >= min_cpt and nb * tpb > grid and queue
        # one tile fewer than the grid holds, or a smaller tile: no queue
        assert not mc.mc_takes_tile_queue(grid, cpt, grid)
        assert not mc.mc_takes_tile_queue(nb * tpb, min_cpt - 256, grid)
        assert c["oracle_stride"] == 16


def test_graph_cases_cover_the_recorded_failure():
    d, bits, nb = S.GRAPH_FAILURE_SHAPE
    assert (d, bits, nb) == (32, 12, 70)
    for m in (1, 2):
        c = S.GRAPH_CASES[f"prune_d32_nb70_mode{m}"]
        assert (c["d"], c["bits"], len(c["sizes"]), c["prune"]) == (d, bits, nb, m)
    assert 3 in S.GRAPH_STEPS and 4 in S.GRAPH_STEPS
    # one tile per block without the queue, in both pruning modes
    one = {c["prune"] for c in S.GRAPH_CASES.values() if c["tiles"] == "one" and not c.get("defer")}
    assert one == {1, 2}
