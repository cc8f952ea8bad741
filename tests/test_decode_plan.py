"""The decode dispatch (csrc/cwq_dispatch.h decode_plan, DESIGN.md "Decode
dispatch") on the host: which kernel a launch_decode call of a given shape
takes, and with which lane mapping.

k_decode, k_decode_q4 and k_decode_q4_glds are bit-exact by design, so the GPU
tests, which compare outputs with the oracle, cannot see a shape being
rerouted.  These tests can: a table of shapes to kernels, every shape of
tests/test_decode_kernels_gpu.py against the kernel its case names, and the
conditions of the float4 kernels' lane mapping that those shapes have to meet
between them -- all evaluated through the plan itself (mc_decode_plan)."""
import ctypes

import pytest

import decode_shapes as S

GENERAL, Q4, Q4_GLDS = range(3)  # DecodeKernel's order
KERNEL = {S.GENERAL: GENERAL, S.Q4: Q4, S.Q4_GLDS: Q4_GLDS}
I64 = ctypes.c_int64


@pytest.fixture(scope="module")
def mc(mathcheck):
    mathcheck.mc_decode_plan.argtypes = [ctypes.c_int, I64, I64, I64, ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(I64)]
    mathcheck.mc_decode_plan.restype = None
    mathcheck.mc_decode_consts.argtypes = [ctypes.POINTER(I64)]
    mathcheck.mc_decode_consts.restype = None
    return mathcheck


def plan(mc, *, d=0, nb, n_steps=1, sizes=None, aligned=True):
    """(kernel, qpb, bpw, groups, workgroups) as launch_decode fills the shape:
    a uniform call has total_dims = nb * d, a ragged one ud = 0."""
    out = (I64 * 5)()
    if sizes is None:
        mc.mc_decode_plan(0, d, nb, nb * d, n_steps, int(aligned), out)
    else:
        assert nb == len(sizes)
        mc.mc_decode_plan(1, 0, nb, sum(sizes), n_steps, int(aligned), out)
    return tuple(out)


def consts(mc):
    c = (I64 * 3)()
    mc.mc_decode_consts(c)
    return tuple(c)


def test_default_build(mc):
    """The grid caps the kernels' strides are written for, and single-step
    codes on the LDS-ring kernel."""
    assert consts(mc) == (16384, 1 << 20, 1)


TABLE = [
    # uniform d % 4 == 0, d <= 256: the float4 kernels, by step count
    (dict(d=4, nb=3, n_steps=1), Q4_GLDS),
    (dict(d=4, nb=3, n_steps=2), Q4),
    (dict(d=32, nb=1000, n_steps=1), Q4_GLDS),
    (dict(d=32, nb=1000, n_steps=2), Q4),
    (dict(d=32, nb=1000, n_steps=1000), Q4),
    (dict(d=252, nb=3, n_steps=1), Q4_GLDS),
    (dict(d=256, nb=3, n_steps=1), Q4_GLDS),
    (dict(d=256, nb=3, n_steps=2), Q4),
    # past 256 dims, and lengths that are no multiple of 4
    (dict(d=260, nb=3, n_steps=1), GENERAL),
    (dict(d=260, nb=3, n_steps=2), GENERAL),
    (dict(d=1024, nb=3, n_steps=1), GENERAL),
    (dict(d=1, nb=3, n_steps=1), GENERAL),
    (dict(d=2, nb=3, n_steps=2), GENERAL),
    (dict(d=5, nb=3, n_steps=1), GENERAL),
    (dict(d=255, nb=3, n_steps=2), GENERAL),
    (dict(d=0, nb=3, n_steps=1), GENERAL),
    (dict(d=0, nb=3, n_steps=2), GENERAL),
    # float4 access needs 16-byte aligned arrays
    (dict(d=32, nb=1000, n_steps=1, aligned=False), GENERAL),
    (dict(d=32, nb=1000, n_steps=2, aligned=False), GENERAL),
    (dict(d=256, nb=3, n_steps=1, aligned=False), GENERAL),
    # ragged blocks, whatever their lengths
    (dict(sizes=[32] * 8, nb=8, n_steps=1), GENERAL),
    (dict(sizes=[32] * 8, nb=8, n_steps=2), GENERAL),
    (dict(sizes=[4], nb=1, n_steps=1), GENERAL),
    (dict(sizes=[0, 0], nb=2, n_steps=1), GENERAL),
]


@pytest.mark.parametrize("shape,kernel", TABLE)
def test_shape_takes_kernel(mc, shape, kernel):
    got, qpb, bpw, groups, wgs = plan(mc, **shape)
    assert got == kernel, shape
    assert wgs >= 1
    if kernel == GENERAL:
        assert (qpb, bpw, groups) == (0, 0, 0)
        total = sum(shape["sizes"]) if "sizes" in shape else shape["nb"] * shape["d"]
        assert wgs == min(max(-(-total // 256), 1), 16384)
    else:
        d, nb = shape["d"], shape["nb"]
        assert qpb == d // 4 and bpw == 64 // qpb and 1 <= bpw * qpb <= 64
        assert groups == -(-nb // (bpw * qpb)) and wgs == -(-groups // 4)  # a wave per group


def test_every_q4_length(mc):
    """Every d from 0 to 300: the float4 kernels exactly at the multiples of 4
    up to 256, and there a mapping that fits a wave."""
    for d in range(0, 301):
        for n_steps, want in ((1, Q4_GLDS), (2, Q4), (3, Q4)):
            k, qpb, bpw, groups, wgs = plan(mc, d=d, nb=70, n_steps=n_steps)
            if d % 4 == 0 and 4 <= d <= 256:
                assert k == want, (d, n_steps)
                assert 4 * qpb == d and bpw == 64 // qpb and 32 < bpw * qpb <= 64
            else:
                assert k == GENERAL, (d, n_steps)
            assert plan(mc, d=d, nb=70, n_steps=n_steps, aligned=False)[0] == GENERAL


def test_no_block_no_launch(mc):
    for nb in (0, -1):
        for d in (0, 5, 32):
            assert plan(mc, d=d, nb=nb)[4] == 0
    assert plan(mc, sizes=[], nb=0)[4] == 0


def test_grid_caps(mc):
    gen_cap, q4_cap, _ = consts(mc)
    # k_decode: one pass up to cap * 256 dims, its stride loop beyond
    nb = (gen_cap - 1) * 256 // 5
    assert plan(mc, d=5, nb=nb)[4] == -(-nb * 5 // 256) == gen_cap - 1
    nb = gen_cap * 256 // 5
    assert plan(mc, d=5, nb=nb)[4] == gen_cap and nb * 5 <= gen_cap * 256
    assert plan(mc, d=5, nb=nb + 1)[4] == gen_cap and (nb + 1) * 5 > gen_cap * 256
    assert plan(mc, d=5, nb=10 * nb)[4] == gen_cap
    # the float4 kernels: a wave per group of 64 blocks up to 4 * cap groups
    for n_steps in (1, 2):
        for d in (4, 256):
            nb = 64 * 4 * q4_cap
            assert plan(mc, d=d, nb=nb - 64, n_steps=n_steps)[3:] == (4 * q4_cap - 1, q4_cap)
            assert plan(mc, d=d, nb=nb - 4 * 64, n_steps=n_steps)[3:] == \
                (4 * q4_cap - 4, q4_cap - 1)
            assert plan(mc, d=d, nb=nb + 1, n_steps=n_steps)[3:] == (4 * q4_cap + 1, q4_cap)


# ---------------------------------------------------------------------------
# test_workspace_state_gpu.py's decoder cases: their comments, as assertions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,nb,n_steps", S.DECODE_CASES)
def test_workspace_state_decode_cases(mc, name, d, nb, n_steps):
    kernel, qpb, bpw = S.DECODE_CASES_PLAN[name]
    if nb is None:
        got = plan(mc, sizes=d, nb=len(d), n_steps=n_steps)
        assert 0 in d and any(n % 4 for n in d) and max(d) < 256
    else:
        got = plan(mc, d=d, nb=nb, n_steps=n_steps)
    assert got[:3] == (KERNEL[kernel], qpb, bpw), name
    if name.startswith("d12"):  # three Philox blocks per row, 21 rows per wave's chunk
        assert got[1:3] == (3, 21) and got[3:] == (1, 1) and nb < 63
    if name == "d36":  # nine per row, 63 of 64 lanes active
        assert got[1] == 9 and got[1] * got[2] == 63 and got[3:] == (1, 1) and nb < 63
    if name == "d256":  # a wave per row: three rows of one group, one workgroup
        assert got[1:3] == (64, 1) and got[3:] == (1, 1) and nb == 3
    assert {c[0] for c in S.DECODE_CASES} == set(S.DECODE_CASES_PLAN)


# ---------------------------------------------------------------------------
# test_decode_kernels_gpu.py: every case takes the kernel its row names
# ---------------------------------------------------------------------------
def test_q4_shape_table(mc):
    """The (d, qpb, bpw) rows of decode_shapes.Q4_DIMS are the plan's."""
    for d, qpb, bpw in S.Q4_DIMS + S.BAD_Q4_DIMS:
        for n_steps in (1, 3):
            assert plan(mc, d=d, nb=1, n_steps=n_steps)[1:3] == (qpb, bpw), d
    assert set(S.BAD_Q4_DIMS) <= set(S.Q4_DIMS)


@pytest.mark.parametrize("case", S.q4_cases(),
                         ids=lambda c: f"{c['what']}-d{c['d']}-nb{c['nb']}-s{c['n_steps']}")
def test_q4_case_takes_its_kernel(mc, case):
    got = plan(mc, d=case["d"], nb=case["nb"], n_steps=case["n_steps"])
    assert got[0] == KERNEL[case["kernel"]] and got[0] in (Q4, Q4_GLDS)
    assert case["nb"] * case["d"] <= 4_200_000


def _q4_plans(mc, kernel):
    """(case, qpb, bpw, B, groups, workgroups, blocks of the last group) of
    every GPU case on ``kernel``."""
    out = []
    for c in S.q4_cases():
        k, qpb, bpw, groups, wgs = plan(mc, d=c["d"], nb=c["nb"], n_steps=c["n_steps"])
        if k == kernel:
            B = qpb * bpw
            out.append((c, qpb, bpw, B, groups, wgs, c["nb"] - (groups - 1) * B))
    return out


CONDITIONS = {
    "qpb == 1 (a one-chunk ring)":
        lambda c, qpb, bpw, B, groups, wgs, last: qpb == 1,
    "bpw == 1 with qpb >= 33":
        lambda c, qpb, bpw, B, groups, wgs, last: bpw == 1 and qpb >= 33,
    "bpw == 1, every chunk of a group populated":
        lambda c, qpb, bpw, B, groups, wgs, last: bpw == 1 and qpb >= 33 and c["nb"] >= B,
    "all 64 lanes active (B == 64, a whole group)":
        lambda c, qpb, bpw, B, groups, wgs, last: B == 64 and c["nb"] >= B,
    "idle lanes, qpb no power of two":
        lambda c, qpb, bpw, B, groups, wgs, last: B < 64 and qpb & (qpb - 1) != 0,
    "groups > 4: a second workgroup":
        lambda c, qpb, bpw, B, groups, wgs, last: groups > 4 and wgs >= 2,
    "last group: a partial last chunk and a wholly empty one":
        lambda c, qpb, bpw, B, groups, wgs, last:
            c["nb"] % bpw != 0 and last % bpw != 0 and -(-last // bpw) < qpb and groups > 1,
    "nb < bpw":
        lambda c, qpb, bpw, B, groups, wgs, last: c["nb"] < bpw,
    "nb == B":
        lambda c, qpb, bpw, B, groups, wgs, last: c["nb"] == B and groups == 1,
    "nb == B + 1":
        lambda c, qpb, bpw, B, groups, wgs, last: c["nb"] == B + 1 and groups == 2 and last == 1,
    "counter past 2^32":
        lambda c, qpb, bpw, B, groups, wgs, last:
            c["what"] == "counter" and ((1 << 30) - 1) * qpb >= 1 << 32 and
            c["bits"] == 30 and groups == 2,
    "bad indices over six groups or more":
        lambda c, qpb, bpw, B, groups, wgs, last: c["what"] == "bad" and groups >= 6,
}


@pytest.mark.parametrize("kernel", [Q4, Q4_GLDS])
@pytest.mark.parametrize("cond", list(CONDITIONS))
def test_q4_cases_cover(mc, kernel, cond):
    """Each condition of the float4 lane mapping is met by at least one GPU
    case of each kernel."""
    met = [p[0] for p in _q4_plans(mc, kernel) if CONDITIONS[cond](*p)]
    assert met, f"no case of kernel {kernel} meets: {cond}"


@pytest.mark.parametrize("kernel", [Q4, Q4_GLDS])
def test_q4_cases_cover_every_shape(mc, kernel):
    """On each kernel every row of Q4_DIMS runs one block, a whole group, a
    group and a block, and six or seven groups in two workgroups whose last
    holds one full chunk and one block of the next."""
    plans = _q4_plans(mc, kernel)
    for d, qpb, bpw in S.Q4_DIMS:
        mine = [p for p in plans if p[0]["d"] == d and p[0]["what"] == "shape"]
        assert [p[0]["nb"] for p in mine] == S.q4_nbs(qpb, bpw), d
        assert [p[4] for p in mine][:3] == [1, 1, 2]
        c, _, _, B, groups, wgs, last = mine[3]
        # (qpb == 1: a group is one chunk, so the call is six whole groups and one block)
        assert (groups, last) == ((7, 1) if qpb == 1 else (6, bpw + 1)) and wgs == 2, d
    assert max(p[0]["nb"] * p[0]["d"] for p in plans) == 322 * 256


def test_counter_cases_pass_2_32():
    for d in S.COUNTER_DIMS:
        assert ((1 << S.COUNTER_BITS) - S.COUNTER_HIGH) * (d // 4) >= 1 << 32, d


@pytest.mark.parametrize("n_steps", S.GENERAL_STEPS)
def test_general_uniform_cases(mc, n_steps):
    for d, nb in S.GENERAL_UNIFORM:
        assert plan(mc, d=d, nb=nb, n_steps=n_steps)[0] == GENERAL, d
        assert plan(mc, d=d, nb=nb, n_steps=n_steps)[4] >= (2 if d * nb > 256 else 1)
    assert {d for d, _ in S.GENERAL_UNIFORM} == {1, 5, 13, 260}
    # d = 32 is the float4 kernels' unless an array is off its boundary
    d, nb = S.UNALIGNED_D, S.UNALIGNED_NB
    assert plan(mc, d=d, nb=nb, n_steps=n_steps)[0] == (Q4_GLDS if n_steps == 1 else Q4)
    assert plan(mc, d=d, nb=nb, n_steps=n_steps, aligned=False)[0] == GENERAL


def test_grid_stride_case(mc):
    """k_decode's second pass: the grid cap binds and 1,000 dims (to the next
    whole block) are left for it."""
    gen_cap = consts(mc)[0]
    d, nb = S.GRID_STRIDE_D, S.GRID_STRIDE_NB
    assert plan(mc, d=d, nb=nb)[::4] == (GENERAL, gen_cap)
    assert gen_cap * 256 + 1000 <= nb * d < gen_cap * 256 + 1000 + d
    assert nb * d <= 4_200_000


@pytest.mark.parametrize("n_steps", S.RAGGED_STEPS + S.BAD_STEPS)
def test_ragged_cases(mc, n_steps):
    for sizes in S.RAGGED_SIZES + [S.BAD_RAGGED_SIZES]:
        assert plan(mc, sizes=sizes, nb=len(sizes), n_steps=n_steps)[0] == GENERAL
    assert plan(mc, sizes=[70000], nb=1, n_steps=n_steps)[4] == -(-70000 // 256)


@pytest.mark.parametrize("d,qpb,bpw", S.BAD_Q4_DIMS)
def test_bad_index_blocks_spread_over_groups_and_chunks(mc, d, qpb, bpw):
    """The four blocks given an out-of-range index lie in four different
    groups, of two workgroups, and in different chunks of them."""
    nb = S.q4_nbs(qpb, bpw)[-1]
    for n_steps in S.BAD_STEPS:
        k, pq, pb, groups, wgs = plan(mc, d=d, nb=nb, n_steps=n_steps)
        assert k == (Q4_GLDS if n_steps == 1 else Q4) and (pq, pb) == (qpb, bpw)
        B = pq * pb
        blocks = S.bad_blocks_q4(pq, pb)
        assert len(set(blocks)) == 4 and blocks[-1] == nb - 1 and max(blocks) < nb
        grp = [b // B for b in blocks]
        chunk = [(b % B) // pb for b in blocks]
        assert len(set(grp)) == 4 and max(grp) == groups - 1
        assert len({g // 4 for g in grp}) == 2 == wgs  # a workgroup's four waves: four groups
        assert len(set(chunk)) >= 3 and pq - 1 in chunk and 0 in chunk
        steps = S.bad_steps(n_steps)
        assert steps[:3] == [0, n_steps // 2, n_steps - 1] and len(steps) == 4
    for d, nb in S.BAD_GENERAL_UNIFORM:
        assert plan(mc, d=d, nb=nb, n_steps=n_steps)[0] == GENERAL
        assert len(set(S.bad_blocks(nb))) == 4
    assert len(set(S.bad_blocks(len(S.BAD_RAGGED_SIZES)))) == 4
    assert all(S.BAD_RAGGED_SIZES[b] > 0 for b in S.bad_blocks(len(S.BAD_RAGGED_SIZES)))


# ---------------------------------------------------------------------------
# test_graph_replay_gpu.py: each captured decoder case takes the kernel it names
# ---------------------------------------------------------------------------
def test_graph_replay_decoder_cases(mc):
    import encode_shapes as E
    seen = set()
    for name, (enc, entry, family) in E.GRAPH_DECODE_CASES.items():
        c = E.GRAPH_CASES[enc]
        for n_steps in E.GRAPH_DECODE_STEPS:
            if entry == "uniform":
                k = plan(mc, d=c["d"], nb=len(c["sizes"]), n_steps=n_steps)[0]
            else:
                assert c["d"] is None
                k = plan(mc, nb=len(c["sizes"]), sizes=c["sizes"], n_steps=n_steps)[0]
            want = GENERAL if family == "general" else (Q4_GLDS if n_steps == 1 else Q4)
            assert k == want, (name, n_steps)
            seen.add(k)
    assert seen == {GENERAL, Q4, Q4_GLDS}
