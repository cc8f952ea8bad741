"""GPU: every path of the greedy block decoders (launch_decode: k_decode,
k_decode_q4, k_decode_q4_glds) against the CPU oracle, bit for bit.

The reference is oracle.greedy_decode on indices drawn uniformly from
[0, 2^bits) -- not an encoder's, whose finalize kernel shares the decoders'
lane mapping and seed helpers -- and every dim of every case is compared on
float32 bit patterns.  The shapes are tests/decode_shapes.py's;
tests/test_decode_plan.py checks on the CPU that each takes the kernel named
here and that together they reach every condition of the float4 kernels' lane
mapping (a second workgroup, partial and empty chunks, one chunk per group, one
block per chunk, the Philox counter past 2^32).  A wave's stride to a second
group needs more than 2^22 groups and is not reached here.
An index < 0 or >= 2^bits makes its block NaN and leaves the others alone
(include/cwq.h)."""
import numpy as np
import pytest
import torch

import decode_shapes as S
from test_decode_batch_gpu import _assert_bits_equal  # on _bits: NaNs as one pattern
from test_decode_plan import GENERAL, KERNEL, Q4, Q4_GLDS, mc, plan  # noqa: F401 (mc: a fixture)

pytestmark = pytest.mark.gpu

FILL = -7.0e30  # what the output holds on entry: no decoded value, and no NaN


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    C.coded_greedy_sampler.VERBOSE = False
    return C


def _wrap32(x):
    return int(np.int32(np.uint32(int(x) & 0xFFFFFFFF)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _inputs(rng, nb, n_steps, bits, D):
    """Uniform indices with 0 and 2^bits - 1 planted in the first and last
    block, p_loc ~ N(0, 1), p_scale ~ U(0.25, 3)."""
    idx = rng.integers(0, 1 << bits, (nb, n_steps)).astype(np.int32)
    idx[0, 0], idx[-1, -1] = 0, (1 << bits) - 1
    pl = rng.standard_normal(D).astype(np.float32)
    ps = rng.uniform(0.25, 3.0, D).astype(np.float32)
    return idx, pl, ps


def _assert_seed_wraps(seed, base, nb):
    """The call's block seeds seed + block_id_base + g need the int32 wrap."""
    if (seed, base) == S.SEED_BASES[0]:
        return
    s = [seed + base + g for g in range(nb)]
    assert all(not -2 ** 31 <= v < 2 ** 31 for v in s), (seed, base)
    if base >= 2 ** 32 - 8 and nb > 8:  # ... and pass zero inside the call
        w = [_wrap32(v) for v in s]
        assert -1 in w and 0 in w


def _decode(cwq, idx, pl, ps, bits, n_steps, seed, rho, base, **kw):
    """decode_blocks into an output prefilled with FILL."""
    out = torch.full((pl.size,), FILL, dtype=torch.float32, device="cuda")
    got = cwq.decode_blocks(_dev(idx), _dev(pl), _dev(ps), bits, n_steps, seed, rho=rho,
                            block_id_base=base, out_sample=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy()


# ---------------------------------------------------------------------------
# the float4 kernels on every lane mapping
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("run", S.Q4_RUNS, ids=lambda r: r["kernel"])
@pytest.mark.parametrize("d,qpb,bpw", S.Q4_DIMS)
def test_q4_shapes_vs_oracle(cwq, oracle, mc, d, qpb, bpw, run):
    n_steps, bits, rho = run["n_steps"], run["bits"], run["rho"]
    k0 = S.Q4_DIMS.index((d, qpb, bpw)) + S.Q4_RUNS.index(run)
    for k, nb in enumerate(S.q4_nbs(qpb, bpw)):
        assert plan(mc, d=d, nb=nb, n_steps=n_steps)[:3] == (KERNEL[run["kernel"]], qpb, bpw)
        seed, base = S.SEED_BASES[(k0 + k) % 3]
        _assert_seed_wraps(seed, base, nb)
        rng = np.random.Generator(np.random.PCG64(1000 * d + 10 * nb + n_steps))
        idx, pl, ps = _inputs(rng, nb, n_steps, bits, nb * d)
        off = np.arange(nb + 1, dtype=np.int64) * d
        want = oracle.greedy_decode(idx, pl, ps, off, bits, n_steps, _wrap32(seed), rho, base)
        got = _decode(cwq, idx, pl, ps, bits, n_steps, seed, rho, base, block_dim=d)
        _assert_bits_equal(got, want, f"d={d} nb={nb} steps={n_steps} seed={seed} base={base}")


def test_seed_rotation_reaches_every_kernel():
    """Each (seed, block_id_base) pair meets both float4 kernels at the
    multi-group size."""
    for r, run in enumerate(S.Q4_RUNS):
        seen = {(i + r + 3) % 3 for i in range(len(S.Q4_DIMS))}  # k = 3: the last nb
        assert seen == {0, 1, 2}, run["kernel"]


@pytest.mark.parametrize("n_steps", S.COUNTER_STEPS)
@pytest.mark.parametrize("d", S.COUNTER_DIMS)
def test_q4_philox_counter_passes_2_32(cwq, oracle, mc, d, n_steps):
    """Rows whose Philox block counter n * qpb + q lies past 2^32 (TF's 128-bit
    counter carries into its second word), beside rows below it."""
    bits, rho, (seed, base) = S.COUNTER_BITS, 0.9, S.SEED_BASES[1]
    k, qpb, bpw, groups, _ = plan(mc, d=d, nb=1, n_steps=n_steps)
    nb = bpw * qpb + 1
    assert plan(mc, d=d, nb=nb, n_steps=n_steps)[0] == (Q4_GLDS if n_steps == 1 else Q4)
    rng = np.random.Generator(np.random.PCG64(77 + d + n_steps))
    idx, pl, ps = _inputs(rng, nb, n_steps, bits, nb * d)
    # half the indices in the last rows: the planted 2^30 - 1 and a random
    # choice of the others (the planted 0 stays)
    N = nb * n_steps
    high = np.zeros(N, bool)
    high[rng.permutation(np.arange(1, N - 1))[:N // 2 - 1]] = True
    high[N - 1] = True
    high = high.reshape(nb, n_steps)
    idx[high] = rng.integers((1 << bits) - S.COUNTER_HIGH, 1 << bits, int(high.sum()))
    idx[-1, -1] = (1 << bits) - 1
    assert int(high.sum()) == N // 2
    assert (idx[high] >= (1 << bits) - S.COUNTER_HIGH).all()
    assert (idx[high].astype(np.int64) * qpb >= 1 << 32).all()
    assert (idx[~high].astype(np.int64) * qpb + qpb < 1 << 32).any()
    off = np.arange(nb + 1, dtype=np.int64) * d
    want = oracle.greedy_decode(idx, pl, ps, off, bits, n_steps, _wrap32(seed), rho, base)
    got = _decode(cwq, idx, pl, ps, bits, n_steps, seed, rho, base, block_dim=d)
    _assert_bits_equal(got, want, f"d={d} steps={n_steps}")


# ---------------------------------------------------------------------------
# uniform calls that k_decode takes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", S.GENERAL_STEPS)
@pytest.mark.parametrize("d,nb", S.GENERAL_UNIFORM)
def test_uniform_general_vs_oracle(cwq, oracle, mc, d, nb, n_steps):
    bits, rho = 10, 0.8
    seed, base = S.SEED_BASES[(d + n_steps) % 3]
    _assert_seed_wraps(seed, base, nb)
    assert plan(mc, d=d, nb=nb, n_steps=n_steps)[0] == GENERAL
    rng = np.random.Generator(np.random.PCG64(500 + d + n_steps))
    idx, pl, ps = _inputs(rng, nb, n_steps, bits, nb * d)
    off = np.arange(nb + 1, dtype=np.int64) * d
    want = oracle.greedy_decode(idx, pl, ps, off, bits, n_steps, _wrap32(seed), rho, base)
    got = _decode(cwq, idx, pl, ps, bits, n_steps, seed, rho, base, block_dim=d)
    _assert_bits_equal(got, want, f"d={d} nb={nb} steps={n_steps}")


@pytest.mark.parametrize("n_steps", S.GENERAL_STEPS)
@pytest.mark.parametrize("which", S.UNALIGNED_WHICH)
def test_uniform_unaligned_takes_general_vs_oracle(cwq, oracle, mc, which, n_steps):
    """d = 32 with exactly one array one float past a 16-byte boundary."""
    d, nb, bits, rho = S.UNALIGNED_D, S.UNALIGNED_NB, 10, 0.8
    seed, base = S.SEED_BASES[(S.UNALIGNED_WHICH.index(which) + n_steps) % 3]
    _assert_seed_wraps(seed, base, nb)
    D = nb * d
    rng = np.random.Generator(np.random.PCG64(600 + n_steps + len(which)))
    idx, pl, ps = _inputs(rng, nb, n_steps, bits, D)
    arrs = {}
    for name, a in (("p_loc", pl), ("p_scale", ps), ("out_sample", np.full(D, FILL, np.float32))):
        if name == which:
            t = torch.empty(D + 1, dtype=torch.float32, device="cuda")[1:]
            t.copy_(torch.from_numpy(a))
        else:
            t = _dev(a)
        arrs[name] = t
    off16 = {name: t.data_ptr() % 16 for name, t in arrs.items()}
    assert off16 == {name: (4 if name == which else 0) for name in arrs}
    assert plan(mc, d=d, nb=nb, n_steps=n_steps, aligned=not any(off16.values()))[0] == GENERAL
    got = cwq.decode_blocks(_dev(idx), arrs["p_loc"], arrs["p_scale"], bits, n_steps, seed,
                            rho=rho, block_id_base=base, block_dim=d,
                            out_sample=arrs["out_sample"])
    assert got.data_ptr() == arrs["out_sample"].data_ptr()  # the wrapper passed the view on
    off = np.arange(nb + 1, dtype=np.int64) * d
    want = oracle.greedy_decode(idx, pl, ps, off, bits, n_steps, _wrap32(seed), rho, base)
    _assert_bits_equal(got.cpu().numpy(), want, f"{which} unaligned, steps={n_steps}")


def test_general_grid_stride_second_pass_vs_oracle(cwq, oracle, mc):
    """k_decode past its grid cap: the threads of the first 1,001 dims take a
    second element 16,384 * 256 dims on."""
    d, nb, bits, n_steps, rho = S.GRID_STRIDE_D, S.GRID_STRIDE_NB, 10, 1, 1.0
    seed, base = S.SEED_BASES[2]
    _assert_seed_wraps(seed, base, nb)
    assert plan(mc, d=d, nb=nb, n_steps=n_steps)[::4] == (GENERAL, 16384)
    assert nb * d > 16384 * 256
    rng = np.random.Generator(np.random.PCG64(700))
    idx, pl, ps = _inputs(rng, nb, n_steps, bits, nb * d)
    off = np.arange(nb + 1, dtype=np.int64) * d
    want = oracle.greedy_decode(idx, pl, ps, off, bits, n_steps, _wrap32(seed), rho, base)
    got = _decode(cwq, idx, pl, ps, bits, n_steps, seed, rho, base, block_dim=d)
    _assert_bits_equal(got, want, "grid-stride second pass")


# ---------------------------------------------------------------------------
# ragged calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", S.RAGGED_STEPS)
@pytest.mark.parametrize("sizes", S.RAGGED_SIZES, ids=["empties", "one_long"])
def test_ragged_vs_oracle(cwq, oracle, mc, sizes, n_steps):
    bits, rho = 10, 0.8
    seed, base = S.SEED_BASES[(len(sizes) + n_steps) % 3]
    nb, off = len(sizes), _offsets(sizes)
    _assert_seed_wraps(seed, base, nb)
    assert plan(mc, sizes=sizes, nb=nb, n_steps=n_steps)[0] == GENERAL
    rng = np.random.Generator(np.random.PCG64(800 + nb + n_steps))
    idx, pl, ps = _inputs(rng, nb, n_steps, bits, int(off[-1]))
    want = oracle.greedy_decode(idx, pl, ps, off, bits, n_steps, _wrap32(seed), rho, base)
    got = _decode(cwq, idx, pl, ps, bits, n_steps, seed, rho, base, block_off=off)
    _assert_bits_equal(got, want, f"sizes={sizes} steps={n_steps}")


# ---------------------------------------------------------------------------
# out-of-range indices: the block is NaN, every other block untouched
# ---------------------------------------------------------------------------
def _bad_case(oracle, sizes, blocks, n_steps, seed, base, rho, rng_seed):
    """Inputs with the four bad indices planted, and the expected output: the
    oracle's with those indices replaced by 0, NaN in the four blocks."""
    bits = S.BAD_BITS
    nb, off = len(sizes), _offsets(sizes)
    rng = np.random.Generator(np.random.PCG64(rng_seed))
    idx, pl, ps = _inputs(rng, nb, n_steps, bits, int(off[-1]))
    clean = idx.copy()
    assert len(set(blocks)) == 4 and blocks[-1] == nb - 1
    for b, s, v in zip(blocks, S.bad_steps(n_steps), S.BAD_INDICES):
        idx[b, s], clean[b, s] = v, 0
    assert sorted(idx[(idx < 0) | (idx >= 1 << bits)].tolist()) == sorted(S.BAD_INDICES)
    want = oracle.greedy_decode(clean, pl, ps, off, bits, n_steps, _wrap32(seed), rho, base)
    assert not np.isnan(want).any()
    bad_dims = np.zeros(int(off[-1]), bool)
    for b in blocks:
        assert off[b + 1] > off[b]
        bad_dims[off[b]:off[b + 1]] = True
    want[bad_dims] = np.nan
    return idx, pl, ps, off, want, bad_dims


def _check_bad(got, want, bad_dims, what):
    assert np.isnan(got[bad_dims]).all(), f"{what}: a dim of a bad block is not NaN"
    assert not np.isnan(got[~bad_dims]).any(), f"{what}: NaN outside the bad blocks"
    _assert_bits_equal(got, want, what)  # every dim: NaNs as one pattern, the rest as the oracle


@pytest.mark.parametrize("n_steps", S.BAD_STEPS)
@pytest.mark.parametrize("d,qpb,bpw", S.BAD_Q4_DIMS)
def test_q4_out_of_range_indices(cwq, cwqlib, oracle, mc, d, qpb, bpw, n_steps):
    """k_decode_q4_glds (one step) and k_decode_q4 (three), through the wrapper
    and through the C ABI itself."""
    nb = S.q4_nbs(qpb, bpw)[-1]
    want_kernel = Q4_GLDS if n_steps == 1 else Q4
    k, pq, pb, groups, wgs = plan(mc, d=d, nb=nb, n_steps=n_steps)
    assert (k, pq, pb, wgs) == (want_kernel, qpb, bpw, 2)
    blocks = S.bad_blocks_q4(qpb, bpw)
    B = qpb * bpw
    assert len({b // B for b in blocks}) == 4  # four groups ...
    assert len({(b % B) // bpw for b in blocks}) >= 3  # ... and different chunks of them
    seed, base, rho = 2147483647, 123, 0.7
    idx, pl, ps, off, want, bad_dims = _bad_case(oracle, [d] * nb, blocks, n_steps, seed, base,
                                                 rho, 900 + d + n_steps)
    got = _decode(cwq, idx, pl, ps, S.BAD_BITS, n_steps, seed, rho, base, block_dim=d)
    _check_bad(got, want, bad_dims, f"d={d} steps={n_steps}")
    # the C ABI: CWQ_OK and the same output
    idxd, pld, psd = _dev(idx.reshape(-1)), _dev(pl), _dev(ps)
    out = torch.full((nb * d,), FILL, dtype=torch.float32, device="cuda")
    assert all(t.data_ptr() % 16 == 0 for t in (pld, psd, out))
    rc = cwqlib.cwq_greedy_decode_uniform(idxd.data_ptr(), pld.data_ptr(), psd.data_ptr(), nb, d,
                                          S.BAD_BITS, n_steps, _wrap32(seed), rho, base,
                                          out.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, cwqlib.cwq_last_error()
    torch.cuda.synchronize()
    _check_bad(out.cpu().numpy(), want, bad_dims, f"C ABI d={d} steps={n_steps}")


@pytest.mark.parametrize("n_steps", S.BAD_STEPS)
@pytest.mark.parametrize("d,nb", S.BAD_GENERAL_UNIFORM)
def test_general_uniform_out_of_range_indices(cwq, cwqlib, oracle, mc, d, nb, n_steps):
    assert plan(mc, d=d, nb=nb, n_steps=n_steps)[0] == GENERAL
    seed, base, rho = -5, 2 ** 32 - 3, 0.7
    idx, pl, ps, off, want, bad_dims = _bad_case(oracle, [d] * nb, S.bad_blocks(nb), n_steps, seed,
                                                 base, rho, 950 + d + n_steps)
    got = _decode(cwq, idx, pl, ps, S.BAD_BITS, n_steps, seed, rho, base, block_dim=d)
    _check_bad(got, want, bad_dims, f"d={d} steps={n_steps}")
    idxd, pld, psd = _dev(idx.reshape(-1)), _dev(pl), _dev(ps)
    out = torch.full((nb * d,), FILL, dtype=torch.float32, device="cuda")
    rc = cwqlib.cwq_greedy_decode_uniform(idxd.data_ptr(), pld.data_ptr(), psd.data_ptr(), nb, d,
                                          S.BAD_BITS, n_steps, _wrap32(seed), rho, base,
                                          out.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, cwqlib.cwq_last_error()
    torch.cuda.synchronize()
    _check_bad(out.cpu().numpy(), want, bad_dims, f"C ABI d={d} steps={n_steps}")


@pytest.mark.parametrize("n_steps", S.BAD_STEPS)
def test_ragged_out_of_range_indices(cwq, cwqlib, oracle, mc, n_steps):
    sizes = S.BAD_RAGGED_SIZES
    nb = len(sizes)
    assert plan(mc, sizes=sizes, nb=nb, n_steps=n_steps)[0] == GENERAL
    seed, base, rho = 42, 0, 0.7
    idx, pl, ps, off, want, bad_dims = _bad_case(oracle, sizes, S.bad_blocks(nb), n_steps, seed,
                                                 base, rho, 990 + n_steps)
    got = _decode(cwq, idx, pl, ps, S.BAD_BITS, n_steps, seed, rho, base, block_off=off)
    _check_bad(got, want, bad_dims, f"ragged steps={n_steps}")
    idxd, pld, psd, offd = _dev(idx.reshape(-1)), _dev(pl), _dev(ps), _dev(off)
    out = torch.full((int(off[-1]),), FILL, dtype=torch.float32, device="cuda")
    rc = cwqlib.cwq_greedy_decode(idxd.data_ptr(), pld.data_ptr(), psd.data_ptr(),
                                  offd.data_ptr(), nb, int(off[-1]), max(sizes), S.BAD_BITS,
                                  n_steps, seed, rho, base, out.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, cwqlib.cwq_last_error()
    torch.cuda.synchronize()
    _check_bad(out.cpu().numpy(), want, bad_dims, f"C ABI ragged steps={n_steps}")
