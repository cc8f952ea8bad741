"""NumPy restatement of the beam encoder's definition (include/cwq.h,
cwq_beam_encode), built from the CPU oracle's pieces.  A helper of
tests/test_beam_reference.py (which holds it to the oracle's greedy coder at
beam 1 and to the oracle's decoder above) and of tests/test_beam_gpu.py; not
a test, and nothing in the product imports it.

Per block and step: the rows come from oracle.stateless_normal_sample on the
shard constants (the stream the greedy coder draws), every live beam's sum is
added to every row in float32, the log-density is the TFP <= 0.7 form in
float32 NumPy operations (one IEEE operation each, so NumPy's results are the
reference's), the row sum runs in the Eigen AVX order (eight strided
accumulators added packet by packet, a scalar tail, t + ((q0+q2)+(q1+q3)):
bit-equal to oracle.eigen_rowsum, which test_beam_reference.py checks), NaN and
values <= -FLT_MAX become -FLT_MAX, -0 becomes +0, and np.lexsort on (index,
-value) takes the L' best candidates, the lower index first among equals.
"""
import numpy as np

F32 = np.float32
LOWEST = F32(-3.4028234663852886e38)  # -FLT_MAX


def wrap32(x):
    return int(np.int32(np.uint32(int(x) & 0xFFFFFFFF)))


def shard_constants(p_loc, p_scale, n_steps, rho):
    """oracle shard_params: loc / n_steps, (rho * scale) / float32(sqrt(n_steps))."""
    nst = F32(n_steps)
    sdiv = F32(np.sqrt(np.float64(n_steps)))
    loc_s = (np.asarray(p_loc, F32) / nst).astype(F32)
    rs = (F32(rho) * np.asarray(p_scale, F32)).astype(F32)
    return loc_s, (rs / sdiv).astype(F32)


def lognorms(O, t_scale):
    L = O.lib()
    return np.array([L.cwqo_log_normalization(float(s)) for s in np.asarray(t_scale, F32)],
                    dtype=F32)


def eigen_rowsums(x):
    """The Eigen 3.3 AVX inner-dim sum of every row of x [M, d], float32."""
    x = np.asarray(x, F32)
    M, d = x.shape
    vec = (d // 8) * 8
    p = np.zeros((M, 8), F32)
    for j in range(0, vec, 8):
        p = p + x[:, j:j + 8]
    t = np.zeros(M, F32)
    for j in range(vec, d):
        t = t + x[:, j]
    q0, q1, q2, q3 = p[:, 0] + p[:, 4], p[:, 1] + p[:, 5], p[:, 2] + p[:, 6], p[:, 3] + p[:, 7]
    return t + ((q0 + q2) + (q1 + q3))


def keyed_values(v):
    """The value a candidate's key holds: NaN and <= -FLT_MAX -> -FLT_MAX, -0 -> +0."""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        v = np.where(v > LOWEST, v, LOWEST).astype(F32)
        return (v + F32(0.0)).astype(F32)


def beam_block(O, t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, block_seed, beam, rho=1.0):
    """One block.  Returns (indices int32 [n_steps], sample f32 [d], value f32)."""
    tl, ts = np.asarray(t_loc, F32), np.asarray(t_scale, F32)
    d = tl.size
    N = 1 << int(n_bits)
    loc_s, scale_s = shard_constants(p_loc, p_scale, n_steps, rho)
    cn = lognorms(O, ts)
    best = np.zeros((1, d), F32)
    paths = np.zeros((1, 0), np.int32)
    value = F32(0.0)
    with np.errstate(all="ignore"):
        for i in range(int(n_steps)):
            if d:
                rows = O.stateless_normal_sample(loc_s, scale_s, N, wrap32(1000 * block_seed + i))
            else:
                rows = np.zeros((N, 0), F32)
            L = best.shape[0]
            x = (best[:, None, :] + rows[None, :, :]).reshape(L * N, d)  # c = k N + r
            z = (x - tl) / ts
            lp = (F32(-0.5) * (z * z)) - cn
            v = keyed_values(eigen_rowsums(lp))
            keep = min(int(beam), L * N)
            order = np.lexsort((np.arange(L * N), -v))[:keep]
            par, r = order // N, order % N
            best = (best[par] + rows[r]).astype(F32)
            paths = np.concatenate([paths[par], r[:, None].astype(np.int32)], axis=1)
            value = v[order[0]]
    return paths[0], best[0], value


def beam_encode(O, t_loc, t_scale, p_loc, p_scale, block_off, n_bits, n_steps, seed, beam,
                rho=1.0, block_id_base=0, blocks=None):
    """Blocks ``blocks`` (default: all) of a CSR layout, block g with seed
    ``seed + block_id_base + g`` (int32 wrap).  Returns (idx int32 [nb, n_steps],
    sample f32 [D], value f32 [nb]); rows of blocks not asked for stay 0."""
    off = np.asarray(block_off, np.int64)
    nb = off.size - 1
    tl, ts, pl, ps = (np.asarray(a, F32).reshape(-1) for a in (t_loc, t_scale, p_loc, p_scale))
    idx = np.zeros((nb, int(n_steps)), np.int32)
    sample = np.zeros(tl.size, F32)
    value = np.zeros(nb, F32)
    for g in (range(nb) if blocks is None else blocks):
        sl = slice(int(off[g]), int(off[g + 1]))
        idx[g], sample[sl], value[g] = beam_block(
            O, tl[sl], ts[sl], pl[sl], ps[sl], n_bits, n_steps,
            wrap32(int(seed) + int(block_id_base) + g), beam, rho)
    return idx, sample, value
