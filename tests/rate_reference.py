"""The rate table's definition (include/cwq.h, cwq_rate_table) from the CPU
oracle: column b is ``oracle.greedy_encode`` at ``n_bits_per_step = b, n_steps =
1``, and the value is the winning row's log-density in the coder's arithmetic
(tests/beam_reference.py: TFP <= 0.7 form in float32, Eigen-order row sum, the
argmax key's clamp).  A helper of tests/test_rate_table_gpu.py and
tests/test_choose_bits_gpu.py; not a test, nothing in the product imports it.
"""
import numpy as np

import beam_reference as R

F32 = np.float32


def inputs(rng, D):
    tl = rng.standard_normal(D).astype(F32)
    ts = rng.uniform(0.3, 0.9, D).astype(F32)
    pl = (0.25 * rng.standard_normal(D)).astype(F32)
    ps = rng.uniform(0.8, 1.3, D).astype(F32)
    return tl, ts, pl, ps


def row_values(O, sample, t_loc, t_scale, off):
    """The key's value of each block's row ``sample[off[g]:off[g + 1]]``; an
    empty block's is +0, and a block whose value is -FLT_MAX has index 0."""
    tl, ts = np.asarray(t_loc, F32), np.asarray(t_scale, F32)
    cn = R.lognorms(O, ts)
    out = np.zeros(len(off) - 1, F32)
    with np.errstate(all="ignore"):
        z = (np.asarray(sample, F32) - tl) / ts
        lp = (F32(-0.5) * (z * z)) - cn
        for g in range(len(off) - 1):
            out[g] = R.keyed_values(R.eigen_rowsums(lp[None, off[g]:off[g + 1]]))[0]
    return out


def table(O, t_loc, t_scale, p_loc, p_scale, off, max_bits, seed, rho=1.0, block_id_base=0):
    """(idx int32 [nb, B + 1], value f32 [nb, B + 1])."""
    off = np.asarray(off, np.int64)
    nb = off.size - 1
    idx = np.zeros((nb, max_bits + 1), np.int32)
    value = np.zeros((nb, max_bits + 1), F32)
    for b in range(max_bits + 1):
        i, s = O.greedy_encode(t_loc, t_scale, p_loc, p_scale, off, b, 1, seed, rho=rho,
                               block_id_base=block_id_base)
        idx[:, b] = i[:, 0]
        value[:, b] = row_values(O, s, t_loc, t_scale, off)
    return idx, value


def choose_bits(value, lam, min_bits=0, max_bits=None):
    """cwq_choose_bits in NumPy: float64 multiply, then subtract; np.argmax takes
    the first (lowest b) of equal maxima."""
    v = np.asarray(value, F32)
    B = v.shape[1] - 1
    hi = B if max_bits is None else min(int(max_bits), B)
    b = np.arange(min_bits, hi + 1, dtype=np.float64)
    score = v[:, min_bits:hi + 1].astype(np.float64) - np.float64(lam) * b
    return (np.argmax(score, axis=1) + min_bits).astype(np.int32)
