"""NumPy restatement of backfitting's definition (include/cwq.h,
cwq_greedy_backfit), built from the CPU oracle's pieces the way
tests/beam_reference.py is.  A helper of tests/test_backfit_reference.py (which
holds it to the oracle's greedy coder and decoder) and of
tests/test_backfit_gpu.py; not a test, and nothing in the product imports it.

Per block: the rows of every step come from oracle.stateless_normal_sample on
the shard constants (the stream the greedy coder draws), dec(idx) adds the
selected rows to +0 in step order in float32, val() is beam_reference's
keyed_values(eigen_rowsums(log-density)), and a sweep is the four numbered
steps of the definition, literally.
"""
import numpy as np

import beam_reference as R

F32 = np.float32


class Block:
    """One block's streams and constants; rows are drawn once per step."""

    def __init__(self, O, t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, block_seed, rho=1.0):
        self.tl, self.ts = np.asarray(t_loc, F32), np.asarray(t_scale, F32)
        self.d = self.tl.size
        self.N = 1 << int(n_bits)
        self.n_steps = int(n_steps)
        loc_s, scale_s = R.shard_constants(p_loc, p_scale, n_steps, rho)
        self.cn = R.lognorms(O, self.ts)
        self.rows = []
        for i in range(self.n_steps):
            if self.d:
                self.rows.append(O.stateless_normal_sample(loc_s, scale_s, self.N,
                                                           R.wrap32(1000 * block_seed + i)))
            else:
                self.rows.append(np.zeros((self.N, 0), F32))

    def dec(self, idx, skip=None):
        """((+0 + row(0, idx_0)) + row(1, idx_1)) + ..., step `skip` left out."""
        x = np.zeros(self.d, F32)
        for i in range(self.n_steps):
            if i != skip:
                x = (x + self.rows[i][int(idx[i])]).astype(F32)
        return x

    def val(self, x):
        """The keyed value of every row of x [M, d]."""
        with np.errstate(all="ignore"):
            z = (np.asarray(x, F32) - self.tl) / self.ts
            lp = (F32(-0.5) * (z * z)) - self.cn
            return R.keyed_values(R.eigen_rowsums(lp))

    def sweep(self, idx, v):
        """One sweep from (idx, v).  Returns (idx, v, accepted steps)."""
        idx = np.array(idx, np.int32)
        accepted = []
        for s in range(self.n_steps):
            base = self.dec(idx, skip=s)
            with np.errstate(all="ignore"):
                vals = self.val((base[None, :] + self.rows[s]).astype(F32))
            r = int(np.lexsort((np.arange(self.N), -vals))[0])  # the lowest index among equals
            if r == int(idx[s]):
                continue
            cand = idx.copy()
            cand[s] = r
            v2 = self.val(self.dec(cand)[None, :])[0]
            if v2 > v:
                idx, v = cand, v2
                accepted.append(s)
        return idx, v, accepted


def backfit_block(O, idx, t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, block_seed, sweeps,
                  rho=1.0):
    """One block.  Returns (idx int32 [n_steps], sample f32 [d], value f32 per
    sweep [sweeps + 1] (entry 0: the starting table's), accepted steps per sweep)."""
    b = Block(O, t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, block_seed, rho)
    idx = np.array(idx, np.int32)
    v = b.val(b.dec(idx)[None, :])[0]
    values, steps = [v], []
    for _ in range(int(sweeps) if int(n_steps) > 1 else 0):  # one step: returned as given
        idx, v, acc = b.sweep(idx, v)
        values.append(v)
        steps.append(acc)
    while len(values) < int(sweeps) + 1:
        values.append(v)
        steps.append([])
    return idx, b.dec(idx), np.array(values, F32), steps


def backfit(O, idx, t_loc, t_scale, p_loc, p_scale, block_off, n_bits, n_steps, seed, sweeps,
            rho=1.0, block_id_base=0, blocks=None):
    """Blocks ``blocks`` (default: all) of a CSR layout, block g with seed
    ``seed + block_id_base + g`` (int32 wrap), from the table idx [nb, n_steps].
    Returns (idx, sample f32 [D], values f32 [nb, sweeps + 1], accepted int32
    [nb], steps: {g: accepted steps per sweep}); rows of blocks not asked for
    stay 0."""
    off = np.asarray(block_off, np.int64)
    nb = off.size - 1
    tl, ts, pl, ps = (np.asarray(a, F32).reshape(-1) for a in (t_loc, t_scale, p_loc, p_scale))
    idx = np.asarray(idx, np.int32).reshape(nb, int(n_steps))
    out = np.zeros_like(idx)
    sample = np.zeros(tl.size, F32)
    values = np.zeros((nb, int(sweeps) + 1), F32)
    accepted = np.zeros(nb, np.int32)
    steps = {}
    for g in (range(nb) if blocks is None else blocks):
        sl = slice(int(off[g]), int(off[g + 1]))
        out[g], sample[sl], values[g], st = backfit_block(
            O, idx[g], tl[sl], ts[sl], pl[sl], ps[sl], n_bits, n_steps,
            R.wrap32(int(seed) + int(block_id_base) + g), sweeps, rho)
        accepted[g] = sum(len(a) for a in st)
        steps[g] = st
    return out, sample, values, accepted, steps
