"""The beam encoder under per-block bit budgets (include/cwq.h,
cwq_beam_encode_var), restated: block g is tests/beam_reference.py's
beam_block at ``n_bits[g]`` bits with block seed ``seed + block_id_base + g``
(int32 wrap), nothing more.  A helper of tests/test_beam_var_reference.py
(which holds it to the oracle's greedy coder at beam 1) and of
tests/test_beam_var_gpu.py; not a test, and nothing in the product imports it.
"""
import numpy as np

import beam_reference as R

F32 = np.float32


def beam_encode_var(O, t_loc, t_scale, p_loc, p_scale, block_off, n_bits, n_steps, seed, beam,
                    rho=1.0, block_id_base=0, blocks=None):
    """Blocks ``blocks`` (default: all) of a CSR layout, block g at ``n_bits[g]``
    bits per step.  Returns (idx int32 [nb, n_steps], sample f32 [D], value f32
    [nb]); rows of blocks not asked for stay 0."""
    off = np.asarray(block_off, np.int64)
    nb = off.size - 1
    bits = np.asarray(n_bits, np.int64).reshape(-1)
    assert bits.size == nb and bits.min(initial=0) >= 0 and bits.max(initial=0) <= 30
    tl, ts, pl, ps = (np.asarray(a, F32).reshape(-1) for a in (t_loc, t_scale, p_loc, p_scale))
    idx = np.zeros((nb, int(n_steps)), np.int32)
    sample = np.zeros(tl.size, F32)
    value = np.zeros(nb, F32)
    for g in (range(nb) if blocks is None else blocks):
        sl = slice(int(off[g]), int(off[g + 1]))
        idx[g], sample[sl], value[g] = R.beam_block(
            O, tl[sl], ts[sl], pl[sl], ps[sl], int(bits[g]), n_steps,
            R.wrap32(int(seed) + int(block_id_base) + g), beam, rho)
    return idx, sample, value
