"""Shapes of tests/test_prune_refill_gpu.py, shared with
tests/test_refill_plan.py.  Uniform shapes are (d, bits, nb, n_steps), as in
tests/prune_tau_shapes.py, whose tiling() and MANY are used here.

A wave's share R is a quarter of its tile's candidates.  Its first S(R) rows
(csrc/cwq_refill.h: the largest multiple of 64 not above 7 R / 8, 0 below 128)
are handed out by stride, the rest by rank.  With MANY blocks a block is one
tile, so bits 8, 9, 10 and 12 give R = 64 (S = 0), 128 (S = 64: one static row
per lane), 256 (S = 192) and 1,024 (S = 896)."""
import prune_tau_shapes as P

MANY = P.MANY

SINGLE_TILE = [(d, bits, MANY, 1) for d in (8, 32, 64) for bits in (8, 9, 10, 12)] + \
              [(16, 10, MANY, 1)]
# fewer blocks: INTER tiles.  Four blocks in tiles of 256 candidates (S = 0);
# 64 blocks at 18 bits in tiles of 1,024 with tail tiles of 256, where later
# tiles start from the value in keys[g]
INTER = [(32, 12, 4, 1), (32, 16, 4, 1), (16, 18, 64, 1)]
ADVERSARIAL = (32, 10, MANY, 1)
MULTI_STEP = (32, 10, MANY, 3)

ALL = SINGLE_TILE + INTER + [ADVERSARIAL, MULTI_STEP]
ORACLE_STRIDE = 4096  # of MANY blocks the oracle codes every 4,096th and the last


def wave_share(nb, bits, tail_split=4):
    """Rows per wave in the full tiles of a launch and, where launch_prune_t
    cuts a block's last tiles in tail_split, in those."""
    tpb, cpt = P.tiling(nb, 1 << bits)
    out = [-(-cpt // 4)]
    if tpb >= 2 and cpt % (256 * tail_split) == 0:
        out.append(-(-(cpt // tail_split) // 4))
    return out
