"""Shapes of tests/test_prune_tau_gpu.py, shared with
tests/test_prune_tau_plan.py, which checks on the CPU that each takes the
uniform pruned kernel (k_encode_prune) in modes 1 and 2 and the exact kernel in
mode 0, and how choose_tiling cuts it.  Uniform shapes are (d, bits, nb,
n_steps), as in tests/encode_shapes.py.

choose_tiling aims at 16,384 tiles per launch, of at least 256 candidates: a
block is one tile when it has at most 256 candidates or the launch has at least
16,384 blocks (as tests/encode_shapes.py WS_TILE_QUEUE); with fewer blocks a
block of 2^12 candidates is cut into 16 tiles of 256, which run the INTER
instance of the kernel.  MANY is the block count that keeps a block whole."""
import encode_shapes as S

MANY = S.WS_TILE_QUEUE[2]
assert MANY == 16384

# one step, three tile sizes: 2^4 candidates, four rows per wave, so most
# lanes are never active; 2^8, one row per lane of each of the four waves
# (every row completes in the same iteration against tau = -inf: the all-lanes
# keep); 2^12 in one tile: refills, several shares of tau
ONE_STEP = [(d, bits, MANY if bits == 12 else 3, 1) for d in (8, 32, 64) for bits in (4, 8, 12)]
WORKLOAD_TILE = (32, 16, MANY, 1)      # C4's own tile: 2^16 candidates, one tile per block
WORKLOAD_BLOCKS = (32, 16, 4, 1)       # four C4 blocks alone: 256 tiles of 256 each
TWO_STEPS = (S.WS_UNIFORM_PRUNED[0], S.WS_UNIFORM_PRUNED[1], MANY, 2)  # STEP0 false in step 1
TWO_STEPS_INTER = (S.WS_UNIFORM_PRUNED[0], S.WS_UNIFORM_PRUNED[1], 5, 2)
# several tiles per block (INTER): 2^9 candidates are the fewest that make two
INTER_SMALLEST = (8, 9, 2, 1)
# ... and 2 x 4,096 tiles, one per workgroup of a grid of 8,192, of which 1,536
# are resident at a time: the later ones start from the value in keys[g]
INTER_SEEDED = (8, 20, 2, 1)
TIED = [(8, 12, MANY, 1), (32, 12, MANY, 1)]   # one tile of 4,096 > CWQ_SURVIVOR_CAP rows
NAN_BLOCK = (32, 12, 3, 1)
WORKSPACE = [(32, 8, 3, 1), (32, 12, 3, 1)]

MODES_CASES = ONE_STEP + [WORKLOAD_TILE, WORKLOAD_BLOCKS, TWO_STEPS, TWO_STEPS_INTER,
                          INTER_SMALLEST, INTER_SEEDED]
ALL = MODES_CASES + [NAN_BLOCK] + TIED + WORKSPACE
ONE_TILE = [s for s in ONE_STEP] + [WORKLOAD_TILE, TWO_STEPS] + TIED + [WORKSPACE[0]]
# the CPU oracle scores every candidate: of MANY blocks it takes every
# ORACLE_STRIDE-th and the last (the whole launch is compared with mode 0)
ORACLE_STRIDE = 4096


def tiling(nb, n_cand, target=16384):
    """csrc/cwq_dispatch.h choose_tiling: (tiles per block, candidates per tile)."""
    want = max(1, min(-(-target // nb), -(-n_cand // 256)))
    cpt = max(256, -(-(-(-n_cand // want)) // 256) * 256)
    return -(-n_cand // cpt), cpt
