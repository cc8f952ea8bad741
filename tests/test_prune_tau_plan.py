"""The shapes of tests/test_prune_tau_gpu.py on the host: each takes the uniform
pruned kernel in modes 1 and 2 and the exact kernel in mode 0
(csrc/cwq_dispatch.h, through the plan check of tests/test_encode_plan.py), and
the two INTER shapes are cut into the tiles their names say."""
import pytest

import prune_tau_shapes as P
from test_encode_plan import EVAL, UNIFORM_PRUNED, mc, plan  # noqa: F401  (mc: a fixture)


@pytest.mark.parametrize("shape", sorted(set(P.ALL)))
def test_shape_takes_uniform_pruned(mc, shape):
    d, bits, nb, n_steps = shape
    for prune in (1, 2):
        assert plan(mc, csr=False, ud=d, bits=bits, prune=prune, nb=nb, n_steps=n_steps) == \
            (UNIFORM_PRUNED, False, False, 1)
    assert plan(mc, csr=False, ud=d, bits=bits, prune=0, nb=nb, n_steps=n_steps)[0] == EVAL
    assert not mc.mc_has_screen_arrays(0, d, nb)


def test_tiles():
    """choose_tiling as launch_prune_t reads it: one tile per block launches
    k_encode_prune<D, STEP0, false>, more launch the INTER instance."""
    for d, bits, nb, _ in P.ONE_TILE:
        assert P.tiling(nb, 1 << bits) == (1, max(256, 1 << bits)), (d, bits, nb)
    for d, bits, nb, _ in (P.TWO_STEPS_INTER, P.NAN_BLOCK, P.WORKSPACE[1]):
        assert P.tiling(nb, 1 << bits) == (16, 256), (d, bits, nb)
    d, bits, nb, _ = P.WORKLOAD_BLOCKS
    assert P.tiling(nb, 1 << bits) == (256, 256)
    d, bits, nb, _ = P.INTER_SMALLEST
    assert P.tiling(nb, 1 << bits) == (2, 256)
    assert P.tiling(nb, 1 << (bits - 1))[0] == 1  # one bit fewer: a single tile
    d, bits, nb, _ = P.INTER_SEEDED
    tpb, cpt = P.tiling(nb, 1 << bits)
    assert (tpb, cpt) == (4096, 256) and nb * tpb > 4 * 1536
    # C4 itself: one tile of 2^16 candidates per block, as WORKLOAD_TILE
    assert P.tiling(1000000, 1 << 16) == (1, 1 << 16)
    # one block fewer than MANY and a block of 2^12 candidates is cut in two
    assert P.tiling(P.MANY - 1, 1 << 12)[0] == 2
    # the 2^4 and 2^8 tiles: four and 64 rows per wave
    assert {bits for _, bits, _, _ in P.ONE_STEP} == {4, 8, 12}
