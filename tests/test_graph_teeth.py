"""Which captured encoder cases can see a key left over from the step before
(CPU; DESIGN.md 2, "Teeth").

A library whose encode_steps skips the reset of ``keys`` before step 2 (the
third step) enters that step with step 1's keys.  The stale key of a block
survives the step's atomicMax, and the block's index and sample come out
wrong, exactly when the block's best value of step 2 lies below its best value
of step 1.  Whether a case has such a block is a property of its inputs alone:
it is computed here from tests/beam_reference.py's restatement of a step (beam
1: the greedy coder, held to the oracle by tests/test_beam_reference.py), and
must equal what that library did on the GPU, case by case, as recorded below
from its one run.  The small pipeline keeps its argmax out of ``keys`` and
passes whatever its values do.
"""
import functools

import numpy as np
import pytest

import beam_reference as R
import encode_shapes as S

# test_encoder_replays[name-n_steps] of tests/test_graph_replay_gpu.py that
# PASSED on the library without the reset before step 2; the other 46 of the
# 58 cases at three and four steps failed, and all 58 cases at one and two
# steps passed.
PASSED_WITHOUT_THE_RESET = {
    ("small_pipe", 3), ("small_pipe", 4),
    ("general_d5", 3), ("general_d5", 4), ("general_d5_x3", 3), ("general_d5_x3", 4),
    ("general_d100", 4), ("general_d100_x8", 4), ("prune_inter", 4), ("prune_inter_x4", 4),
    ("exact_ragged", 3), ("small_three", 3),
}
SCAN_BLOCKS = 64  # of a case with thousands of blocks: enough to find one


def step_values(O, tl, ts, pl, ps, n_bits, n_steps, block_seed, rho, upto):
    """The greedy coder's best value of steps 0 .. upto of one block."""
    F32 = R.F32
    loc_s, scale_s = R.shard_constants(pl, ps, n_steps, rho)
    cn = R.lognorms(O, ts)
    best = np.zeros(tl.size, F32)
    out = []
    with np.errstate(all="ignore"):
        for i in range(upto + 1):
            rows = O.stateless_normal_sample(loc_s, scale_s, 1 << n_bits,
                                             R.wrap32(1000 * block_seed + i))
            x = best[None, :] + rows
            z = (x - tl) / ts
            v = R.keyed_values(R.eigen_rowsums((F32(-0.5) * (z * z)) - cn))
            r = int(np.lexsort((np.arange(v.size), -v))[0])
            best = (best + rows[r]).astype(F32)
            out.append(v[r])
    return out


@functools.lru_cache(maxsize=None)
def falling_block(name, n_steps):
    """The first block whose best value falls from step 1 to step 2, or None;
    and whether any block scanned has the two equal (then the index decides)."""
    from oracle import oracle as O
    O.build()
    from test_graph_replay_gpu import BASE, RHO, SEED, _enc_inputs
    c = S.GRAPH_CASES[name]
    off, (tl, ts, pl, ps) = _enc_inputs(name)
    equal = False
    for g in range(min(len(c["sizes"]), SCAN_BLOCKS)):
        sl = slice(int(off[g]), int(off[g + 1]))
        if sl.stop == sl.start:
            continue  # an empty block: index 0 whatever its key
        v = step_values(O, tl[sl], ts[sl], pl[sl], ps[sl], c["bits"], n_steps,
                        R.wrap32(SEED + BASE + g), RHO, 2)
        if v[2] < v[1]:
            return g, equal
        equal = equal or v[2] == v[1]
    return None, equal


CASES = [(n, s) for n in S.GRAPH_CASES for s in (3, 4) if S.GRAPH_CASES[n]["path"] != "small_pipe"]


def test_the_record_names_cases_that_exist():
    every = {(n, s) for n in S.GRAPH_CASES for s in (3, 4)}
    assert len(every) == 58 and PASSED_WITHOUT_THE_RESET <= every
    assert len(every - PASSED_WITHOUT_THE_RESET) == 46
    assert {n for n, _ in every - set(CASES)} == {"small_pipe"}


@pytest.mark.parametrize("name,n_steps", CASES)
def test_a_case_fails_without_the_reset_iff_a_block_falls(oracle, name, n_steps):
    g, equal = falling_block(name, n_steps)
    if (name, n_steps) in PASSED_WITHOUT_THE_RESET:
        assert len(S.GRAPH_CASES[name]["sizes"]) <= SCAN_BLOCKS  # every block was looked at
        assert g is None and not equal, \
            f"{name}, {n_steps} steps: block {g} falls, yet the case passed without the reset"
    else:
        assert g is not None, f"{name}, {n_steps} steps failed without the reset, no block falls"
