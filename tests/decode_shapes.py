"""Shapes of the GPU tests of the greedy block decoders, shared with
tests/test_decode_plan.py, which checks on the CPU that each shape takes the
kernel its case names (csrc/cwq_dispatch.h decode_plan) and that together they
meet every lane-mapping condition of the float4 kernels.  Plain data: nothing
here restates the plan."""

GENERAL, Q4, Q4_GLDS = "general", "q4", "q4_glds"  # k_decode, k_decode_q4, k_decode_q4_glds

# test_workspace_state_gpu.py::test_decode_blocks_ignores_buffer_contents:
# (name, d or ragged sizes, nb or None, n_steps)
# d = 12: three Philox blocks per row, 21 rows per wave; d = 36: nine per row,
# 63 of 64 lanes active; d = 256: a wave per row; ragged: the general kernel
DECODE_CASES = [("d12_1step", 12, 37, 1), ("d12_3steps", 12, 37, 3), ("d36", 36, 9, 1),
                ("d256", 256, 3, 1), ("ragged", [3, 20, 0, 45, 1, 64, 130, 0], None, 2)]
# what those comments say, for test_decode_plan.py: name -> (kernel, qpb, bpw)
DECODE_CASES_PLAN = {"d12_1step": (Q4_GLDS, 3, 21), "d12_3steps": (Q4, 3, 21),
                     "d36": (Q4_GLDS, 9, 7), "d256": (Q4_GLDS, 64, 1), "ragged": (GENERAL, 0, 0)}

# ---------------------------------------------------------------------------
# test_decode_kernels_gpu.py
# ---------------------------------------------------------------------------
# uniform float4 shapes: (d, qpb = Philox blocks per row, bpw = blocks per
# chunk); a wave owns a group of B = bpw * qpb blocks as qpb chunks
Q4_DIMS = [(4, 1, 64), (8, 2, 32), (12, 3, 21), (20, 5, 12), (28, 7, 9), (68, 17, 3),
           (100, 25, 2), (132, 33, 1), (252, 63, 1), (256, 64, 1)]


def q4_nbs(qpb, bpw):
    """One block, one whole group, one block more, and six or seven groups
    (two workgroups) whose last holds a full chunk and one block of the next."""
    B = bpw * qpb
    return [1, B, B + 1, 5 * B + bpw + 1]


# the two runs of every shape: single-step codes take the LDS-ring kernel
Q4_RUNS = [dict(n_steps=1, bits=10, rho=1.0, kernel=Q4_GLDS),
           dict(n_steps=3, bits=10, rho=0.7, kernel=Q4)]
# (seed, block_id_base), rotated over the cases; the second and third make
# seed + block_id_base + g leave the int32 range
SEED_BASES = [(42, 0), (2147483647, 123), (-5, 2 ** 32 - 3)]

# Philox block counter n * qpb + q past 2^32: d, at nb = B + 1
COUNTER_DIMS = [20, 32, 256]
COUNTER_BITS = 30
COUNTER_STEPS = [1, 2]
COUNTER_HIGH = 64  # half the indices lie in the last COUNTER_HIGH rows

# uniform calls k_decode takes: d % 4 != 0 or d > 256, (d, nb) ...
GENERAL_UNIFORM = [(1, 300), (5, 103), (13, 41), (260, 5)]
# ... d = 32 with one of the three float arrays one float off a 16-byte boundary
UNALIGNED_D, UNALIGNED_NB = 32, 19
UNALIGNED_WHICH = ["p_loc", "p_scale", "out_sample"]
GENERAL_STEPS = [1, 2]
# ... and k_decode's grid-stride loop into a second pass: the grid is capped at
# 16,384 workgroups of 256 threads; the first multiple of d past 1,000 dims more
GRID_STRIDE_D = 5
GRID_STRIDE_NB = (16384 * 256 + 1000 + GRID_STRIDE_D - 1) // GRID_STRIDE_D

# ragged calls (block_off): empty blocks at both ends and inside, one block of
# 70,000 dims
RAGGED_SIZES = [[0, 0, 3, 1, 0, 64, 257, 0], [70000]]
RAGGED_STEPS = [1, 2]

# out-of-range indices: the planted values, the runs, the shapes
BAD_INDICES = [-1, 1024, -2 ** 31, 2 ** 31 - 1]
BAD_BITS = 10
BAD_STEPS = [1, 3]
BAD_Q4_DIMS = [(12, 3, 21), (100, 25, 2), (256, 64, 1)]  # rows of Q4_DIMS, at nb = 5B + bpw + 1
BAD_GENERAL_UNIFORM = [(5, 331), (260, 7)]
BAD_RAGGED_SIZES = [3, 0, 64, 1, 0, 257, 20, 130]


def bad_blocks_q4(qpb, bpw):
    """The four blocks of a 5B + bpw + 1 block call that get a bad index: a
    middle chunk of group 1, the last lane of group 3's last chunk, the first
    block of group 4 and the call's last block."""
    B = bpw * qpb
    return [B + (qpb // 2) * bpw + bpw // 2, 3 * B + B - 1, 4 * B, 5 * B + bpw]


def bad_blocks(nb):
    """... of a call of nb blocks on the general kernel."""
    return [0, nb // 3, (2 * nb) // 3, nb - 1]


def bad_steps(n_steps):
    """The step of each bad index: first, middle, last, and the first again for
    the last block (whose last step keeps the planted 2^bits - 1)."""
    return [0, n_steps // 2, n_steps - 1, 0]


def q4_cases():
    """Every call of the float4 kernels the GPU tests make:
    dicts (d, nb, n_steps, bits, kernel, what)."""
    out = []
    for d, qpb, bpw in Q4_DIMS:
        for run in Q4_RUNS:
            for nb in q4_nbs(qpb, bpw):
                out.append(dict(d=d, nb=nb, n_steps=run["n_steps"], bits=run["bits"],
                                kernel=run["kernel"], what="shape"))
    for d in COUNTER_DIMS:
        qpb = d // 4
        for n_steps in COUNTER_STEPS:
            out.append(dict(d=d, nb=(64 // qpb) * qpb + 1, n_steps=n_steps, bits=COUNTER_BITS,
                            kernel=Q4_GLDS if n_steps == 1 else Q4, what="counter"))
    for d, qpb, bpw in BAD_Q4_DIMS:
        for n_steps in BAD_STEPS:
            out.append(dict(d=d, nb=q4_nbs(qpb, bpw)[-1], n_steps=n_steps, bits=BAD_BITS,
                            kernel=Q4_GLDS if n_steps == 1 else Q4, what="bad"))
    return out
