"""Shapes of the GPU tests that name an encoder path, shared with
tests/test_encode_plan.py, which checks on the CPU that each shape takes the
path its test names (csrc/cwq_dispatch.h)."""

# test_gpu.py::test_small_path_adversarial: ragged block lengths by path, and
# its (bits, n_steps) cases
SMALL_PATH_SIZES = {
    "pipeline": [3, 20, 1, 45, 0, 7, 64, 33, 64, 2, 0, 0, 5],
    "three_kernel": [3, 20, 1, 45, 0, 7, 64, 130],
}
SMALL_PATH_BITS_STEPS = [(6, 1), (8, 2), (11, 1)]

# test_gpu.py::test_uniform_odd_d_general_pruned: (d, bits, nb), two steps each
UNIFORM_GENERAL_PRUNED = [(5, 13, 7), (12, 12, 4), (100, 14, 2), (72, 12, 3)]
UNIFORM_GENERAL_PRUNED_STEPS = 2

# test_gpu.py::test_csr_cooperative_rows_vs_oracle: (sizes, bits, n_steps, kind)
CSR_COOP = [
    ([4095, 2000, 300, 257], 14, 2, "normal"),   # few long rows: cooperative 16-lane rows
    ([1500, 255, 256, 40], 13, 3, "normal"),     # coop and per-lane rows in one launch
    ([600] * 3, 14, 1, "flat"),                  # near-ties: survivor overflow, redo, exact
    ([700, 900], 12, 2, "heavy"),
    # row lengths around the loops' unit strides (4 units per lane of a 16-lane
    # slot: 64 units per iteration; 2 units per iteration of a per-lane row)
    # and the LDS / visit-order-record boundary at 1024 dims
    ([256, 257, 259, 255, 1021, 1024, 1025, 1027], 12, 2, "normal"),
    ([1087, 1089, 4093, 513, 511, 7, 3, 1], 12, 2, "heavy"),
]

# test_rows_wave_gpu.py: the forced wave-per-row selftest's block lengths (the
# 248-dim chunk boundary, the 8-wide vector / tail boundary, odd lengths -- a
# Philox block straddles two rows --, an empty block between non-empty ones,
# and the longest group of the PLN codec), its bit counts, and the buckets of
# test_encode_var_long_buckets
ROWS_WAVE_LENGTHS = [1, 3, 0, 4, 5, 7, 8, 9, 247, 4095, 248, 249, 255, 256, 257, 496, 1023, 1025]
ROWS_WAVE_BITS = [0, 1, 5, 9, 11]
LONG_LENS = [4095, 300, 256, 1024, 2049, 700]
LONG_BITS = [9, 9, 1, 5, 9, 11]

# test_workspace_state_gpu.py: the smallest shape at which each encoder path
# exists.  Uniform shapes are (d, bits, nb, n_steps), ragged ones
# (sizes, bits, n_steps).  The tile-queue shape is the fast pruned kernel with
# its tile queue on: 2^12 candidates make one tile of 4,096 per block
# (k_encode_prune draws tiles from the workspace counter from 4,096 candidates
# per tile and more than 1,536 tiles on), and 16,384 blocks make 16,384 tiles.
WS_UNIFORM_PRUNED = (16, 12, 16, 1)        # prune_mode 1 and 2; prune_mode 0: the exact kernel
WS_TILE_QUEUE = (16, 12, 16384, 1)
WS_EVAL_RAGGED = ([3, 20, 0, 45], 4, 2)    # 16 candidates: below the small paths' 64
WS_UNIFORM_GENERAL = [(5, 13, 7, 2), (100, 14, 2, 2)]  # rows of UNIFORM_GENERAL_PRUNED
# per-lane rows (every block below 256 dims), constants in LDS; two steps and
# more than one block: the call forks
WS_CSR_LANE = ([5, 12, 100, 72, 33, 0, 255], 12, 2)
WS_CSR_ALL = CSR_COOP[4][:3]               # cooperative rows, records, the 1,024-dim boundary
WS_SMALL = {"pipeline": (SMALL_PATH_SIZES["pipeline"], 8, 2),
            "three_kernel": (SMALL_PATH_SIZES["three_kernel"], 8, 2)}

# ---------------------------------------------------------------------------
# test_near_ties.py / test_near_ties_gpu.py: one case per scoring path of the
# greedy family, on tests/near_ties.py's inputs.  A block-length list above is
# repeated until the case has at least 16 non-empty blocks.  Each case:
#   group       the GPU test that runs it
#   d           uniform block length, or None: ragged blocks of ``sizes`` dims
#   bits        bits per step: one count, or one per block (a budget call)
#   input_seed  near_ties.inputs' seed;  level: its t_scale level
#   path        the path the case is there for (test_encode_plan.py checks it)
# and what forces the path: ``prune`` (the prune_modes to run), ``guess`` (the
# tau-guess selftest's modes), ``oracle_stride`` (the oracle on every n-th
# block, the whole against prune_mode 0), ``ref_stride`` (the backfitting
# restatement on every n-th block).
# ---------------------------------------------------------------------------
NEAR_TIE_MIN_BLOCKS = 16


def _case(group, sizes, bits, n_steps, input_seed, d=None, level=300.0, **how):
    return dict(group=group, d=d, sizes=list(sizes), bits=bits, n_steps=n_steps,
                input_seed=input_seed, level=level, **how)


def _uni(group, d, bits, nb, n_steps, input_seed, **how):
    return _case(group, [d] * nb, bits, n_steps, input_seed, d=d, **how)


VAR_SHORT_SIZES = SMALL_PATH_SIZES["pipeline"] * 2 + SMALL_PATH_SIZES["three_kernel"]
# the last block (130 dims) at 8 bits: a bucket on the three-kernel path
VAR_SHORT_BITS = ([4, 7, 9, 12, 6, 11, 0, 8, 5, 10, 12] * 4)[:len(VAR_SHORT_SIZES) - 1] + [8]
BACKFIT_LANE = (8, 6, 16384, 3)  # (d, bits, nb, n_steps): a lane per block from 16,384 blocks on

NEAR_TIE_CASES = {
    # the exact kernel
    "exact_uniform": _uni("encode", 16, 12, 64, 1, 1, path="eval", prune=(0,)),
    "exact_ragged": _case("encode", WS_EVAL_RAGGED[0] * 6, WS_EVAL_RAGGED[1], WS_EVAL_RAGGED[2], 5,
                          level=1000.0, path="eval", prune=(None,)),
    # k_encode_prune
    "prune_d8": _uni("encode", 8, 6, 64, 3, 3, path="uniform_pruned", prune=(1, 2)),
    "prune_d16": _uni("encode", 16, 12, 64, 1, 4, path="uniform_pruned", prune=(1, 2)),
    "prune_d32": _uni("encode", 32, 12, 64, 1, 5, path="uniform_pruned", prune=(1, 2)),
    "prune_d64": _uni("encode", 64, 14, 64, 1, 6, path="uniform_pruned", prune=(1, 2)),
    "tau_guess": _uni("tau_guess", 32, 12, 64, 1, 7, path="uniform_pruned", guess=(0, 1, 2)),
    "tile_queue": _uni("encode", *WS_TILE_QUEUE, 8, path="uniform_pruned", prune=(None,),
                       oracle_stride=16),
    # the general pruned kernel on uniform blocks
    "general_d5": _uni("encode", 5, 13, 64, 2, 9, path="csr_pruned", prune=(None,)),
    "general_d100": _uni("encode", 100, 14, 32, 2, 10, path="csr_pruned", prune=(None,)),
    # k_encode_prune_csr: per-lane rows (forked), cooperative rows and records
    "csr_lane": _case("encode", WS_CSR_LANE[0] * 3, WS_CSR_LANE[1], WS_CSR_LANE[2], 11,
                      path="csr_pruned", prune=(0, 2)),
    "csr_coop": _case("encode", CSR_COOP[4][0] * 2, CSR_COOP[4][1], CSR_COOP[4][2], 12,
                      path="csr_pruned", prune=(0, 2)),
    # the small-candidate paths
    "small_pipe_b8": _case("encode", SMALL_PATH_SIZES["pipeline"] * 4, 8, 2, 13,
                           path="small_pipe", prune=(None,)),
    "small_pipe_b11": _case("encode", SMALL_PATH_SIZES["pipeline"] * 4, 11, 1, 14,
                            path="small_pipe", prune=(None,)),
    "small_three_b8": _case("encode", SMALL_PATH_SIZES["three_kernel"] * 4, 8, 2, 15,
                            path="small_three", prune=(None,)),
    "small_three_b11": _case("encode", SMALL_PATH_SIZES["three_kernel"] * 4, 11, 1, 16,
                             path="small_three", prune=(None,)),
    # k_encode_rows_wave, forced
    "rows_wave_b9": _case("rows_wave", ROWS_WAVE_LENGTHS * 2, 9, 2, 17, path="rows_wave"),
    "rows_wave_b11": _case("rows_wave", ROWS_WAVE_LENGTHS * 2, 11, 1, 18, path="rows_wave"),
    # encode_blocks_var: block g at bits[g]
    "var_uniform": _uni("var", 32, [4 + g % 9 for g in range(64)], 64, 2, 19,
                        path="uniform_pruned"),
    "var_long": _case("var", LONG_LENS * 3, LONG_BITS * 3, 2, 20, path="rows_wave"),
    "var_short": _case("var", VAR_SHORT_SIZES, VAR_SHORT_BITS, 2, 21, path="mixed"),
    # the beam encoder: blocks of at most 64 dims, so every selftest path takes them
    "beam": _case("beam", SMALL_PATH_SIZES["pipeline"] * 2, 6, 2, 22, path="beam_lane"),
    "beam_var": _case("beam_var", VAR_SHORT_SIZES[:26], [min(b, 8) for b in VAR_SHORT_BITS[:26]],
                      2, 23, path="beam_lane"),
    # backfitting: a wave per block (short and long ragged blocks), a lane per
    # block, and under budgets
    "backfit_short": _case("backfit", SMALL_PATH_SIZES["three_kernel"] * 3, 6, 3, 21,
                           path="backfit_wave"),
    "backfit_ragged": _case("backfit", ROWS_WAVE_LENGTHS, 5, 3, 25, path="backfit_wave"),
    "backfit_lane": _uni("backfit", *BACKFIT_LANE, 26, path="backfit_lane", ref_stride=64),
    "backfit_var": _case("backfit_var", VAR_SHORT_SIZES, [min(b, 8) for b in VAR_SHORT_BITS], 2,
                         27, path="backfit_wave"),
}

# ---------------------------------------------------------------------------
# test_graph_replay_gpu.py: one case per encoder path, each captured into a
# graph at every step count of GRAPH_STEPS (tests/graph_replay.py).  Each case:
#   entry   the C entry point: "uniform" (cwq_greedy_encode_uniform), "defer"
#           (cwq_selftest_encode_uniform_defer, ``defer``: its mode), "csr"
#           (cwq_greedy_encode), "rows_wave" (cwq_selftest_encode_rows_wave)
#   d, nb   uniform blocks, or ``sizes``: ragged ones
#   prune   cwq_options.prune_mode
#   path    the path of every block range (test_encode_plan.py checks it), and
#           ``tiles``: "one" tile per block, "many" (the interleaved launch, its
#           tail tiles split), or "queue" (one tile per block, the tile queue)
#   oracle_stride  the oracle on every n-th block, the whole table against a
#           prune_mode 0 run that the oracle has confirmed on those blocks
# The seed and the base make seed + base + g wrap past 2^31 - 1 in every case.
# ---------------------------------------------------------------------------
GRAPH_STEPS = (1, 2, 3, 4)
GRAPH_RHO, GRAPH_SEED, GRAPH_BASE = 0.8, 2 ** 31 - 4, 5
GRAPH_FAILURE_SHAPE = (32, 12, 70)  # (d, bits, nb) of the failure DESIGN.md 4 recorded


def _guni(d, bits, nb, prune, path, tiles=None, entry="uniform", **how):
    return dict(entry=entry, d=d, sizes=[d] * nb, bits=bits, prune=prune, path=path, tiles=tiles,
                **how)


def _gcsr(sizes, bits, path, entry="csr", prune=2, **how):
    return dict(entry=entry, d=None, sizes=list(sizes), bits=bits, prune=prune, path=path,
                tiles=None, **how)


GRAPH_CASES = {
    "exact_uniform": _guni(*WS_UNIFORM_PRUNED[:3], 0, "eval"),
    # (the tiling aims at 16,384 tiles a launch: below 16,384 blocks a block of
    # 4,096 candidates is split into tiles of 256, and the uniform entry runs one
    # tile per block only where the tile queue is on; the deferral selftest's
    # mode 0 is the single launch with one tile per block and no queue)
    "prune_d16_mode1": _guni(*WS_UNIFORM_PRUNED[:3], 1, "uniform_pruned", "many"),
    "prune_d16_mode2": _guni(*WS_UNIFORM_PRUNED[:3], 2, "uniform_pruned", "many"),
    **{f"prune_d{d}_nb70_mode{m}": _guni(d, 12, 70, m, "uniform_pruned", "many")
       for d in (8, 32, 64) for m in (1, 2)},
    "prune_inter": _guni(32, 16, 4, 2, "uniform_pruned", "many"),
    "prune_one_tile": _guni(*GRAPH_FAILURE_SHAPE, 2, "uniform_pruned", "one", entry="defer",
                            defer=0),
    "prune_one_tile_mode1": _guni(*GRAPH_FAILURE_SHAPE, 1, "uniform_pruned", "one",
                                  entry="defer", defer=0),
    "tile_queue": _guni(*WS_TILE_QUEUE[:3], 2, "uniform_pruned", "queue", oracle_stride=16),
    **{f"defer_mode{m}": _guni(*GRAPH_FAILURE_SHAPE, 2, "uniform_pruned", "one", entry="defer",
                               defer=m) for m in (1, 2, 3)},
    "general_d5": _guni(*WS_UNIFORM_GENERAL[0][:3], 2, "csr_pruned"),
    "general_d100": _guni(*WS_UNIFORM_GENERAL[1][:3], 2, "csr_pruned"),
    "exact_ragged": _gcsr(*WS_EVAL_RAGGED[:2], "eval"),
    "csr_lane": _gcsr(*WS_CSR_LANE[:2], "csr_pruned"),
    "csr_all": _gcsr(*WS_CSR_ALL[:2], "csr_pruned"),
    "small_pipe": _gcsr(*WS_SMALL["pipeline"][:2], "small_pipe"),
    "small_three": _gcsr(*WS_SMALL["three_kernel"][:2], "small_three"),
    "rows_wave": _gcsr(ROWS_WAVE_LENGTHS[:8], 9, "rows_wave", entry="rows_wave"),
    # The few-block cases above once more with their layout repeated to
    # GRAPH_MIN_BLOCKS blocks or more.  A key left over from the step before
    # shows only in a block whose best value falls from that step to the next;
    # with 2 to 8 blocks a case may hold none ("Teeth").
    "prune_inter_x4": _guni(32, 16, 16, 2, "uniform_pruned", "many"),
    "general_d5_x3": _guni(WS_UNIFORM_GENERAL[0][0], WS_UNIFORM_GENERAL[0][1],
                           3 * WS_UNIFORM_GENERAL[0][2], 2, "csr_pruned"),
    "general_d100_x8": _guni(WS_UNIFORM_GENERAL[1][0], WS_UNIFORM_GENERAL[1][1],
                             8 * WS_UNIFORM_GENERAL[1][2], 2, "csr_pruned"),
    "exact_ragged_x6": _gcsr(WS_EVAL_RAGGED[0] * 6, WS_EVAL_RAGGED[1], "eval"),
    "small_three_x3": _gcsr(WS_SMALL["three_kernel"][0] * 3, WS_SMALL["three_kernel"][1],
                            "small_three"),
}
GRAPH_MIN_BLOCKS = 16
# the uniform decoders' cases of test_graph_replay_gpu.py: (encoder case, kernel family)
GRAPH_DECODE_STEPS = (1, 3)  # the LDS-ring float4 kernel takes one step, the other more
GRAPH_DECODE_CASES = {
    "uniform_float4": ("prune_d32_nb70_mode2", "uniform", "q4"),   # d % 4 == 0: the float4 kernels
    "uniform_general": ("general_d5", "uniform", "general"),       # a d they do not take
    "ragged": ("csr_lane", "csr", "general"),
}
