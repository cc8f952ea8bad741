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
