"""Generate tests/golden/workspace_sizes.json: what every *_workspace_size
function of libcwq.so answers over a fixed table of shapes.

The size functions are pure host arithmetic (no device is touched), so this
runs anywhere the library loads.  The committed file was written by the
library as it stood before the workspace layouts moved to
csrc/cwq_workspace.h; tests/test_workspace_layout.py holds every later build
to it row by row.  Regenerate only when a size is meant to change, and say so
in CHANGELOG.md.

Run:  python tests/golden/gen_workspace_sizes.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

I32 = 2 ** 31 - 1
UNIFORM_D = [4, 9, 32, 64, 72, 2000]  # fast pruned kernel / screen arrays / long-block records
# ragged (nb, total_dims, max_block_dim): one block, the 18 blocks of the beam
# tests, blocks at and past CWQ_CSR_LDS_DIMS, many short blocks
RAGGED = [(1, 1, 1), (1, 2000, 2000), (18, 8711, 4095), (7, 3000, 1024), (7, 3000, 1025),
          (300, 9600, 32), (5000, 25000, 9), (3, 0, 0)]
STEPS = [1, 3, 30]
ITEMS = [0, 1, 48]
GROUPED_D = [0, 1, 3, 37, 2049, 5000, 65536]


def table():
    t = []

    def add(fn, *rows):
        t.extend((fn, list(r)) for r in rows)

    add("cwq_greedy_encode_workspace_size", (0, 0, 0), *RAGGED,
        (-1, 0, 0), (0, -1, 0), (0, 0, -1))
    add("cwq_greedy_encode_uniform_workspace_size", (0, 0), (0, 8), (5, 0),
        *[(nb, d) for d in UNIFORM_D for nb in (1, 37, 1000)],
        (-1, 4), (4, -1), (2 ** 62, 4))
    add("cwq_greedy_encode_uniform_var_workspace_size", (0, 0), (0, 8), (5, 0),
        *[(nb, d) for d in UNIFORM_D for nb in (1, 37, 5000)],
        (-1, 4), (4, -1), (I32 + 1, 4))
    add("cwq_greedy_encode_var_workspace_size", (0, 0, 0, 1),
        *[r + (s,) for r in RAGGED for s in STEPS],
        (-1, 0, 0, 1), (1, -1, 0, 1), (1, 1, -1, 1), (1, 1, 1, 0), (I32 + 1, 1, 1, 1))
    add("cwq_pack_indices_var_workspace_size", (0,), (1,), (37,), (4096,), (4097,), (I32,),
        (-1,), (I32 + 1,))
    add("cwq_code_grouped_greedy_workspace_size",
        *[(D, s) for D in GROUPED_D for s in [0] + STEPS], (-1, 1), (4, -1))
    for fn in ("cwq_code_grouped_greedy_batch_workspace_size",
               "cwq_code_grouped_greedy_batch_host_workspace_size"):
        add(fn, *[(D, n, s) for D in (0, 37, 4137, 65536) for n in ITEMS for s in STEPS],
            (-1, 1, 1), (4, -1, 1), (4, 1, -1))
    add("cwq_importance_workspace_size", (0, 0), (1, 1), (1, 0), (42, 357), (5000, 25000),
        (-1, 0), (0, -1))
    add("cwq_code_grouped_importance_workspace_size", *[(D,) for D in GROUPED_D], (-1,))
    add("cwq_code_grouped_importance_batch_workspace_size",
        *[(D, n) for D in (0, 863, 65536) for n in (1, 4, 48)], (4, 0), (-1, 1))
    for fn in ("cwq_decode_grouped_greedy_batch_workspace_size",
               "cwq_decode_grouped_greedy_batch_host_workspace_size"):
        add(fn, *[(D, G, s) for D, G in ((0, 0), (1, 1), (4137, 300), (65536, 48)) for s in STEPS],
            (-1, 0, 1), (0, -1, 1), (4, 1, 0))
    for fn in ("cwq_decode_grouped_importance_batch_workspace_size",
               "cwq_decode_grouped_importance_batch_host_workspace_size"):
        add(fn, (0, 0), (1, 1), (863, 9), (65536, 48), (-1, 0), (0, -1))
    add("cwq_beam_encode_workspace_size",
        *[r + (s, b) for r in RAGGED for s in STEPS for b in (1, 16)], (0, 0, 0, 1, 1),
        (-1, 0, 0, 1, 1), (1, 4, 4, 0, 1), (1, 4, 4, 1, 0), (1, 4, 4, 1, 17))
    add("cwq_greedy_backfit_workspace_size", (0, 0, 0, 1),
        *[r + (s,) for r in RAGGED for s in STEPS],
        *[(nb, nb * d, d, 3) for d in UNIFORM_D for nb in (1, 37)],
        (-1, 0, 0, 1), (1, -1, 0, 1), (1, 1, -1, 1), (1, 1, 1, 0))
    add("cwq_debug_partition_workspace_size", (0,), (1,), (3,), (1024,), (1025,), (2049,),
        (5000,), (262145,), (-1,))
    return t


def main():
    from compression_without_quantization_amd import _lib
    lib = _lib.load()
    rows = [{"function": fn, "arguments": args, "bytes": int(getattr(lib, fn)(*args))}
            for fn, args in table()]
    out = {"abi": "0.12", "rows": rows}
    with open(os.path.join(HERE, "workspace_sizes.json"), "w") as f:
        f.write("{\n \"abi\": \"0.12\",\n \"rows\": [\n")
        f.write(",\n".join("  " + json.dumps(r) for r in out["rows"]))
        f.write("\n ]\n}\n")
    print(len(rows), "rows,", len({r["function"] for r in rows}), "functions")


if __name__ == "__main__":
    main()
