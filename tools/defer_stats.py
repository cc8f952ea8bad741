"""What k_encode_prune's screening-only form deferred in one call (run on the
GPU box; CWQ_LIB_PATH selects the build, e.g. one with -DCWQ_DEFER_Q=4).
Usage: python tools/defer_stats.py [nb] [d] [bits]

Runs one cwq_greedy_encode_uniform call on the bench's synthetic blocks (C4 by
default) with the deferral regions in its workspace and reads them back: how
many blocks listed 1, 2, ... rows for k_score_survivors, and how many went to
the deferred list.  With Q slots in use the blocks with more than q < Q rows
are those that list more than q plus the deferred ones, so one run at Q = 4
gives the overflow share of every smaller Q."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import compression_without_quantization_amd as C
from compression_without_quantization_amd import _lib
from compression_without_quantization_amd.synthetic import DEFAULT_SEED, make_blocks_range

SLOTS = 4  # kDeferSlots


def up(v):
    return (v + 255) // 256 * 256


def main():
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    d = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    bits = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    lib = _lib.load()
    host = make_blocks_range(0, nb, d, bits, seed=DEFAULT_SEED)
    t = {k: torch.from_numpy(v.reshape(-1)).cuda() for k, v in host.items()}
    enc = int(lib.cwq_greedy_encode_uniform_workspace_size(nb, d))
    need = int(lib.cwq_greedy_encode_uniform_defer_bytes(nb, d))
    assert need > enc, "this shape has no deferral regions"
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    C.encode_blocks(t["post_loc"], t["post_scale"], t["prior_loc"], t["prior_scale"], bits, 1, 42,
                    block_dim=d, workspace=ws)
    torch.cuda.synchronize()
    o_count = up(enc) + up(nb * SLOTS * 4)
    o_list = o_count + up(nb * 4)
    o_dcount = o_list + up(nb * 4)
    w = ws.cpu().numpy()
    count = w[o_count:o_count + 4 * nb].view(np.uint32)
    deferred = int(w[o_dcount:o_dcount + 4].view(np.uint32)[0])
    hist = np.bincount(count, minlength=SLOTS + 1)[:SLOTS + 1]
    took = deferred != 0xFFFFFFFF and int(hist[1:].sum()) > 0
    out = {"nb": nb, "d": d, "bits": bits, "deferral_ran": bool(took), "deferred": deferred,
           "blocks_listing_rows": {str(c): int(hist[c]) for c in range(1, SLOTS + 1)},
           "share_more_than": {}}
    for q in range(0, SLOTS):
        if hist[q + 1:].sum() or q == 0:  # Q of this build is at least q + 1
            more = int(hist[q + 1:].sum()) + deferred
            out["share_more_than"][str(q)] = more / nb
    print(json.dumps(out))


if __name__ == "__main__":
    main()
