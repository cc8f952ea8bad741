"""Per-block bit budgets: what the bucketed call costs.

    python tools/bench_varbits.py [--nb 1000000] [--d 32] [--rounds 3] [--timeout 300]

For nb uniform blocks of dimension d, n_steps = 1, inputs resident in HBM:

  (a) encode_blocks_var with every block at 16 bits against encode_blocks at
      16 bits (config C4's blocks), interleaved in one process;
  (b) a spread of budgets, bits = clip(round(N(12, 2)), 4, 16), each block
      made with the KL its budget stands for: encode_blocks_var against the
      sum of plain encode_blocks calls over the same blocks sorted by budget
      on the host beforehand -- the floor of any bucketed design;
  (c) on (b)'s result: block_bits, pack_indices, unpack_indices and
      decode_blocks_var, and the stream's bytes per second.

The parent process never touches the GPU: each part runs in a child of its own
under --timeout seconds, and a part that fails or runs out of time ends the
run.  Times are host wall clock around synchronised calls (the variable call
synchronises once itself), milliseconds; every line is one JSON object.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _dev(torch, blocks):
    return [torch.from_numpy(blocks[k].reshape(-1)).cuda()
            for k in ("post_loc", "post_scale", "prior_loc", "prior_scale")]


def part_a(args):
    import numpy as np
    import torch
    import compression_without_quantization_amd as C
    from compression_without_quantization_amd.synthetic import make_blocks
    from compression_without_quantization_amd.varbits import encode_var_workspace_bytes
    nb, d = args.nb, args.d
    tl, ts, pl, ps = _dev(torch, make_blocks(nb, d, 16))
    bits = torch.full((nb,), 16, dtype=torch.int32, device="cuda")
    oi = torch.empty((nb, 1), dtype=torch.int32, device="cuda")
    os_ = torch.empty(nb * d, dtype=torch.float32, device="cuda")
    vi, vs = torch.empty_like(oi), torch.empty_like(os_)
    ws = torch.empty(C.encode_workspace_bytes(nb, nb * d, block_dim=d), dtype=torch.uint8,
                     device="cuda")
    vws = torch.empty(encode_var_workspace_bytes(nb, d), dtype=torch.uint8, device="cuda")

    def plain():
        C.encode_blocks(tl, ts, pl, ps, 16, 1, 42, block_dim=d, out_idx=oi, out_sample=os_,
                        workspace=ws)

    def var():
        C.encode_blocks_var(tl, ts, pl, ps, bits, 1, 42, block_dim=d, out_idx=vi, out_sample=vs,
                            workspace=vws)

    plain(), var()  # warm-up
    same = bool(torch.equal(oi, vi)) and bool(torch.equal(os_.view(torch.int32),
                                                          vs.view(torch.int32)))
    tp, tv = [], []
    for _ in range(args.rounds):
        tp.append(_timed(torch, plain))
        tv.append(_timed(torch, var))
    mp, mv = float(np.median(tp)), float(np.median(tv))
    print(json.dumps({"part": "a", "nb": nb, "d": d, "bits": 16, "plain_ms": tp, "var_ms": tv,
                      "plain_median_ms": mp, "var_median_ms": mv,
                      "var_over_plain": mv / mp, "identical": same}))


def _spread(args):
    """Blocks whose KL matches a spread of budgets, in random block order."""
    import numpy as np
    from compression_without_quantization_amd.synthetic import make_blocks
    nb, d = args.nb, args.d
    rng = np.random.Generator(np.random.PCG64(12))
    bits = np.clip(np.round(rng.normal(12.0, 2.0, nb)), 4, 16).astype(np.int32)
    blocks = {k: np.empty((nb, d), np.float32)
              for k in ("post_loc", "post_scale", "prior_loc", "prior_scale")}
    for b in np.unique(bits):
        rows = np.nonzero(bits == b)[0]
        part = make_blocks(rows.size, d, int(b), seed=1000 + int(b))
        for k in blocks:
            blocks[k][rows] = part[k]
    return bits, blocks


def part_bc(args):
    import numpy as np
    import torch
    import compression_without_quantization_amd as C
    from compression_without_quantization_amd.varbits import encode_var_workspace_bytes
    nb, d = args.nb, args.d
    bits_h, blocks = _spread(args)
    tl, ts, pl, ps = _dev(torch, blocks)
    bits = torch.from_numpy(bits_h).cuda()
    # the floor: the same blocks sorted by budget on the host, one plain call each
    order = np.argsort(bits_h, kind="stable")
    sl, ss, spl, sps = _dev(torch, {k: v[order] for k, v in blocks.items()})
    counts = np.bincount(bits_h, minlength=31)
    starts = np.concatenate([[0], np.cumsum(counts)])
    ws = torch.empty(C.encode_workspace_bytes(nb, nb * d, block_dim=d), dtype=torch.uint8,
                     device="cuda")
    vws = torch.empty(encode_var_workspace_bytes(nb, d), dtype=torch.uint8, device="cuda")
    fi = torch.empty((nb, 1), dtype=torch.int32, device="cuda")
    fs = torch.empty(nb * d, dtype=torch.float32, device="cuda")
    vi, vs = torch.empty_like(fi), torch.empty_like(fs)

    def floor():
        for b in range(30, -1, -1):
            r0, r1 = int(starts[b]), int(starts[b + 1])
            if r1 == r0:
                continue
            C.encode_blocks(sl[r0 * d:r1 * d], ss[r0 * d:r1 * d], spl[r0 * d:r1 * d],
                            sps[r0 * d:r1 * d], b, 1, 42, block_dim=d, out_idx=fi[r0:r1],
                            out_sample=fs[r0 * d:r1 * d], workspace=ws)

    def var():
        C.encode_blocks_var(tl, ts, pl, ps, bits, 1, 42, block_dim=d, out_idx=vi, out_sample=vs,
                            workspace=vws)

    floor(), var()  # warm-up
    tf, tv = [], []
    for _ in range(args.rounds):
        tf.append(_timed(torch, floor))
        tv.append(_timed(torch, var))
    # each bucket alone, for the table of where the time goes
    per_bucket = {}
    for b in range(30, -1, -1):
        r0, r1 = int(starts[b]), int(starts[b + 1])
        if r1 > r0:
            per_bucket[b] = [int(r1 - r0), _timed(torch, lambda: C.encode_blocks(
                sl[r0 * d:r1 * d], ss[r0 * d:r1 * d], spl[r0 * d:r1 * d], sps[r0 * d:r1 * d], b,
                1, 42, block_dim=d, out_idx=fi[r0:r1], out_sample=fs[r0 * d:r1 * d],
                workspace=ws))]
    mf, mv = float(np.median(tf)), float(np.median(tv))
    print(json.dumps({"part": "b", "nb": nb, "d": d, "mean_bits": float(bits_h.mean()),
                      "floor_ms": tf, "var_ms": tv, "floor_median_ms": mf, "var_median_ms": mv,
                      "var_over_floor": mv / mf,
                      "bucket_blocks_ms": per_bucket,
                      "blocks_per_s": nb / (mv * 1e-3)}))

    # (c) the budgets, the stream and the way back
    post = [tl, ts, pl, ps]
    C.block_bits(*post, d)
    t_bits = [_timed(torch, lambda: C.block_bits(*post, d)) for _ in range(args.rounds)]
    code, total = C.pack_indices(vi, bits)
    t_pack = [_timed(torch, lambda: C.pack_indices(vi, bits)) for _ in range(args.rounds)]
    back = C.unpack_indices(code, bits, 1)
    t_unpack = [_timed(torch, lambda: C.unpack_indices(code, bits, 1))
                for _ in range(args.rounds)]
    dec = C.decode_blocks_var(code, bits, pl, ps, 1, 42, block_dim=d)
    t_dec = [_timed(torch, lambda: C.decode_blocks_var(code, bits, pl, ps, 1, 42, block_dim=d))
             for _ in range(args.rounds)]
    ok = bool(torch.equal(back, vi)) and bool(torch.equal(dec.view(torch.int32),
                                                          vs.view(torch.int32)))
    n_bytes = int(code.numel())
    print(json.dumps({"part": "c", "nb": nb, "total_bits": total, "stream_bytes": n_bytes,
                      "block_bits_ms": t_bits, "pack_ms": t_pack, "unpack_ms": t_unpack,
                      "decode_var_ms": t_dec,
                      "pack_bytes_per_s": n_bytes / (float(np.median(t_pack)) * 1e-3),
                      "unpack_bytes_per_s": n_bytes / (float(np.median(t_unpack)) * 1e-3),
                      "round_trip_identical": ok}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nb", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per part")
    ap.add_argument("--part", choices=["a", "bc"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part:
        return {"a": part_a, "bc": part_bc}[args.part](args)
    for part in ("a", "bc"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--nb", str(args.nb),
               "--d", str(args.d), "--rounds", str(args.rounds)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"part": part, "error": f"no result in {args.timeout} s"}))
            return 124
        if rc != 0:  # nothing more is started on the GPU after a failed part
            print(json.dumps({"part": part, "error": f"exit status {rc}"}))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
