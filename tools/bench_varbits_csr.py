#!/usr/bin/env python
"""Per-block bit budgets on ragged (CSR) blocks, measured on one MI355X
(DESIGN.md 4d).  Synchronised wall clock, three interleaved rounds in one
process, one JSON object on stdout.

  (a) the layer's cost: encode_blocks_var with every block at one count against
      the plain encode_blocks(block_off=...) call on the same blocks (the plain
      call is the yardstick): the c2cli item's groups at 14 bits x 30 steps,
      and C2's ~41k short groups at 8 bits.
  (b) the gain on the grouped coder: code_grouped_greedy_sample_var against
      code_grouped_greedy_sample on the c2low and the C2 latents (bench.py's
      make_latents parameters): time per call (also with prune_mode=0), code
      bits, histogram of budgets.
  (long) what a bucket of c2low's long groups costs by itself: the plain call
      at 14, 12 and 9 bits, and at 9 bits with prune_mode=0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import compression_without_quantization_amd as C  # noqa: E402
import compression_without_quantization_amd.coded_greedy_sampler as S  # noqa: E402
from compression_without_quantization_amd import _lib  # noqa: E402
from compression_without_quantization_amd.synthetic import make_latents  # noqa: E402
from compression_without_quantization_amd.varbits import _ptr  # noqa: E402

D_C2 = 32 * 48 * 128
ROUNDS = 3


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def interleaved(fns, reps):
    """ms per call of every function, ROUNDS rounds, the functions taking turns."""
    for fn in fns.values():  # warm-up: workspaces, library streams, code objects
        fn()
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            out[k].append(timed(fn, reps))
    return out


def standardised(bpd):
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    q_loc, q_scale, p_loc, p_scale = (torch.from_numpy(a).to(dev)
                                      for a in make_latents(D_C2, bits_per_dim=bpd, seed=0))
    t_loc, t_scale, kl = (torch.empty(D_C2, dtype=torch.float32, device=dev) for _ in range(3))
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.cwq_standardise(_ptr(q_loc), _ptr(q_scale), _ptr(p_loc), _ptr(p_scale), D_C2,
                                   _ptr(t_loc), _ptr(t_scale), st), "cwq_standardise")
    _lib.check(lib.cwq_kl_normal_normal(_ptr(q_loc), _ptr(q_scale), _ptr(p_loc), _ptr(p_scale),
                                        D_C2, _ptr(kl), st), "cwq_kl_normal_normal")
    return (q_loc, q_scale, p_loc, p_scale), t_loc, t_scale, kl.cpu().numpy()


def layer_cost(name, bpd, n_bits, n_steps, reps):
    _, t_loc, t_scale, kl = standardised(bpd)
    starts = np.asarray(C.group_starts(kl, n_bits * n_steps), dtype=np.int64)
    nb, mbd = starts.size - 1, int(np.diff(starts).max())
    dev = t_loc.device
    zeros, ones = torch.zeros_like(t_loc), torch.ones_like(t_loc)
    bits = torch.full((nb,), n_bits, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws_p = torch.empty(S.encode_workspace_bytes(nb, D_C2, max_block_dim=mbd), dtype=torch.uint8,
                       device=dev)
    ws_v = torch.empty(lib.cwq_greedy_encode_var_workspace_size(nb, D_C2, mbd, n_steps),
                       dtype=torch.uint8, device=dev)
    oi = [torch.empty((nb, n_steps), dtype=torch.int32, device=dev) for _ in range(2)]
    os_ = [torch.empty(D_C2, dtype=torch.float32, device=dev) for _ in range(2)]
    fns = {
        "plain": lambda: C.encode_blocks(t_loc, t_scale, zeros, ones, n_bits, n_steps, 42,
                                         block_off=starts, max_block_dim=mbd, out_idx=oi[0],
                                         out_sample=os_[0], workspace=ws_p),
        "var": lambda: C.encode_blocks_var(t_loc, t_scale, zeros, ones, bits, n_steps, 42,
                                           block_off=starts, max_block_dim=mbd, out_idx=oi[1],
                                           out_sample=os_[1], workspace=ws_v),
    }
    ms = interleaved(fns, reps)
    same = bool(torch.equal(oi[0], oi[1]) and torch.equal(os_[0].view(torch.int32),
                                                          os_[1].view(torch.int32)))
    p, v = np.array(ms["plain"]), np.array(ms["var"])
    return {"shape": name, "groups": nb, "max_block_dim": mbd, "n_bits": n_bits,
            "n_steps": n_steps, "reps": reps, "plain_ms": ms["plain"], "var_ms": ms["var"],
            "ratio_by_round": (v / p).tolist(), "ratio_of_medians": float(np.median(v) /
                                                                          np.median(p)),
            "plain_spread": float(p.max() / p.min()), "extra_ms": float(np.median(v) -
                                                                        np.median(p)),
            "outputs_equal": same}


def grouped_gain(name, bpd, n_bits, n_steps, reps):
    (q_loc, q_scale, p_loc, p_scale), _, _, _ = standardised(bpd)
    t, p = C.Normal(q_loc, q_scale), C.Normal(p_loc, p_scale)
    res = {}
    fns = {
        "reference_shaped": lambda: res.__setitem__(
            "ref", C.code_grouped_greedy_sample(None, t, p, n_steps, n_bits, 42)),
        "per_group_budgets": lambda: res.__setitem__(
            "var", C.code_grouped_greedy_sample_var(t, p, n_steps, n_bits, 42)),
        # every candidate scored exactly: the same results by another encoder path
        "per_group_budgets_prune0": lambda: res.__setitem__(
            "var0", C.code_grouped_greedy_sample_var(t, p, n_steps, n_bits, 42, prune_mode=0)),
    }
    ms = interleaved(fns, reps)
    _, ref_code, ref_starts = res["ref"]
    sample, code, total, starts, gb = res["var"]
    dec = C.decode_grouped_greedy_sample_var(code, starts, gb, p, n_steps, 42)
    return {"latents": name, "n_bits_per_step": n_bits, "n_steps": n_steps, "reps": reps,
            "groups": len(gb), "same_partition": starts == ref_starts,
            "reference_ms": ms["reference_shaped"], "var_ms": ms["per_group_budgets"],
            "var_prune0_ms": ms["per_group_budgets_prune0"],
            "prune0_same_code": res["var0"][1] == code,
            "reference_bits": len(ref_code), "var_bits": int(total),
            "side_info_bits_raw": 5 * len(gb),
            "group_bits_hist": np.bincount(gb, minlength=n_bits + 1).tolist(),
            "round_trip": bool(np.array_equal(dec.view(np.uint32), sample.view(np.uint32)))}


def plain_at(bpd, part_bits, n_steps, n_bits, prune_mode):
    """One plain encode_blocks call on the groups of a latent set at n_bits per
    step (what a bucket of that budget costs by itself), ms."""
    _, t_loc, t_scale, kl = standardised(bpd)
    starts = np.asarray(C.group_starts(kl, part_bits * n_steps), dtype=np.int64)
    zeros, ones = torch.zeros_like(t_loc), torch.ones_like(t_loc)
    fn = lambda: C.encode_blocks(t_loc, t_scale, zeros, ones, n_bits, n_steps, 42,  # noqa: E731
                                 block_off=starts, prune_mode=prune_mode)
    fn()
    return {"groups": int(starts.size - 1), "max_block_dim": int(np.diff(starts).max()),
            "n_bits": n_bits, "n_steps": n_steps, "prune_mode": prune_mode, "ms": timed(fn, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5, help="calls per round")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--only", default="layer,gain,long", help="sections: layer, layer-short "
                    "(the short groups alone), gain, long (plain calls on c2low's long groups "
                    "below 4096 candidates)")
    args = ap.parse_args()
    S.VERBOSE = False
    torch.cuda.set_device(0)
    only = args.only.split(",")
    result = {}
    if "layer" in only:
        result["layer_cost"] = [layer_cost("c2cli groups", 1.1, 14, 30, args.reps),
                                layer_cost("C2 short groups", 1.1, 8, 1, args.reps)]
    if "layer-short" in only:
        result["layer_cost"] = [layer_cost("C2 short groups", 1.1, 8, 1, args.reps)]
    if "gain" in only:
        result["grouped_gain"] = [grouped_gain("c2low", 0.06, 14, 30, args.reps),
                                  grouped_gain("C2", 1.1, 8, 1, args.reps)]
    if "long" in only:
        result["c2low_plain"] = [plain_at(0.06, 14, 30, 14, None), plain_at(0.06, 14, 30, 9, None),
                                 plain_at(0.06, 14, 30, 9, 0), plain_at(0.06, 14, 30, 12, None)]
    text = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
