#!/usr/bin/env python
"""Per-group bit budgets in the PLN codec and the wave-per-row encoder behind
them, measured on one MI355X.  Synchronised wall clock, three
interleaved rounds in one process, one JSON object on stdout.

  (c2low)  the grouped coder on the c2low latents (50 groups, 46 of 4,095 dims,
           30 steps x 14 bits): code_grouped_greedy_sample_var in the default
           mode (long buckets on k_encode_rows_wave) against prune_mode=0
           (k_encode_eval) and against the reference-shaped call.
  (bucket) the largest budget bucket of that call alone, through
           encode_blocks_var with a preallocated workspace, both modes.
  (pln)    code_image_greedy on one 512x768 image at the CLI defaults (random
           weights): plain against first_level_group_bits=True: time, level-1
           code bits, side information, file bytes, the budget histogram.

Run it with CWQ_LIB_PATH pointing at a build made with -DCWQ_VAR_ROWS_WAVE=0
for the dispatch the library had before the wave-per-row kernel.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import compression_without_quantization_amd as C  # noqa: E402
import compression_without_quantization_amd.coded_greedy_sampler as S  # noqa: E402
import compression_without_quantization_amd.coded_importance_sampler as I  # noqa: E402
from compression_without_quantization_amd import _lib  # noqa: E402
from compression_without_quantization_amd import pln as P  # noqa: E402
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


def spread(ms):
    return float(max(ms) - min(ms))


def c2low_latents():
    dev = torch.device("cuda", 0)
    return tuple(torch.from_numpy(a).to(dev)
                 for a in make_latents(D_C2, bits_per_dim=0.06, seed=0))


def c2low(reps, n_bits=14, n_steps=30):
    q_loc, q_scale, p_loc, p_scale = c2low_latents()
    t, p = C.Normal(q_loc, q_scale), C.Normal(p_loc, p_scale)
    res = {}
    fns = {
        "reference_shaped": lambda: res.__setitem__(
            "ref", C.code_grouped_greedy_sample(None, t, p, n_steps, n_bits, 42)),
        "budgets": lambda: res.__setitem__(
            "var", C.code_grouped_greedy_sample_var(t, p, n_steps, n_bits, 42)),
        "budgets_prune0": lambda: res.__setitem__(
            "var0", C.code_grouped_greedy_sample_var(t, p, n_steps, n_bits, 42, prune_mode=0)),
    }
    ms = interleaved(fns, reps)
    sample, code, total, starts, gb = res["var"]
    dec = C.decode_grouped_greedy_sample_var(code, starts, gb, p, n_steps, 42)
    lens = np.diff(np.asarray(starts))
    return {"n_bits_per_step": n_bits, "n_steps": n_steps, "reps": reps, "groups": len(gb),
            "groups_of_4095": int((lens == 4095).sum()), "ms": ms,
            "spread_ms": {k: spread(v) for k, v in ms.items()},
            "prune0_same_code": res["var0"][1] == code and
            np.array_equal(res["var0"][0].view(np.uint32), sample.view(np.uint32)),
            "reference_bits": len(res["ref"][1]), "budget_bits": int(total),
            "group_bits_hist": np.bincount(gb, minlength=n_bits + 1).tolist(),
            "round_trip": bool(np.array_equal(dec.view(np.uint32), sample.view(np.uint32)))}


def bucket(reps, n_bits=14, n_steps=30):
    """The call's largest bucket alone: its groups, gathered, at their budget."""
    lib = _lib.load()
    q_loc, q_scale, p_loc, p_scale = c2low_latents()
    dev = q_loc.device
    t_loc, t_scale, kl = (torch.empty(D_C2, dtype=torch.float32, device=dev) for _ in range(3))
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.cwq_standardise(_ptr(q_loc), _ptr(q_scale), _ptr(p_loc), _ptr(p_scale), D_C2,
                                   _ptr(t_loc), _ptr(t_scale), st), "cwq_standardise")
    _lib.check(lib.cwq_kl_normal_normal(_ptr(q_loc), _ptr(q_scale), _ptr(p_loc), _ptr(p_scale),
                                        D_C2, _ptr(kl), st), "cwq_kl_normal_normal")
    starts = np.asarray(C.group_starts(kl.cpu().numpy(), n_bits * n_steps), dtype=np.int64)
    gb = C.block_bits(q_loc, q_scale, p_loc, p_scale, block_off=starts, n_steps=n_steps,
                      max_bits=n_bits).cpu().numpy()
    b = int(np.bincount(gb).argmax())
    rows = np.flatnonzero(gb == b)
    dims = np.concatenate([np.arange(starts[g], starts[g + 1]) for g in rows])
    sel = torch.from_numpy(dims).to(dev)
    tl, ts = t_loc[sel].contiguous(), t_scale[sel].contiguous()
    zeros, ones = torch.zeros_like(tl), torch.ones_like(tl)
    lens = np.diff(starts)[rows]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nb, D, mbd = len(rows), int(off[-1]), int(lens.max())
    bits = torch.full((nb,), b, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.cwq_greedy_encode_var_workspace_size(nb, D, mbd, n_steps),
                     dtype=torch.uint8, device=dev)
    oi = [torch.empty((nb, n_steps), dtype=torch.int32, device=dev) for _ in range(2)]
    os_ = [torch.empty(D, dtype=torch.float32, device=dev) for _ in range(2)]
    call = lambda k, mode: C.encode_blocks_var(  # noqa: E731
        tl, ts, zeros, ones, bits, n_steps, 42, block_off=off, max_block_dim=mbd, out_idx=oi[k],
        out_sample=os_[k], workspace=ws, prune_mode=mode)
    ms = interleaved({"default": lambda: call(0, None), "prune0": lambda: call(1, 0)}, reps)
    same = bool(torch.equal(oi[0], oi[1]) and torch.equal(os_[0].view(torch.int32),
                                                          os_[1].view(torch.int32)))
    return {"n_bits": b, "n_steps": n_steps, "groups": nb, "dims": D, "max_block_dim": mbd,
            "rows_per_step": nb << b, "reps": reps, "ms": ms,
            "spread_ms": {k: spread(v) for k, v in ms.items()}, "outputs_equal": same}


def pln(reps, H=512, W=768):
    dev = torch.device("cuda", 0)
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    model = P.ProbabilisticLadderNetwork().to(dev).eval()
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W] / max(H, W)
    base = np.stack([np.sin(6 * xx + c) * np.cos(4 * yy - c) for c in range(3)], -1)
    img = np.clip(0.5 + 0.35 * base + 0.05 * rng.standard_normal((H, W, 3)), 0, 1) \
        .astype(np.float32)[None]
    kw = dict(n_steps=30, n_bits_per_step=14, greedy_max_group_size_bits=12,
              second_level_n_bits_per_group=20, second_level_max_group_size_bits=2,
              second_level_dim_kl_bit_limit=16)
    tmp = tempfile.mkdtemp()
    paths = {k: os.path.join(tmp, k + ".miracle") for k in ("plain", "budgets")}
    summ = {}
    fns = {
        "plain": lambda: summ.__setitem__("plain", model.code_image_greedy(
            None, img, 42, comp_file_path=paths["plain"], **kw)[1]),
        "budgets": lambda: summ.__setitem__("budgets", model.code_image_greedy(
            None, img, 42, comp_file_path=paths["budgets"], first_level_group_bits=True,
            **kw)[1]),
    }
    ms = interleaved(fns, reps)
    rec = {k: model.decode_image_greedy(None, paths[k], use_importance_sampling=False,
                                        second_level_max_group_size_bits=2,
                                        first_level_group_bits=(k == "budgets"))
           for k in paths}
    sb, sp = summ["budgets"], summ["plain"]
    groups1 = sp["first_level_groups"] - 1
    return {"image": [H, W], "reps": reps, "ms": ms,
            "spread_ms": {k: spread(v) for k, v in ms.items()},
            "level1_groups": groups1,
            "level1_bits": {"plain": groups1 * kw["n_steps"] * kw["n_bits_per_step"],
                            "budgets": sb["first_level_code_bits"]},
            # extra_byte_size counts the variable bit strings' bits (the reference's name)
            "budget_side_info_bits": sb["extra_byte_size"] - sp["extra_byte_size"],
            "file_bytes": {"plain": sp["actual_byte_size"], "budgets": sb["actual_byte_size"]},
            "group_bits_hist": sb["first_level_bits_histogram"],
            "decoded_finite": {k: bool(np.isfinite(v).all()) for k, v in rec.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=3, help="calls per round")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--only", default="c2low,bucket,pln", help="sections: c2low, bucket, pln")
    ap.add_argument("--once", action="store_true", help="one c2low call with budgets in the "
                    "default mode and nothing else (for a kernel trace)")
    args = ap.parse_args()
    S.VERBOSE = I.VERBOSE = False
    torch.cuda.set_device(0)
    if args.once:
        q_loc, q_scale, p_loc, p_scale = c2low_latents()
        r = C.code_grouped_greedy_sample_var(C.Normal(q_loc, q_scale), C.Normal(p_loc, p_scale),
                                             30, 14, 42)
        torch.cuda.synchronize()
        print(json.dumps({"once": "c2low", "budget_bits": int(r[2]),
                          "group_bits_hist": np.bincount(r[4], minlength=15).tolist()}))
        return
    only = args.only.split(",")
    result = {"lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" +
              os.path.basename(_lib.LIB_PATH)}
    if "c2low" in only:
        result["c2low"] = c2low(args.reps)
    if "bucket" in only:
        result["bucket"] = bucket(args.reps)
    if "pln" in only:
        result["pln"] = pln(args.reps)
    text = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
