#!/usr/bin/env python
"""The rate table measured on one MI355X: ms per ``cwq_rate_table``
call against what a caller had to do before it existed, B + 1 plain encodes at
b = 0 .. B through the parent commit's library (``--parent-lib``, loaded directly:
the bindings refuse another ABI version, and the encoders' argument lists are
the same in both), on the same buffers in the same process.

  (u32)    65,536 uniform blocks of d = 32 at B = 8, 11 and 16
  (c2low)  the c2low item's standardised groups at B = 9

Per figure: HIP events around the whole call (for the loop: around all B + 1
calls) on the current stream, outputs and workspaces allocated beforehand,
warm-up rounds first, then interleaved rounds whose order alternates; every
call's time is kept, the median is quoted.  Also:

  * the plain encode at B bits alone on both libraries in alternating rounds
    (nothing it runs has changed: ``inside_parent_spread`` says whether this
    build's median lies inside the parent's own run-to-run range);
  * ``cwq_choose_bits`` and ``choose_bits_total`` on a table of 10^6 blocks;
  * the mean value per block that ``choose_bits_total`` gains over ``block_bits``
    at the same total, on 65,536 synthetic d = 32 blocks whose KLs follow
    bits = clip(round(N(12, 2)), 4, 16) (README's ``encode_blocks_var`` row).

One JSON object on stdout.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import compression_without_quantization_amd as C  # noqa: E402
import compression_without_quantization_amd.coded_greedy_sampler as S  # noqa: E402
from compression_without_quantization_amd import _lib  # noqa: E402
from compression_without_quantization_amd.synthetic import make_blocks  # noqa: E402
from compression_without_quantization_amd.varbits import _ptr  # noqa: E402
from bench_beam_var import bind, rounds_ms, stat  # noqa: E402

SEED = 42
ENCODERS = ["cwq_greedy_encode", "cwq_greedy_encode_uniform", "cwq_greedy_encode_workspace_size",
            "cwq_greedy_encode_uniform_workspace_size", "cwq_greedy_encode_uniform_defer_bytes"]


def standardised(blk):
    dev = torch.device("cuda", 0)
    pl, ps = blk["prior_loc"].reshape(-1), blk["prior_scale"].reshape(-1)
    tl = ((blk["post_loc"].reshape(-1) - pl) / ps).astype(np.float32)
    ts = (blk["post_scale"].reshape(-1) / ps).astype(np.float32)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return f(tl), f(ts), torch.zeros(tl.size, device=dev), torch.ones(tl.size, device=dev)


def u32_shape(nb=65536, d=32):
    ins = standardised(make_blocks(nb, d, 12, seed=7))
    return dict(name=f"{nb:,} uniform blocks of d = {d}", ins=ins, nb=nb, D=nb * d, longest=d,
                offs=None)


def c2low_shape():
    from bench_backfit_var import c2low_shape as shape
    sh = shape()
    offs = torch.from_numpy(np.asarray(sh["kw"]["block_off"], np.int64)).to(sh["t_loc"].device)
    return dict(name="the c2low item's standardised groups",
                ins=tuple(sh[k] for k in ("t_loc", "t_scale", "p_loc", "p_scale")), nb=sh["nb"],
                D=sh["D"], longest=sh["longest"], offs=offs)


class Plain:
    """The plain single-step encoder of library `lib` on sh's buffers."""

    def __init__(self, lib, sh):
        self.lib, self.sh = lib, sh
        dev = sh["ins"][0].device
        nb, D, d = sh["nb"], sh["D"], sh["longest"]
        self.idx = torch.empty((nb, 1), dtype=torch.int32, device=dev)
        self.sample = torch.empty(D, dtype=torch.float32, device=dev)
        need = lib.cwq_greedy_encode_uniform_defer_bytes(nb, d) if sh["offs"] is None \
            else lib.cwq_greedy_encode_workspace_size(nb, D, d)
        self.ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device=dev)

    def at(self, b):
        sh, lib = self.sh, self.lib
        ins = tuple(_ptr(t) for t in sh["ins"])
        st = torch.cuda.current_stream().cuda_stream
        if sh["offs"] is None:
            rc = lib.cwq_greedy_encode_uniform(*ins, sh["nb"], sh["longest"], b, 1, SEED, 1.0, 0,
                                               _ptr(self.idx), _ptr(self.sample),
                                               self.ws.data_ptr(), self.ws.numel(), None, st)
        else:
            rc = lib.cwq_greedy_encode(*ins, sh["offs"].data_ptr(), sh["nb"], sh["D"],
                                       sh["longest"], b, 1, SEED, 1.0, 0, _ptr(self.idx),
                                       _ptr(self.sample), self.ws.data_ptr(), self.ws.numel(),
                                       None, st)
        assert rc == 0, rc

    def loop(self, B):
        def call():
            for b in range(B + 1):
                self.at(b)
        return call


def table_call(lib, sh, B):
    dev = sh["ins"][0].device
    nb, D, d = sh["nb"], sh["D"], sh["longest"]
    idx = torch.empty((nb, B + 1), dtype=torch.int32, device=dev)
    value = torch.empty((nb, B + 1), dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.cwq_rate_table_workspace_bytes(nb, D, d, B)), dtype=torch.uint8,
                     device=dev)

    def call():
        rc = lib.cwq_rate_table(*(_ptr(t) for t in sh["ins"]),
                                None if sh["offs"] is None else sh["offs"].data_ptr(), nb, D, d, B,
                                SEED, 1.0, 0, _ptr(idx), _ptr(value), ws.data_ptr(), ws.numel(),
                                None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return call, idx, value, ws


def measure(sh, B, lib, plib, warmup, reps):
    table, idx, value, ws = table_call(lib, sh, B)
    par, here = Plain(plib, sh), Plain(lib, sh)
    t, lp = (stat(ms) for ms in rounds_ms([table, par.loop(B)], warmup, reps, alternate=True))
    # the table's columns are the loop's indices
    table()
    same = True
    for b in sorted({0, min(5, B), min(11, B), B}):
        par.at(b)
        same = same and bool(torch.equal(par.idx[:, 0], idx[:, b]))
    p, h = (stat(ms) for ms in rounds_ms([lambda: par.at(B), lambda: here.at(B)], warmup, reps,
                                         alternate=True))
    spread = lp["max_ms"] - lp["min_ms"]
    return {"shape": sh["name"], "blocks": sh["nb"], "dims": sh["D"], "longest_block": sh["longest"],
            "max_bits": B, "rate_table": t, "parent_loop_of_encodes": lp, "parent_calls": B + 1,
            "table_over_loop": t["median_ms"] / lp["median_ms"],
            "table_slower_than_loop_by_more_than_its_spread":
                t["median_ms"] > lp["median_ms"] + spread,
            "columns_equal_the_loops_indices": same, "workspace_mib": ws.numel() / 2 ** 20,
            "encode_at_B": {"parent": p, "this": h, "this_over_parent": h["median_ms"] / p["median_ms"],
                            "inside_parent_spread": p["min_ms"] <= h["median_ms"] <= p["max_ms"]}}


def mixed_blocks(nb, d):
    """bench_varbits.py's spread: blocks whose KL matches bits = clip(round(N(12, 2)), 4, 16)."""
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


def budgets(warmup, reps, nb=65536, d=32, B=16):
    made_for, blocks = mixed_blocks(nb, d)
    q = [torch.from_numpy(blocks[k].reshape(-1)).cuda()
         for k in ("post_loc", "post_scale", "prior_loc", "prior_scale")]
    kl_bits = C.block_bits(*q, block_dim=d, max_bits=B)
    idx, value = C.rate_table(*standardised(blocks), B, SEED, block_dim=d)
    total = int(kl_bits.sum().item())
    bits, lam = C.choose_bits_total(value, total)
    at = lambda b: value.gather(1, b.long().unsqueeze(1)).double().reshape(-1)  # noqa: E731
    gain = at(bits) - at(kl_bits)
    res = {"blocks": nb, "d": d, "max_bits": B,
           "made_for_bits_hist": np.bincount(made_for, minlength=B + 1).tolist(),
           "block_bits_total": total, "choose_bits_total_total": int(bits.sum().item()),
           "lam_nats_per_bit": lam,
           "block_bits_hist": np.bincount(kl_bits.cpu().numpy(), minlength=B + 1).tolist(),
           "choose_bits_hist": np.bincount(bits.cpu().numpy(), minlength=B + 1).tolist(),
           "mean_value_block_bits": float(at(kl_bits).mean().item()),
           "mean_value_choose_bits_total": float(at(bits).mean().item()),
           "mean_gain_nats_per_block": float(gain.mean().item()),
           "blocks_that_lose": int((gain < 0).sum().item())}
    # the two chooser calls on a table of 10^6 blocks (this table, tiled)
    big = value.repeat((10 ** 6 + nb - 1) // nb, 1)[:10 ** 6].contiguous()
    out = torch.empty(10 ** 6, dtype=torch.int32, device="cuda")
    tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib = _lib.load()

    def choose():
        rc = lib.cwq_choose_bits(_ptr(big), 10 ** 6, B, 0.6931471805599453, 0, B, _ptr(out),
                                 _ptr(tot), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    res["choose_bits_1e6_blocks"] = stat(rounds_ms([choose], warmup, reps)[0])
    target = int(C.block_bits(*q, block_dim=d, max_bits=B).sum().item()) * 10 ** 6 // nb
    ms = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        C.choose_bits_total(big, target)
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    res["choose_bits_total_1e6_blocks_host_wall"] = stat(ms)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=7, help="timed rounds per figure (at least 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="u32,c2low,budgets")
    ap.add_argument("--parent-lib", required=True,
                    help="a libcwq.so built from the parent commit (the baseline)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    S.VERBOSE = False
    torch.cuda.set_device(0)
    lib = bind(_lib.load(), ENCODERS + ["cwq_rate_table", "cwq_rate_table_workspace_bytes"])
    plib = bind(ctypes.CDLL(a.parent_lib), ENCODERS)
    plib.cwq_version.restype = ctypes.c_int
    ver = plib.cwq_version()
    reps, only = max(a.reps, 5), a.only.split(",")
    result = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "timed_rounds": reps,
              "parent_abi": f"{ver >> 16}.{ver & 0xffff}", "tables": []}

    def keep():
        if a.out:  # keep what is measured so far
            with open(a.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    if "u32" in only:
        sh = u32_shape()
        for B in (8, 11, 16):
            result["tables"].append(measure(sh, B, lib, plib, a.warmup, reps))
            keep()
        del sh
    if "c2low" in only:
        result["tables"].append(measure(c2low_shape(), 9, lib, plib, a.warmup, reps))
        keep()
    if "budgets" in only:
        result["budgets"] = budgets(a.warmup, reps)
        keep()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
