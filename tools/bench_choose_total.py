#!/usr/bin/env python
"""Budgets under a bit total measured on one MI355X: ms per
``cwq_choose_bits_total`` call against the parent commit's way to the same
budgets, the host loop of ``choose_bits_total`` (one ``cwq_choose_bits`` call and
one read of its total per halving) run through the parent commit's library
(``--parent-lib``, loaded directly: the bindings refuse another ABI version, and
the argument lists used here are the same in both), on the same buffers in the
same process.

  (solver)  a table of 10^6 blocks x 17 budgets and one of 65,536 x 9
  (encode)  ``cwq_greedy_encode_rate`` against the parent's
            ``encode_blocks_rate(total_bits=...)`` (table, host loop, gather,
            decode) at 65,536 uniform blocks of d = 32, B = 8 and B = 16

Per figure: HIP events around the whole call on the current stream, outputs and
workspaces allocated beforehand, warm-up rounds first, then interleaved rounds
whose order alternates; every call's time is kept, the median is quoted with
its range.  ``slowest_below_parents_fastest`` is the pass mark of 4k.
``--variant-lib`` (repeatable, ``r=path``): the solver of other builds of this
tree (``-DCWQ_SOLVE_LEVELS=r``) timed in the same rounds, for the choice of r.

One JSON object on stdout and in ``--out`` (profiles/choose_total_bench.json,
the committed record: ``python tools/bench_choose_total.py --parent-lib PARENT.so
--variant-lib 4=R4.so --variant-lib 5=R5.so --variant-lib 6=R6.so``).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import compression_without_quantization_amd as C  # noqa: E402
import compression_without_quantization_amd.coded_greedy_sampler as S  # noqa: E402
from compression_without_quantization_amd import _lib  # noqa: E402
from compression_without_quantization_amd.varbits import _ptr  # noqa: E402
from bench_beam_var import bind, rounds_ms, stat  # noqa: E402
from bench_rate_table import mixed_blocks, standardised, u32_shape  # noqa: E402

SEED = 42
PARENT = ["cwq_rate_table", "cwq_rate_table_workspace_bytes", "cwq_choose_bits",
          "cwq_greedy_decode_uniform"]
NEW = ["cwq_choose_bits_total", "cwq_choose_bits_total_workspace_bytes", "cwq_greedy_encode_rate",
       "cwq_greedy_encode_rate_workspace_bytes"]


def host_loop(lib, value, total_bits, bits, total):
    """ratetable.choose_bits_total's loop on library `lib` (min_bits = 0, the
    whole table); returns lam."""
    nb, B = value.shape[0], value.shape[1] - 1
    st = torch.cuda.current_stream().cuda_stream

    def total_at(lam):
        rc = lib.cwq_choose_bits(_ptr(value), nb, B, float(lam), 0, B, _ptr(bits), _ptr(total), st)
        assert rc == 0, rc
        return int(total.item())

    if total_at(0.0) <= total_bits:
        return 0.0
    span = value.double() - value[:, :1].double()
    lam_lo, lam_hi = 0.0, float(span.max().item())
    for _ in range(60):
        mid = 0.5 * (lam_lo + lam_hi)
        if total_at(mid) <= total_bits:
            lam_hi = mid
        else:
            lam_lo = mid
    total_at(lam_hi)
    return lam_hi


class Solver:
    """cwq_choose_bits_total of library `lib` on `value`, buffers made once."""

    def __init__(self, lib, value, total_bits):
        self.lib, self.value, self.T = lib, value, total_bits
        nb, self.B = value.shape[0], value.shape[1] - 1
        dev = value.device
        self.bits = torch.empty(nb, dtype=torch.int32, device=dev)
        self.lam = torch.empty(1, dtype=torch.float64, device=dev)
        self.total = torch.empty(1, dtype=torch.int64, device=dev)
        self.ws = torch.empty(int(lib.cwq_choose_bits_total_workspace_bytes(self.B)),
                              dtype=torch.uint8, device=dev)

    def __call__(self):
        rc = self.lib.cwq_choose_bits_total(
            _ptr(self.value), self.value.shape[0], self.B, self.T, 0, self.B, _ptr(self.bits),
            _ptr(self.lam), _ptr(self.total), self.ws.data_ptr(), self.ws.numel(),
            torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc


def verdict(new, parent):
    return {"this": new, "parent": parent, "parent_over_this": parent["median_ms"] / new["median_ms"],
            "slowest_below_parents_fastest": new["max_ms"] < parent["min_ms"]}


def measure_solver(name, value, total_bits, lib, plib, variants, warmup, reps):
    nb = value.shape[0]
    new = Solver(lib, value, total_bits)
    others = [(r, Solver(v, value, total_bits)) for r, v in variants]
    pbits = torch.empty(nb, dtype=torch.int32, device=value.device)
    ptotal = torch.zeros(1, dtype=torch.int64, device=value.device)
    plam = [None]

    def parent():
        plam[0] = host_loop(plib, value, total_bits, pbits, ptotal)

    fns = [new, parent] + [s for _, s in others]
    ms = [stat(m) for m in rounds_ms(fns, warmup, reps, alternate=True)]
    new()
    parent()
    torch.cuda.synchronize()
    same = bool(torch.equal(new.bits, pbits)) and \
        np.float64(new.lam.item()).view(np.uint64) == np.float64(plam[0]).view(np.uint64)
    res = {"table": name, "blocks": nb, "budgets": value.shape[1], "total_bits": total_bits,
           "table_mib": value.numel() * 4 / 2 ** 20, "lam": plam[0],
           "total_chosen": int(new.total.item()), "equal_to_the_parent_loop": bool(same),
           "workspace_bytes": new.ws.numel()}
    res.update(verdict(ms[0], ms[1]))
    for (r, s), m in zip(others, ms[2:]):
        torch.cuda.synchronize()
        s()
        torch.cuda.synchronize()
        res[f"variant_r{r}"] = dict(m, equal=bool(torch.equal(s.bits, pbits) and
                                                  torch.equal(s.lam, new.lam)))
    return res


def measure_encode(sh, B, lib, plib, warmup, reps):
    dev = sh["ins"][0].device
    nb, D, d = sh["nb"], sh["D"], sh["longest"]
    T = nb * B // 2
    ins = tuple(_ptr(t) for t in sh["ins"])
    out = {k: (torch.empty((nb, 1), dtype=torch.int32, device=dev),
               torch.empty(D, dtype=torch.float32, device=dev),
               torch.empty(nb, dtype=torch.int32, device=dev)) for k in ("this", "parent")}
    lam = torch.empty(1, dtype=torch.float64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.cwq_greedy_encode_rate_workspace_bytes(nb, D, d, B)), dtype=torch.uint8,
                     device=dev)
    tidx = torch.empty((nb, B + 1), dtype=torch.int32, device=dev)
    tval = torch.empty((nb, B + 1), dtype=torch.float32, device=dev)
    pws = torch.empty(int(plib.cwq_rate_table_workspace_bytes(nb, D, d, B)), dtype=torch.uint8,
                      device=dev)
    ptotal = torch.zeros(1, dtype=torch.int64, device=dev)

    def new():
        idx, sample, bits = out["this"]
        rc = lib.cwq_greedy_encode_rate(*ins, None, nb, D, d, B, T, 0, SEED, 1.0, 0, _ptr(idx),
                                        _ptr(sample), _ptr(bits), _ptr(lam), _ptr(total), None,
                                        ws.data_ptr(), ws.numel(), None,
                                        torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def parent():  # encode_blocks_rate(total_bits=T) on the parent's library
        idx, sample, bits = out["parent"]
        st = torch.cuda.current_stream().cuda_stream
        rc = plib.cwq_rate_table(*ins, None, nb, D, d, B, SEED, 1.0, 0, _ptr(tidx), _ptr(tval),
                                 pws.data_ptr(), pws.numel(), None, st)
        assert rc == 0, rc
        host_loop(plib, tval, T, bits, ptotal)
        idx.copy_(tidx.gather(1, bits.long().unsqueeze(1)))
        rc = plib.cwq_greedy_decode_uniform(_ptr(idx), ins[2], ins[3], nb, d, 30, 1, SEED, 1.0, 0,
                                            _ptr(sample), st)
        assert rc == 0, rc

    ms = [stat(m) for m in rounds_ms([new, parent], warmup, reps, alternate=True)]
    new()
    parent()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a, b)) for a, b in zip(out["this"], out["parent"]))
    res = {"shape": sh["name"], "blocks": nb, "dims": D, "max_bits": B, "total_bits": T,
           "total_chosen": int(total.item()), "lam": float(lam.item()),
           "equal_to_the_parent": same, "workspace_mib": ws.numel() / 2 ** 20}
    res.update(verdict(ms[0], ms[1]))
    return res


def tables():
    """The 10^6 x 17 table of bench_rate_table.py's budgets (a 65,536-block
    table of mixed KLs, tiled), and a 65,536 x 9 table; each with the total its
    blocks' block_bits budgets spend, or three quarters of what lam = 0 spends
    where that is less."""
    nb, d = 65536, 32
    _, blocks = mixed_blocks(nb, d)
    q = [torch.from_numpy(blocks[k].reshape(-1)).cuda()
         for k in ("post_loc", "post_scale", "prior_loc", "prior_scale")]
    ins = standardised(blocks)
    for B, rows in ((16, 10 ** 6), (8, nb)):
        value = C.rate_table(*ins, B, SEED, block_dim=d)[1]
        per_table = int(C.block_bits(*q, block_dim=d, max_bits=B).sum().item())
        big = value.repeat((rows + nb - 1) // nb, 1)[:rows].contiguous()
        free = int(C.choose_bits(big, 0.0).sum(dtype=torch.int64).item())
        # (at B = 8 these blocks' KLs ask for more than lam = 0 spends: the target must bind)
        yield f"{rows:,} blocks x {B + 1} budgets", big, min(per_table * rows // nb, 3 * free // 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=7, help="timed rounds per figure (at least 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="solver,encode")
    ap.add_argument("--parent-lib", required=True,
                    help="a libcwq.so built from the parent commit (the baseline)")
    ap.add_argument("--variant-lib", action="append", default=[],
                    help="r=path: a build of this tree with -DCWQ_SOLVE_LEVELS=r")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "choose_total_bench.json"),
                    help="the JSON is also written here (default: profiles/choose_total_bench.json)")
    a = ap.parse_args()
    S.VERBOSE = False
    torch.cuda.set_device(0)
    lib = bind(_lib.load(), PARENT + NEW)
    plib = bind(ctypes.CDLL(a.parent_lib), PARENT)
    plib.cwq_version.restype = ctypes.c_int
    ver = plib.cwq_version()
    variants = [(int(s.split("=", 1)[0]), bind(ctypes.CDLL(s.split("=", 1)[1]), NEW))
                for s in a.variant_lib]
    reps, only = max(a.reps, 5), a.only.split(",")
    result = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "timed_rounds": reps,
              "parent_abi": f"{ver >> 16}.{ver & 0xffff}", "solver": [], "encode": []}

    def keep():
        if a.out:  # keep what is measured so far
            with open(a.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    if "solver" in only:
        for name, value, total_bits in tables():
            result["solver"].append(measure_solver(name, value, total_bits, lib, plib, variants,
                                                   a.warmup, reps))
            keep()
    if "encode" in only:
        sh = u32_shape()
        for B in (8, 16):
            result["encode"].append(measure_encode(sh, B, lib, plib, a.warmup, reps))
            keep()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
