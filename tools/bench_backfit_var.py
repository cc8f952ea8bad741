#!/usr/bin/env python
"""Backfitting under per-block bit budgets measured on one MI355X (DESIGN.md
4h): ms per ``backfit_blocks_var`` call for 0 to 3 sweeps from the greedy table
of ``encode_blocks_var``, ms per sweep, the gain in the final log-density over
the starting table and the accepts per sweep.

  (lane)     65,536 uniform blocks of d = 32, 4 steps, per-step budgets
             clip(round(N(6, 1.5)), 2, 8)
  (control)  the same blocks, every budget 8
  (c2low)    the c2low item's standardised groups with block_bits(...,
             n_steps=30, max_bits=14) budgets (DESIGN.md 4e's case)

Per figure: HIP events around the whole call on the current stream, warm-up
calls first, then the median of the timed calls; every call's time is kept.

The units are the parent commit's library (``--parent-lib``, loaded directly:
the bindings refuse another ABI version, and the two calls' argument lists are
the same in both versions), on the same buffers in the same process, its calls
interleaved call by call with this build's: the budget encode on the same
budgets, and cwq_greedy_backfit (0 and 1 sweeps) at the call's largest budget.
One JSON object on stdout.
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
from compression_without_quantization_amd.backfit import backfit_var_workspace_bytes  # noqa: E402
from compression_without_quantization_amd.varbits import _ptr  # noqa: E402
from bench_backfit import event_ms  # noqa: E402
from bench_beam import lane_shape  # noqa: E402
from bench_pln_var import D_C2, c2low_latents  # noqa: E402

SWEEPS = (0, 1, 2, 3)
SEED = 42


def lane(control):
    sh = lane_shape()
    rng = np.random.Generator(np.random.PCG64(11))
    bits = np.clip(np.rint(rng.normal(6.0, 1.5, sh["nb"])), 2, 8).astype(np.int32)
    if control:
        bits[:] = 8
    sh["bits"] = torch.from_numpy(bits).to(sh["t_loc"].device)
    sh["name"] = "65,536 uniform blocks of d = 32, 4 steps, " + \
        ("every budget 8 (control)" if control else "budgets clip(round(N(6, 1.5)), 2, 8)")
    return sh


def c2low_shape():
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    q_loc, q_scale, p_loc, p_scale = c2low_latents()
    t_loc, t_scale, kl = (torch.empty(D_C2, dtype=torch.float32, device=dev) for _ in range(3))
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.cwq_standardise(_ptr(q_loc), _ptr(q_scale), _ptr(p_loc), _ptr(p_scale), D_C2,
                                   _ptr(t_loc), _ptr(t_scale), st), "cwq_standardise")
    _lib.check(lib.cwq_kl_normal_normal(_ptr(q_loc), _ptr(q_scale), _ptr(p_loc), _ptr(p_scale),
                                        D_C2, _ptr(kl), st), "cwq_kl_normal_normal")
    starts = np.asarray(C.group_starts(kl.cpu().numpy(), 14 * 30), dtype=np.int64)
    bits = C.block_bits(q_loc, q_scale, p_loc, p_scale, block_off=starts, n_steps=30, max_bits=14)
    return dict(name="the c2low item's standardised groups, 30 steps, block_bits budgets up to 14",
                t_loc=t_loc, t_scale=t_scale, p_loc=torch.zeros(D_C2, device=dev),
                p_scale=torch.ones(D_C2, device=dev), bits=bits, n_steps=30,
                nb=int(starts.size - 1), D=D_C2, longest=int(np.diff(starts).max()),
                kw=dict(block_off=starts))


def raw_calls(lib, sh, top, table_top):
    """(budget encode, cwq_greedy_backfit at `top` bits with 0 sweeps, with 1)
    of the library `lib` on sh's buffers; the backfit calls restore their table
    (a device copy) inside the call, in both builds alike."""
    names = ["cwq_greedy_encode_var", "cwq_greedy_encode_uniform_var", "cwq_greedy_backfit",
             "cwq_greedy_encode_var_workspace_size", "cwq_greedy_encode_uniform_var_workspace_size",
             "cwq_greedy_backfit_workspace_size"]
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    dev = sh["t_loc"].device
    nb, D, d, n = sh["nb"], sh["D"], sh["longest"], sh["n_steps"]
    uniform = "block_dim" in sh["kw"]
    offs = None if uniform else torch.from_numpy(np.asarray(sh["kw"]["block_off"])).to(dev)
    idx = torch.empty((nb, n), dtype=torch.int32, device=dev)
    sample = torch.empty(D, dtype=torch.float32, device=dev)
    ins = tuple(_ptr(sh[k]) for k in ("t_loc", "t_scale", "p_loc", "p_scale"))
    need = (lib.cwq_greedy_encode_uniform_var_workspace_size(nb, d) if uniform
            else lib.cwq_greedy_encode_var_workspace_size(nb, D, d, n))
    ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device=dev)
    bws = torch.empty(max(int(lib.cwq_greedy_backfit_workspace_size(nb, D, d, n)), 1),
                      dtype=torch.uint8, device=dev)

    def encode():
        st = torch.cuda.current_stream().cuda_stream
        if uniform:
            rc = lib.cwq_greedy_encode_uniform_var(*ins, nb, d, _ptr(sh["bits"]), n, SEED, 1.0, 0,
                                                   _ptr(idx), _ptr(sample), ws.data_ptr(),
                                                   ws.numel(), None, st)
        else:
            rc = lib.cwq_greedy_encode_var(*ins, offs.data_ptr(), nb, D, d, _ptr(sh["bits"]), n,
                                           SEED, 1.0, 0, _ptr(idx), _ptr(sample), ws.data_ptr(),
                                           ws.numel(), None, st)
        assert rc == 0, rc

    def backfit(sweeps):
        def call():
            idx.copy_(table_top)
            rc = lib.cwq_greedy_backfit(*ins, None if uniform else offs.data_ptr(), nb, D, d, top,
                                        n, sweeps, SEED, 1.0, 0, _ptr(idx), _ptr(sample), None,
                                        None, bws.data_ptr(), bws.numel(), None,
                                        torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
        return call

    return [encode, backfit(0), backfit(1)], (idx, sample, ws, bws, offs)


def measure(sh, warmup, reps, parent, parent_first=False, units_only=False, top_sweep=True):
    dev = sh["t_loc"].device
    ins = (sh["t_loc"], sh["t_scale"], sh["p_loc"], sh["p_scale"])
    bits, n = sh["bits"], sh["n_steps"]
    top = int(bits.max().item())
    res = {"shape": sh["name"], "blocks": sh["nb"], "dims": sh["D"], "longest_block": sh["longest"],
           "n_steps": n, "budget_hist": np.bincount(bits.cpu().numpy(), minlength=top + 1).tolist(),
           "code_bits": int(bits.sum().item()) * n, "warmup": warmup, "timed_calls": reps,
           "units": {}, "cases": []}
    table_top = C.encode_blocks(*ins, top, n, SEED, **sh["kw"])[0]
    labels = ["encode_blocks_var", "backfit_blocks_top_budget_0_sweeps",
              "backfit_blocks_top_budget_1_sweep"]
    if not top_sweep:  # (a long-block shape: the one-budget call walks each row with a lane)
        labels = labels[:2]
    fns, keep = raw_calls(_lib.load(), sh, top, table_top)
    fns = fns[:len(labels)]
    names = [k + "_this_build" for k in labels]
    if parent:
        plib = ctypes.CDLL(parent)
        plib.cwq_version.restype = ctypes.c_int
        ver = plib.cwq_version()
        res["parent_abi"] = f"{ver >> 16}.{ver & 0xffff}"
        pf, pkeep = raw_calls(plib, sh, top, table_top)
        # interleaved call by call: this build's, then the parent's, of each kind
        order = ("_parent_build", "_this_build") if parent_first else ("_this_build",
                                                                        "_parent_build")
        fns = [f for pair in (zip(pf, fns) if parent_first else zip(fns, pf)) for f in pair]
        names = [k + s for k in labels for s in order]
        res["interleave_order"] = [o.strip("_") for o in order]
    for label, ms in zip(names, event_ms(fns, warmup, reps)):
        res["units"][label] = {"ms": ms, "median_ms": float(np.median(ms)),
                               "spread_ms": float(max(ms) - min(ms))}
    if units_only:
        return res
    suffix = "_parent_build" if parent else "_this_build"
    unit = res["units"]["encode_blocks_var" + suffix]["median_ms"]
    ws = torch.empty(backfit_var_workspace_bytes(sh["nb"], sh["D"], sh["longest"], n,
                                                 uniform="block_dim" in sh["kw"]),
                     dtype=torch.uint8, device=dev)
    res["workspace_mib"] = ws.numel() / 2 ** 20
    table = C.encode_blocks_var(*ins, bits, n, SEED, **sh["kw"])[0]
    base_value, prev_acc = None, 0
    for k in SWEEPS:
        out = {}

        def call():
            out["r"] = C.backfit_blocks_var(table, *ins, bits, n, SEED, k, return_value=True,
                                            return_accepted=True, workspace=ws, **sh["kw"])
        ms = event_ms([call], warmup, reps)[0]
        _, _, value, acc = out["r"]
        value = value.double().cpu().numpy()
        acc = int(acc.sum().item())
        if k == 0:
            base_value = value
        gain = value - base_value
        row = {"sweeps": k, "ms": ms, "median_ms": float(np.median(ms)),
               "gain_nats_mean": float(gain.mean()), "gain_nats_min": float(gain.min()),
               "blocks_below_start": int((gain < 0).sum()), "accepted_total": acc,
               "accepted_this_sweep": acc - prev_acc}
        if k > 0:
            row["ms_per_sweep"] = (row["median_ms"] - res["cases"][0]["median_ms"]) / k
            row["sweep_over_encode_blocks_var"] = row["ms_per_sweep"] / unit
        prev_acc = acc
        res["cases"].append(row)
    for k, label in list(enumerate(labels))[1:]:
        k -= 1
        res[f"call_minus_backfit_blocks_top_budget_{k}_sweeps_ms"] = \
            res["cases"][k]["median_ms"] - res["units"][label + suffix]["median_ms"]
    res["no_block_below_start"] = all(r["gain_nats_min"] >= 0 for r in res["cases"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per figure (at least 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="lane,control,c2low")
    ap.add_argument("--parent-lib", default=None,
                    help="a libcwq.so built from the parent commit (the units)")
    ap.add_argument("--parent-first", action="store_true",
                    help="interleave the parent's call before this build's (default: after)")
    ap.add_argument("--units-only", action="store_true", help="the units alone, no sweeps")
    ap.add_argument("--no-top-sweep", action="store_true",
                    help="leave out the one-budget call with a sweep (minutes on c2low)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    S.VERBOSE = False
    torch.cuda.set_device(0)
    result = {"device": torch.cuda.get_device_name(0), "shapes": []}
    makers = (("lane", lambda: lane(False)), ("control", lambda: lane(True)),
              ("c2low", c2low_shape))
    for name, make in makers:
        if name in a.only.split(","):
            result["shapes"].append(measure(make(), a.warmup, max(a.reps, 5), a.parent_lib,
                                            a.parent_first, a.units_only, not a.no_top_sweep))
            if a.out:  # keep what is measured so far
                with open(a.out, "w") as f:
                    f.write(json.dumps(result) + "\n")
    print(json.dumps(result))
    bad = [s["shape"] for s in result["shapes"] if not s.get("no_block_below_start", True)]
    if bad:
        sys.exit(f"a block ended below its start on: {bad}")


if __name__ == "__main__":
    main()
