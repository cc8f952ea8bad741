#!/usr/bin/env python
"""Backfitting measured on one MI355X: ms per call, the gain in
the final log-density over the starting table, and the accepts per sweep, for
0, 1, 2 and 3 sweeps from the greedy table and from a beam of 4.

  (lane)  65,536 uniform blocks of d = 32, 4 steps x 8 bits (DESIGN.md 4f's).
  (wave)  the standardised groups of the item ``bench.py --config c2cli``
          codes (196,608 dims), 30 steps x 14 bits.

Per case: HIP events around the whole ``backfit_blocks`` call on the current
stream, warm-up calls first, then the median of the timed calls; the mean and
the minimum over blocks of ``out_value(K) - out_value(0)`` in nats; the accepts
of sweep k as ``sum(out_accepted(k)) - sum(out_accepted(k - 1))``.

The yardstick for time is another build's ``encode_blocks``: ``--parent-lib``
names a libcwq.so built from the parent commit, whose cwq_greedy_encode and
cwq_beam_encode (beam 2) are called on the same buffers, interleaved call by
call with this build's ``encode_blocks``.  (The bindings refuse a library of
another ABI version, so the parent's is loaded here directly; the two calls'
argument lists are the same in both versions.)  One JSON object on stdout.
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
from compression_without_quantization_amd.backfit import backfit_workspace_bytes  # noqa: E402
from compression_without_quantization_amd.varbits import _ptr  # noqa: E402
from bench_beam import lane_shape, wave_shape  # noqa: E402

SWEEPS = (0, 1, 2, 3)
SEED = 42


def event_ms(fns, warmup, reps):
    """ms of every timed call of each fn in fns, the calls interleaved:
    events on the current stream around one call."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def parent_calls(path, sh):
    """(encode call, beam-2 call) of the library at path on sh's buffers."""
    lib = ctypes.CDLL(path)
    for name in ("cwq_greedy_encode", "cwq_greedy_encode_uniform", "cwq_beam_encode",
                 "cwq_greedy_encode_workspace_size", "cwq_greedy_encode_uniform_workspace_size",
                 "cwq_beam_encode_workspace_size"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    lib.cwq_version.restype = ctypes.c_int
    dev = sh["t_loc"].device
    nb, D, d, b, n = sh["nb"], sh["D"], sh["longest"], sh["n_bits"], sh["n_steps"]
    idx = torch.empty((nb, n), dtype=torch.int32, device=dev)
    sample = torch.empty(D, dtype=torch.float32, device=dev)
    ins = tuple(_ptr(sh[k]) for k in ("t_loc", "t_scale", "p_loc", "p_scale"))
    uniform = "block_dim" in sh["kw"]
    offs = None if uniform else torch.from_numpy(np.asarray(sh["kw"]["block_off"])).to(dev)
    need = (lib.cwq_greedy_encode_uniform_workspace_size(nb, d) if uniform
            else lib.cwq_greedy_encode_workspace_size(nb, D, d))
    ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device=dev)
    bws = torch.empty(max(int(lib.cwq_beam_encode_workspace_size(nb, D, d, n, 2)), 1),
                      dtype=torch.uint8, device=dev)

    def encode():
        st = torch.cuda.current_stream().cuda_stream
        if uniform:
            rc = lib.cwq_greedy_encode_uniform(*ins, nb, d, b, n, SEED, 1.0, 0, _ptr(idx),
                                               _ptr(sample), ws.data_ptr(), ws.numel(), None, st)
        else:
            rc = lib.cwq_greedy_encode(*ins, offs.data_ptr(), nb, D, d, b, n, SEED, 1.0, 0,
                                       _ptr(idx), _ptr(sample), ws.data_ptr(), ws.numel(), None, st)
        assert rc == 0, rc

    def beam2():
        st = torch.cuda.current_stream().cuda_stream
        rc = lib.cwq_beam_encode(*ins, None if uniform else offs.data_ptr(), nb, D, d, b, n, 2,
                                 SEED, 1.0, 0, _ptr(idx), _ptr(sample), None, bws.data_ptr(),
                                 bws.numel(), None, st)
        assert rc == 0, rc

    ver = lib.cwq_version()
    return encode, beam2, f"{ver >> 16}.{ver & 0xffff}", (idx, sample, ws, bws, offs)


def measure(sh, warmup, reps, parent):
    dev = sh["t_loc"].device
    args = (sh["t_loc"], sh["t_scale"], sh["p_loc"], sh["p_scale"], sh["n_bits"], sh["n_steps"],
            SEED)
    res = {"shape": sh["name"], "blocks": sh["nb"], "dims": sh["D"], "longest_block": sh["longest"],
           "n_bits_per_step": sh["n_bits"], "n_steps": sh["n_steps"], "warmup": warmup,
           "timed_calls": reps, "baselines": {}, "cases": []}
    fns = [lambda: C.encode_blocks(*args, **sh["kw"])]
    labels = ["encode_blocks_this_build"]
    if parent:
        enc, beam2, ver, keep = parent_calls(parent, sh)
        fns.append(enc)
        labels.append("encode_blocks_parent_build")
        res["parent_abi"] = ver
    for label, ms in zip(labels, event_ms(fns, warmup, reps)):
        res["baselines"][label] = {"ms": ms, "median_ms": float(np.median(ms))}
    if parent:
        ms = event_ms([beam2], 1, 3)[0]
        res["baselines"]["beam_2_parent_build"] = {"ms": ms, "median_ms": float(np.median(ms))}
    unit = res["baselines"][labels[-1]]["median_ms"]
    ws = torch.empty(backfit_workspace_bytes(sh["nb"], sh["D"], sh["longest"], sh["n_steps"]),
                     dtype=torch.uint8, device=dev)
    res["workspace_mib"] = ws.numel() / 2 ** 20
    starts = {"greedy": C.encode_blocks(*args, **sh["kw"])[0],
              "beam_4": C.encode_blocks_beam(*args, 4, **sh["kw"])[0]}
    for start, table in starts.items():
        base_value, prev_acc = None, 0
        for k in SWEEPS:
            out = {}

            def call():
                out["r"] = C.backfit_blocks(table, *args, k, return_value=True,
                                            return_accepted=True, workspace=ws, **sh["kw"])
            ms = event_ms([call], warmup, reps)[0]
            _, _, value, acc = out["r"]
            value = value.double().cpu().numpy()
            acc = int(acc.sum().item())
            if k == 0:
                base_value = value
            gain = value - base_value
            row = {"start": start, "sweeps": k, "ms": ms, "median_ms": float(np.median(ms)),
                   "gain_nats_mean": float(gain.mean()), "gain_nats_min": float(gain.min()),
                   "blocks_below_start": int((gain < 0).sum()), "accepted_total": acc,
                   "accepted_this_sweep": acc - prev_acc}
            if k > 0:
                zero = res["cases"][-k]["median_ms"]
                row["ms_per_sweep"] = (row["median_ms"] - zero) / k
                row["sweep_over_encode_blocks"] = row["ms_per_sweep"] / unit
            prev_acc = acc
            res["cases"].append(row)
    if parent:
        one = next(r for r in res["cases"] if r["start"] == "greedy" and r["sweeps"] == 1)
        res["one_sweep_call_below_parent_beam_2"] = bool(
            one["median_ms"] < res["baselines"]["beam_2_parent_build"]["median_ms"])
    res["min_gain_nonnegative_everywhere"] = all(r["gain_nats_min"] >= 0 for r in res["cases"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per figure (at least 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="lane,wave")
    ap.add_argument("--parent-lib", default=None,
                    help="a libcwq.so built from the parent commit (the yardstick)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    S.VERBOSE = False
    torch.cuda.set_device(0)
    result = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for name, make in (("lane", lane_shape), ("wave", wave_shape)):
        if name in a.only.split(","):
            result["shapes"].append(measure(make(), a.warmup, max(a.reps, 5), a.parent_lib))
            if a.out:  # keep what is measured so far
                with open(a.out, "w") as f:
                    f.write(json.dumps(result) + "\n")
    print(json.dumps(result))
    bad = [s["shape"] for s in result["shapes"]
           if not s["min_gain_nonnegative_everywhere"]
           or s.get("one_sweep_call_below_parent_beam_2") is False and "c2cli" in s["shape"]]
    if bad:
        sys.exit(f"conditions of DESIGN.md 4g not met on: {bad}")


if __name__ == "__main__":
    main()
