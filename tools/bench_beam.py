#!/usr/bin/env python
"""The beam encoder measured on one MI355X: ms per call and the
gain in the final log-density over the greedy coder, for beams 1, 2, 4, 8, 16.

  (lane)  65,536 uniform blocks of d = 32, 4 steps x 8 bits: the lane-per-row
          scoring kernel.
  (wave)  the standardised groups of the item ``bench.py --config c2cli``
          codes (196,608 dims), 30 steps x 14 bits: the wave-per-row kernel.

Per beam: HIP events around the whole call on the current stream, warm-up
calls first, then the median of the timed calls; the mean and the minimum over
blocks of ``out_value(beam) - out_value(1)`` in nats.  Baselines from the same
build and run: ``encode_blocks`` at ``prune_mode=0`` (the arithmetic of beam 1
without the selection) and at the default.  One JSON object on stdout.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import compression_without_quantization_amd as C  # noqa: E402
import compression_without_quantization_amd.coded_greedy_sampler as S  # noqa: E402
from compression_without_quantization_amd import _lib  # noqa: E402
from compression_without_quantization_amd.beam import beam_workspace_bytes  # noqa: E402
from compression_without_quantization_amd.synthetic import make_blocks, make_latents  # noqa: E402
from compression_without_quantization_amd.varbits import _ptr  # noqa: E402

BEAMS = (1, 2, 4, 8, 16)
D_C2 = 32 * 48 * 128


def event_ms(fn, warmup, reps):
    """ms of every timed call: events on the current stream around one call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def lane_shape():
    nb, d, bits = 65536, 32, 8
    blk = make_blocks(nb, d, 4 * bits, seed=7)  # the code spends 4 steps x 8 bits per block
    dev = torch.device("cuda", 0)
    pl, ps = blk["prior_loc"].reshape(-1), blk["prior_scale"].reshape(-1)
    tl = ((blk["post_loc"].reshape(-1) - pl) / ps).astype(np.float32)
    ts = (blk["post_scale"].reshape(-1) / ps).astype(np.float32)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    D = nb * d
    return dict(name="65,536 uniform blocks of d = 32, 4 steps x 8 bits (lane per row)",
                t_loc=f(tl), t_scale=f(ts), p_loc=torch.zeros(D, device=dev),
                p_scale=torch.ones(D, device=dev), n_bits=bits, n_steps=4, nb=nb, D=D,
                longest=d, kw=dict(block_dim=d))


def wave_shape():
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    q_loc, q_scale, p_loc, p_scale = (torch.from_numpy(a).to(dev)
                                      for a in make_latents(D_C2, bits_per_dim=1.1, seed=0))
    t_loc, t_scale, kl = (torch.empty(D_C2, dtype=torch.float32, device=dev) for _ in range(3))
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.cwq_standardise(_ptr(q_loc), _ptr(q_scale), _ptr(p_loc), _ptr(p_scale), D_C2,
                                   _ptr(t_loc), _ptr(t_scale), st), "cwq_standardise")
    _lib.check(lib.cwq_kl_normal_normal(_ptr(q_loc), _ptr(q_scale), _ptr(p_loc), _ptr(p_scale),
                                        D_C2, _ptr(kl), st), "cwq_kl_normal_normal")
    starts = np.asarray(C.group_starts(kl.cpu().numpy(), 14 * 30), dtype=np.int64)
    return dict(name="the c2cli item's standardised groups, 30 steps x 14 bits (wave per row)",
                t_loc=t_loc, t_scale=t_scale, p_loc=torch.zeros(D_C2, device=dev),
                p_scale=torch.ones(D_C2, device=dev), n_bits=14, n_steps=30,
                nb=int(starts.size - 1), D=D_C2, longest=int(np.diff(starts).max()),
                kw=dict(block_off=starts))


def measure(sh, beams, warmup, reps):
    dev = sh["t_loc"].device
    args = (sh["t_loc"], sh["t_scale"], sh["p_loc"], sh["p_scale"], sh["n_bits"], sh["n_steps"], 42)
    res = {"shape": sh["name"], "blocks": sh["nb"], "dims": sh["D"], "longest_block": sh["longest"],
           "n_bits_per_step": sh["n_bits"], "n_steps": sh["n_steps"], "warmup": warmup,
           "timed_calls": reps, "baselines": {}, "beams": []}
    for label, mode in (("encode_blocks_prune_mode_0", 0), ("encode_blocks_default", None)):
        ms = event_ms(lambda: C.encode_blocks(*args, prune_mode=mode, **sh["kw"]), warmup, reps)
        res["baselines"][label] = {"ms": ms, "median_ms": float(np.median(ms))}
    greedy_idx, _ = C.encode_blocks(*args, **sh["kw"])
    base_value = None
    for beam in beams:
        ws = torch.empty(beam_workspace_bytes(sh["nb"], sh["D"], sh["longest"], sh["n_steps"], beam),
                         dtype=torch.uint8, device=dev)
        out = {}

        def call():
            out["r"] = C.encode_blocks_beam(*args, beam, return_value=True, workspace=ws,
                                            **sh["kw"])
        ms = event_ms(call, warmup, reps)
        idx, _, value = out["r"]
        value = value.double().cpu().numpy()
        row = {"beam": beam, "ms": ms, "median_ms": float(np.median(ms)),
               "workspace_mib": ws.numel() / 2 ** 20}
        if beam == 1:
            base_value = value
            row["equals_encode_blocks"] = bool(torch.equal(idx, greedy_idx))
        if base_value is not None:
            gain = value - base_value
            row.update(gain_nats_mean=float(gain.mean()), gain_nats_min=float(gain.min()),
                       blocks_below_greedy=int((gain < 0).sum()))
        res["beams"].append(row)
        del ws
    t = {r["beam"]: r["median_ms"] for r in res["beams"]}
    if 1 in t:
        res["beam1_over_prune_mode_0"] = t[1] / res["baselines"]["encode_blocks_prune_mode_0"][
            "median_ms"]
        if 16 in t:
            res["beam16_over_beam1"] = t[16] / t[1]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per figure (at least 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="lane,wave")
    ap.add_argument("--beams", default=",".join(map(str, BEAMS)))
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    S.VERBOSE = False
    torch.cuda.set_device(0)
    beams = [int(b) for b in a.beams.split(",")]
    result = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for name, make in (("lane", lane_shape), ("wave", wave_shape)):
        if name in a.only.split(","):
            result["shapes"].append(measure(make(), beams, a.warmup, max(a.reps, 5)))
            if a.out:  # keep what is measured so far
                with open(a.out, "w") as f:
                    f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
