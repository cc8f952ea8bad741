#!/usr/bin/env python
"""The beam encoder under per-block bit budgets measured on one MI355X
(DESIGN.md 4i): ms per ``cwq_beam_encode_var`` call and the gain in the final
log-density over beam 1, for beams 1, 2, 4, 8, 16.

  (lane)   65,536 uniform blocks of d = 32, 4 steps, per-step budgets
           clip(round(N(6, 1.5)), 2, 8)  (DESIGN.md 4h's blocks)
  (c2low)  the c2low item's standardised groups with block_bits(...,
           n_steps=30, max_bits=14) budgets (DESIGN.md 4e's case)

Per figure: HIP events around the whole call on the current stream, warm-up
calls first, then the median of the timed calls; every call's time is kept.
Every line is held against the parent commit's library (``--parent-lib``,
loaded directly: the bindings refuse another ABI version, and cwq_beam_encode's
argument list is the same in both), on the same buffers in the same process:

  (a) mixed budgets.  What a caller could do before this call existed: the
      blocks sorted by budget beforehand (the sort, the gather and the scatter
      are NOT timed: they are left out in the baseline's favour), then one
      parent cwq_beam_encode per distinct budget on that budget's slice.  The
      var call runs on the unsorted blocks.  Calls interleaved.
  (b) every budget equal to b (``--equal-bits``: 8 on the lane shape, 14 on
      c2low, cwq_beam_encode's cases in DESIGN.md 4f).  The parent's
      cwq_beam_encode at b against this build's, in rounds whose order
      alternates (P H, H P, ...); ``fixed_inside_parent_spread`` says whether
      this build's median lies inside the parent's own run-to-run range.  The
      var call at every budget b is then timed against this build's fixed call
      in alternating rounds of their own.

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

import compression_without_quantization_amd.coded_greedy_sampler as S  # noqa: E402
from compression_without_quantization_amd import _lib  # noqa: E402
from compression_without_quantization_amd.varbits import _ptr  # noqa: E402
from bench_backfit_var import c2low_shape, lane  # noqa: E402

BEAMS = (1, 2, 4, 8, 16)
SEED = 42


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rounds_ms(fns, warmup, reps, alternate=False):
    """ms of every timed call of each fn, one call of each per round; with
    ``alternate`` odd rounds run the fns in reverse order."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for r in range(reps):
        order = range(len(fns))
        for k in (reversed(order) if alternate and r % 2 else order):
            out[k].append(timed(fns[k]))
    return out


def stat(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)),
            "max_ms": float(max(ms))}


def bind(lib, names):
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


class Buffers:
    """The shape's inputs on the device, outputs and one workspace for beam B."""

    def __init__(self, sh, lib, beam):
        dev = sh["t_loc"].device
        self.nb, self.D, self.d, self.n = sh["nb"], sh["D"], sh["longest"], sh["n_steps"]
        self.uniform = "block_dim" in sh["kw"]
        self.off_h = None if self.uniform else np.asarray(sh["kw"]["block_off"], np.int64)
        self.offs = None if self.uniform else torch.from_numpy(self.off_h).to(dev)
        self.ins = tuple(sh[k] for k in ("t_loc", "t_scale", "p_loc", "p_scale"))
        self.idx = torch.empty((self.nb, self.n), dtype=torch.int32, device=dev)
        self.sample = torch.empty(self.D, dtype=torch.float32, device=dev)
        self.value = torch.empty(self.nb, dtype=torch.float32, device=dev)
        need = int(lib.cwq_beam_encode_workspace_size(self.nb, self.D, self.d, self.n, beam))
        self.ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)


def var_call(lib, bf, bits, max_bits, beam):
    def call():
        rc = lib.cwq_beam_encode_var(
            *(_ptr(t) for t in bf.ins), None if bf.uniform else bf.offs.data_ptr(), bf.nb, bf.D,
            bf.d, _ptr(bits), max_bits, bf.n, beam, SEED, 1.0, 0, _ptr(bf.idx), _ptr(bf.sample),
            _ptr(bf.value), bf.ws.data_ptr(), bf.ws.numel(), None,
            torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return call


def fixed_call(lib, bf, b, beam):
    def call():
        rc = lib.cwq_beam_encode(
            *(_ptr(t) for t in bf.ins), None if bf.uniform else bf.offs.data_ptr(), bf.nb, bf.D,
            bf.d, b, bf.n, beam, SEED, 1.0, 0, _ptr(bf.idx), _ptr(bf.sample), _ptr(bf.value),
            bf.ws.data_ptr(), bf.ws.numel(), None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return call


def sorted_call(lib, bf, bits_h, beam):
    """One cwq_beam_encode of `lib` per distinct budget on the blocks sorted by
    budget (done here, untimed); outputs stay in sorted order (no scatter)."""
    dev = bf.idx.device
    order = np.argsort(bits_h, kind="stable")
    lens = np.full(bf.nb, bf.d, np.int64) if bf.uniform else np.diff(bf.off_h)
    starts = np.arange(bf.nb, dtype=np.int64) * bf.d if bf.uniform else bf.off_h[:-1]
    gather = np.concatenate([np.arange(starts[g], starts[g] + lens[g]) for g in order]) \
        if bf.D else np.zeros(0, np.int64)
    gi = torch.from_numpy(gather).to(dev)
    ins = tuple(t[gi].contiguous() for t in bf.ins)
    soff = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.int64)
    sb = bits_h[order]
    slices = []
    for b in np.unique(sb):
        r0, r1 = int(np.searchsorted(sb, b, "left")), int(np.searchsorted(sb, b, "right"))
        d0 = int(soff[r0])
        off = None if bf.uniform else torch.from_numpy(soff[r0:r1 + 1] - d0).to(dev)
        longest = bf.d if bf.uniform else int(lens[order][r0:r1].max())
        slices.append((int(b), r0, r1 - r0, d0, int(soff[r1]) - d0, longest, off))
    # a slice of few blocks is cut into more tiles each: its own workspace size
    need = max(int(lib.cwq_beam_encode_workspace_size(c[2], c[4], c[5], bf.n, beam))
               for c in slices)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    keep = (ins, gi, ws)

    def call():
        st = torch.cuda.current_stream().cuda_stream
        for b, r0, cnt, d0, dims, longest, off in slices:
            rc = lib.cwq_beam_encode(
                *(t.data_ptr() + 4 * d0 for t in ins), None if off is None else off.data_ptr(),
                cnt, dims, longest, b, bf.n, beam, SEED, 1.0, r0,
                bf.idx.data_ptr() + 4 * r0 * bf.n, bf.sample.data_ptr() + 4 * d0,
                bf.value.data_ptr() + 4 * r0, ws.data_ptr(), ws.numel(), None, st)
            assert rc == 0, rc
    return call, len(slices), keep


def measure(sh, beams, warmup, reps, parent, skip_control, skip_mixed, eq_bits):
    lib = bind(_lib.load(), ["cwq_beam_encode", "cwq_beam_encode_var",
                             "cwq_beam_encode_workspace_size"])
    plib = bind(ctypes.CDLL(parent), ["cwq_beam_encode", "cwq_beam_encode_workspace_size"])
    plib.cwq_version.restype = ctypes.c_int
    ver = plib.cwq_version()
    bits = sh["bits"]
    bits_h = bits.cpu().numpy()
    top = int(bits_h.max())
    eq = torch.full_like(bits, eq_bits)
    res = {"shape": sh["name"], "blocks": sh["nb"], "dims": sh["D"], "longest_block": sh["longest"],
           "n_steps": sh["n_steps"], "budget_hist": np.bincount(bits_h, minlength=top + 1).tolist(),
           "distinct_budgets": int(np.unique(bits_h).size), "max_bits": top,
           "code_bits": int(bits_h.sum()) * sh["n_steps"], "warmup": warmup, "timed_calls": reps,
           "parent_abi": f"{ver >> 16}.{ver & 0xffff}", "mixed": [], "equal": []}
    base_value = None
    for beam in beams:
        bf = Buffers(sh, lib, beam)
        if not skip_mixed:
            base_value = mixed(res, sh, lib, plib, bf, bits, bits_h, top, beam, warmup, reps,
                               base_value)
        if not skip_control:
            par, fix = fixed_call(plib, bf, eq_bits, beam), fixed_call(lib, bf, eq_bits, beam)
            p, h = (stat(ms) for ms in rounds_ms([par, fix], warmup, reps, alternate=True))
            # the var call against this build's fixed call, in rounds of their own
            h2, v = (stat(ms) for ms in rounds_ms([fix, var_call(lib, bf, eq, eq_bits, beam)],
                                                  warmup, reps, alternate=True))
            res["equal"].append({
                "beam": beam, "n_bits": eq_bits, "parent_fixed": p, "this_fixed": h,
                "this_fixed_beside_var": h2, "this_var": v,
                "fixed_over_parent": h["median_ms"] / p["median_ms"],
                "fixed_inside_parent_spread": p["min_ms"] <= h["median_ms"] <= p["max_ms"],
                "var_over_fixed": v["median_ms"] / h2["median_ms"]})
        del bf
    return res


def mixed(res, sh, lib, plib, bf, bits, bits_h, top, beam, warmup, reps, base_value):
    """Part (a) for one beam: a row of res["mixed"]; returns beam 1's values."""
    var = var_call(lib, bf, bits, top, beam)
    base, n_calls, keep = sorted_call(plib, bf, bits_h, beam)
    ms_var, ms_base = rounds_ms([var, base], warmup, reps)
    var()
    torch.cuda.synchronize()
    value = bf.value.double().cpu().numpy()
    if beam == 1:
        base_value = value
    row = {"beam": beam, "var": stat(ms_var), "parent_sorted_per_budget": stat(ms_base),
           "parent_calls": n_calls, "launches_var": 3 * sh["n_steps"] + 2,
           "launches_parent": n_calls * (3 * sh["n_steps"] + 2),
           "workspace_mib": bf.ws.numel() / 2 ** 20}
    row["var_over_parent"] = row["var"]["median_ms"] / row["parent_sorted_per_budget"][
        "median_ms"]
    if base_value is not None:
        gain = value - base_value
        row.update(gain_nats_mean=float(gain.mean()), gain_nats_min=float(gain.min()),
                   blocks_below_beam1=int((gain < 0).sum()))
    res["mixed"].append(row)
    del keep
    return base_value


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per figure (at least 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="lane,c2low")
    ap.add_argument("--beams", default=",".join(map(str, BEAMS)))
    ap.add_argument("--parent-lib", required=True,
                    help="a libcwq.so built from the parent commit (the baselines)")
    ap.add_argument("--skip-equal", action="store_true", help="leave out part (b)")
    ap.add_argument("--skip-mixed", action="store_true", help="leave out part (a)")
    ap.add_argument("--equal-bits", default="lane=8,c2low=14", help="part (b)'s b per shape")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    S.VERBOSE = False
    torch.cuda.set_device(0)
    beams = [int(b) for b in a.beams.split(",")]
    result = {"device": torch.cuda.get_device_name(0), "shapes": []}
    eq_bits = {k: int(v) for k, v in (kv.split("=") for kv in a.equal_bits.split(","))}
    for name, make in (("lane", lambda: lane(False)), ("c2low", c2low_shape)):
        if name in a.only.split(","):
            result["shapes"].append(measure(make(), beams, a.warmup, max(a.reps, 5), a.parent_lib,
                                            a.skip_equal, a.skip_mixed, eq_bits[name]))
            if a.out:  # keep what is measured so far
                with open(a.out, "w") as f:
                    f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
