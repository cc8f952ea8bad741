"""Units-per-candidate histogram of the pruned encoder (run on the GPU box
with a -DCWQ_PRUNE_STATS build selected through CWQ_LIB_PATH).
Usage: CWQ_LIB_PATH=tools/vrun/libcwq_stats.so python tools/prune_stats.py [nb] [mode]
(PS_D / PS_BITS select the block shape; default the C4 shape d=32, 16 bits)
--guess G runs the screening pass with the tau guess in mode G (0 off, 1 on, 2
every tile retried; cwq_selftest_encode_uniform_tau_guess); --guess-ab runs
modes 0 and 1 in turn and prints both."""
import ctypes, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from compression_without_quantization_amd import _lib
import compression_without_quantization_amd as C
from compression_without_quantization_amd.synthetic import make_blocks

nb = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 20000
mode = int(sys.argv[2]) if len(sys.argv) > 2 and not sys.argv[2].startswith("-") else 2
d = int(os.environ.get("PS_D", "32"))
bits = int(os.environ.get("PS_BITS", "16"))
lib = _lib.load()
h = make_blocks(nb, d, bits, seed=20261015)
t = {k: torch.from_numpy(v.reshape(-1)).cuda() for k, v in h.items()}
out = (ctypes.c_ulonglong * 72)()


def opt(name, default=None):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def encode(guess):
    if guess is None:
        i, _ = C.encode_blocks(t["post_loc"], t["post_scale"], t["prior_loc"], t["prior_scale"],
                               bits, 1, 42, block_dim=d, prune_mode=mode)
        return i
    i = torch.empty((nb, 1), dtype=torch.int32, device="cuda")
    smp = torch.empty(nb * d, dtype=torch.float32, device="cuda")
    ws = torch.empty(max(1, int(lib.cwq_greedy_encode_uniform_workspace_size(nb, d))),
                     dtype=torch.uint8, device="cuda")
    rc = lib.cwq_selftest_encode_uniform_tau_guess(
        t["post_loc"].data_ptr(), t["post_scale"].data_ptr(), t["prior_loc"].data_ptr(),
        t["prior_scale"].data_ptr(), nb, d, bits, 1, 42, 1.0, 0, i.data_ptr(), smp.data_ptr(),
        ws.data_ptr(), ws.numel(), _lib.options(mode, None),
        torch.cuda.current_stream().cuda_stream, guess)
    _lib.check(rc, "cwq_selftest_encode_uniform_tau_guess")
    return i


def run(flags, guess=None):
    lib.cwq_debug_prune_stats(out, 1 | flags)
    i = encode(guess)
    torch.cuda.synchronize()
    assert lib.cwq_debug_prune_stats(out, 1) == 1, "not a CWQ_PRUNE_STATS build"
    return i.cpu().numpy(), np.array(out[:], dtype=np.float64)


if "--guess-ab" in sys.argv:   # the tau guess off and on: same indices, units of each
    res = [run(4, g) for g in (0, 1)]
    assert np.array_equal(res[0][0], res[1][0]), "indices differ between guess modes"
    for g, (_, b) in zip((0, 1), res):
        # a retried tile's first pass is counted too: units over the real candidates
        print(f"guess {g}: units/candidate {(b[:65] * np.arange(65)).sum() / (nb * 2.0 ** bits):.4f}"
              f", tiles with a guess {b[50]:.0f}, retried {b[51]:.0f} of {b[67]:.0f} screened")
i0, a = run(4, opt("--guess"))
if "--oracle-tau" in sys.argv:   # second launch seeded with each block's exact best value
    i1, a = run(2)
    lib.cwq_debug_prune_stats(out, 4)
    assert np.array_equal(i0, i1)
    print("oracle tau: each tile starts at its exact best value")
hist = a[:65]
ncand = hist.sum()
print(f"blocks {nb} mode {mode}: candidates finished {ncand:.0f} (expected {nb * 2**bits})")
print("units/candidate %.4f" % ((hist * np.arange(65)).sum() / ncand))
if a[50] or a[51]:   # tau guess: a retried tile's candidates are counted in both passes
    print(f"tiles with a tau guess {a[50]:.0f}, retried {a[51]:.0f}; units per real candidate "
          f"{(hist * np.arange(65)).sum() / (nb * 2.0 ** bits):.4f}")
for k in range(1, 65):
    if hist[k]:
        print(f"  finished after {k:2d} units: {hist[k] / ncand:.5f}")
print(f"completed rows {a[65]:.0f} ({a[65] / nb:.2f}/block), survivors pushed {a[66]:.0f} "
      f"({a[66] / nb:.2f}/block), screened tiles {a[67]:.0f}")
print(f"survivors re-evaluated exactly {a[68]:.0f} ({a[68] / nb:.2f}/block), "
      f"in-loop exact evaluations (list full) {a[69]:.0f}")
if a[71]:  # builds with the static-stride refill count their loop iterations
    print(f"wave-iterations {a[71]:.0f}, of them through the pool refill {a[70]:.0f} "
          f"({a[70] / a[71]:.4f})")
if "--json" in sys.argv:   # record for bench.py's roofline.valu.evaluated
    import json
    path = sys.argv[sys.argv.index("--json") + 1]
    with open(path, "w") as f:
        json.dump({"config": os.environ.get("PS_CONFIG", "c4"), "blocks": nb, "block_dim": d,
                   "kl_bits": bits, "prune_mode": mode,
                   "units_per_candidate": float((hist * np.arange(65)).sum() / ncand),
                   "unit_dims": 4, "candidates": float(ncand),
                   "survivors_exact_per_block": float(a[68] / nb),
                   "method": "tools/prune_stats.py on a -DCWQ_PRUNE_STATS build of libcwq.so "
                             "(counters inside k_encode_prune; same inputs as bench.py --config "
                             "c4 but a block sample)"}, f, indent=1)
    print("wrote", path)
