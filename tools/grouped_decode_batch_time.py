"""Wall time of decode_grouped_greedy_sample_batch against a loop of
decode_grouped_greedy_sample (GPU box): 24 C2-size images (1 step x 8 bits,
~41.6k groups each) and one c2cli-shaped item (30 steps x 14 bits, groups of
up to 4,095 dims).  The two ways are timed interleaved, 3 rounds of 30 passes
each after a warm-up; prints per-image milliseconds, the single loop's spread
over the rounds and the ratio.  ``--once``: one pass of each way after the
warm-up and no timing loop (for a kernel trace of its own)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import compression_without_quantization_amd as C  # noqa: E402
import compression_without_quantization_amd.coded_greedy_sampler as S  # noqa: E402
from compression_without_quantization_amd.synthetic import make_latents  # noqa: E402

S.VERBOSE = False
ONCE = "--once" in sys.argv
dev = torch.device("cuda", 0)
ROUNDS, PASSES = 3, 30


def items(n, D, seed0):
    t, p = [], []
    for k in range(n):
        q_loc, q_scale, p_loc, p_scale = make_latents(D, bits_per_dim=1.1, seed=seed0 + k)
        t.append(C.Normal(torch.from_numpy(q_loc).to(dev), torch.from_numpy(q_scale).to(dev)))
        p.append(C.Normal(torch.from_numpy(p_loc).to(dev), torch.from_numpy(p_scale).to(dev)))
    return t, p


def lap(f, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def compare(name, n_items, D, n_steps, bits, mgsb):
    t, p = items(n_items, D, 0)
    enc = C.code_grouped_greedy_sample_batch(None, t, p, n_steps, bits, 42,
                                             max_group_size_bits=mgsb)
    codes, starts = [e[1] for e in enc], [e[2] for e in enc]

    def single():
        return [C.decode_grouped_greedy_sample(None, codes[i], starts[i], p[i], bits, n_steps, 42)
                for i in range(n_items)]

    def batch():
        return C.decode_grouped_greedy_sample_batch(None, codes, starts, p, bits, n_steps, 42)

    a, b = single(), batch()   # warm-up, and the results checked once
    for i in range(n_items):
        assert np.array_equal(a[i].view(np.uint32), b[i].view(np.uint32)), f"{name}: item {i}"
        assert np.array_equal(b[i].view(np.uint32), np.asarray(enc[i][0]).view(np.uint32))
    if ONCE:
        print(f"{name}: one pass of each way done")
        return
    single(), batch()
    ts, tb = [], []
    for _ in range(ROUNDS):
        ts.append(lap(single, PASSES) / n_items)
        tb.append(lap(batch, PASSES) / n_items)
    groups = sum(len(s) - 1 for s in starts) / n_items
    print(f"{name}: {n_items} x {D} dims, {groups:.0f} groups/image, {n_steps} x {bits} bits")
    print(f"  single loop  {np.mean(ts):.4f} ms/image  rounds {['%.4f' % v for v in ts]} "
          f"spread {max(ts) - min(ts):.4f}")
    print(f"  batch call   {np.mean(tb):.4f} ms/image  rounds {['%.4f' % v for v in tb]} "
          f"spread {max(tb) - min(tb):.4f}")
    gain = np.mean(ts) - np.mean(tb)
    print(f"  ratio single / batch {np.mean(ts) / np.mean(tb):.2f}, gain {gain:.4f} ms/image "
          f"({'more' if gain > max(ts) - min(ts) else 'no more'} than the single loop's spread)")


compare("C2 x 24", 24, 32 * 48 * 128, 1, 8, 4)
compare("c2cli", 1, 32 * 48 * 128, 30, 14, 12)
