"""Graph replay of one library call (a helper of tests/test_graph_replay_gpu.py).

include/cwq.h: calls are stream-ordered, allocate nothing and do not
synchronise, so a caller may capture them into a graph.  ``replay_check`` holds
one call to that: the call goes through the C ABI on tensors made before the
capture, runs once eagerly on a side stream (module loading, the library's fork
streams), is captured once on that stream and replayed three times.  Before
each replay every output and every workspace is filled with another of
tests/poison.py's byte patterns (0x00, 0xFF, seeded random bytes), so that a
result taken from what the buffers held, from the run before or from a launch
that ran out of order differs from ``want``, which comes from a reference and
never from the eager run.  Every word of every output is compared, as int32.

No environment variable, stream or queue setting is touched; one process, one
capture stream, the library forks where it does anyway.
"""
import os
import re

import numpy as np
import torch

PATTERNS = (0x00, 0xFF, "random")  # tests/poison.py's


def words(x):
    """A tensor or array as a flat numpy int32 view of its bytes."""
    if isinstance(x, torch.Tensor):
        x = x.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy()
    else:
        x = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    if x.size % 4:  # a byte stream: its last word padded with zeros
        x = np.concatenate([x, np.zeros(-x.size % 4, np.uint8)])
    return x.view(np.int32).copy()


def fill(t, pattern, rng):
    """Every byte of tensor t set to the pattern."""
    if t.numel() == 0:
        return
    u8 = t.view(-1).view(torch.uint8)
    if pattern == "random":
        u8.copy_(torch.from_numpy(rng.integers(0, 256, u8.numel(), dtype=np.uint8)))
    else:
        u8.fill_(pattern)


class Steps:
    """What an output of a multi-step encoder holds, for the message: ``idx``
    [nb, n_steps] int32 (one word per block and step), or ``sample`` (the words
    of block g are [off[g], off[g + 1]))."""

    def __init__(self, kind, n_steps, off):
        assert kind in ("idx", "sample")
        self.kind, self.n_steps, self.off = kind, int(n_steps), np.asarray(off, np.int64)

    def block_step(self, at):
        """(block, step or -1) of each word number."""
        if self.kind == "idx":
            return at // self.n_steps, at % self.n_steps
        return np.searchsorted(self.off, at, side="right") - 1, np.full(at.shape, -1)


def classify(got, want, filled, prev, layout=None):
    """The wrong words of one output by what they hold: the fill pattern (the
    store never ran), index 0 (keys zeroed after the scoring; an index output
    only: the sample is not held against the step's row 0), the previous
    step's index (keys not zeroed between steps), the value the run before
    left there (``prev``: that run's output, right or wrong), anything else;
    per step and block parity where ``layout`` says how."""
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    cls = np.full(bad.size, 4)
    cls[got[bad] == prev[bad]] = 3
    if layout is not None and layout.kind == "idx":
        g, s = layout.block_step(bad)
        before = np.where(s > 0, want[np.maximum(bad - 1, 0)], -1)
        cls[(s > 0) & (got[bad] == before)] = 2
        cls[got[bad] == 0] = 1
    cls[got[bad] == filled[bad]] = 0
    names = ("the fill pattern", "index 0" if layout is not None and layout.kind == "idx" else "-",
             "the previous step's index", "the previous replay's value", "something else")
    out = [f"{bad.size} of {want.size} words differ, first at {bad[:8].tolist()}: "
           f"got {got[bad[:4]].tolist()}, want {want[bad[:4]].tolist()}"]
    if layout is None:
        keys = [((), np.ones(bad.size, bool))]
    else:
        g, s = layout.block_step(bad)
        keys = [((f"step {st}" if st >= 0 else "all steps", ("even", "odd")[par] + " blocks"),
                 (s == st) & (g % 2 == par))
                for st in sorted(set(s.tolist())) for par in (0, 1)]
    for key, m in keys:
        if not m.any():
            continue
        counts = ", ".join(f"{int((cls[m] == k).sum())} hold {names[k]}"
                           for k in range(5) if (cls[m] == k).any())
        out.append((" ".join(key) + ": " if key else "") + counts)
    return "; ".join(out)


def _compare(outputs, want, filled, prev, layouts, what):
    torch.cuda.synchronize()
    got = {k: words(t) for k, t in outputs.items()}
    msgs = []
    for k, g in got.items():
        w = want[k]
        assert g.shape == w.shape, f"{what}: output {k}: {g.size} words, the reference has {w.size}"
        m = classify(g, w, filled[k], prev[k], layouts.get(k))
        if m:
            msgs.append(f"{k}: {m}")
    return got, (f"{what}: " + " | ".join(msgs) if msgs else "")


def replay_check(run, outputs, scratch, want, what, layouts=None, replays=3):
    """run(stream): enqueues the call on the torch stream given (nothing else).
    outputs: {name: tensor}, each compared whole; scratch: workspaces, filled
    like the outputs; want: {name: array}, the reference's bytes."""
    assert set(outputs) == set(want) and replays >= len(PATTERNS)
    layouts = layouts or {}
    want = {k: words(v) for k, v in want.items()}
    rng = np.random.Generator(np.random.PCG64(11))
    every = list(outputs.values()) + list(scratch)

    def poison(pattern):
        for t in every:
            fill(t, pattern, rng)
        torch.cuda.synchronize()
        return {k: words(t) for k, t in outputs.items()}

    side = torch.cuda.Stream()
    filled = poison(0xFF)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(side)
    side.synchronize()
    prev, msg = _compare(outputs, want, filled, filled, layouts,
                         f"{what}: eager, before the capture")
    assert not msg, msg

    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        run(side)
    # every replay runs, also after a wrong one, and is held against what the
    # replay before it left: a word that keeps a wrong value from replay to
    # replay is told from one that is wrong anew
    failed = []
    for r in range(replays):
        pattern = PATTERNS[r % len(PATTERNS)]
        filled = poison(pattern)
        graph.replay()
        prev, msg = _compare(outputs, want, filled, prev, layouts,
                             f"{what}: replay {r} on buffers filled with {pattern!r}")
        if msg:
            failed.append(msg)
    assert not failed, "\n".join(failed)


# The calls outside the contract: include/cwq.h documents each as synchronising
# or as not capturable (tests/test_graph_contract.py holds this list to it).
NOT_CAPTURABLE = {
    "cwq_greedy_encode_uniform_var", "cwq_greedy_encode_var", "cwq_greedy_backfit_var",
    "cwq_code_grouped_greedy", "cwq_code_grouped_greedy_begin",
    "cwq_code_grouped_greedy_end", "cwq_code_grouped_greedy_batch",
    "cwq_code_grouped_importance", "cwq_code_grouped_importance_batch",
    "cwq_decode_grouped_greedy_batch", "cwq_decode_grouped_importance_batch",
}


def header_not_capturable(text):
    """The functions whose comment in include/cwq.h says they synchronise or
    cannot be captured.  A comment covers the declarations that follow it up to
    the next comment (a size function and its call share one); size functions
    compute on the host and touch no stream."""
    marks = re.compile(r"NOT graph-capturable|SYNCHRONISES|[Ss]ynchronises the stream|"
                       r"cannot be captured")
    out = set()
    for m in re.finditer(r"/\*(.*?)\*/(.*?)(?=/\*|\Z)", text, re.S):
        if marks.search(" ".join(m.group(1).replace("*", " ").split())):
            out |= {n for n in re.findall(r"\b(cwq_\w+)\(", m.group(2))
                    if not n.endswith("_size")}
    return out


def header_text():
    here = os.path.dirname(os.path.abspath(__file__))
    return open(os.path.join(here, "..", "include", "cwq.h")).read()
