"""The deferral regions of a cwq_greedy_encode_uniform workspace
(csrc/cwq_workspace.h defer_ws), restated for the tests: tests/test_defer_plan.py
holds this against the header, compiled for the host, and
tests/test_prune_defer_gpu.py reads the regions back after a call with it."""
SLOTS = 4   # kDeferSlots
Q = 2       # kDeferQ


def up(v):
    return (v + 255) // 256 * 256


def applies(nb, d):
    return 0 < nb < (1 << 31) and d % 8 == 0 and 8 <= d <= 64


def regions(enc_total, nb, d):
    """{name: (offset, bytes)} and the total, behind an encoder layout of
    enc_total bytes."""
    n = nb if applies(nb, d) else 0
    out, o = {}, up(enc_total)
    for name, nbytes in (("surv", n * SLOTS * 4), ("count", n * 4), ("dlist", n * 4),
                         ("dcount", 4 if n else 0)):
        out[name] = (o, nbytes)
        o = up(o + nbytes)
    return out, o


def slot(g, q):
    return g * SLOTS + q


def count_word(c, q):
    return c if c <= q else 0
