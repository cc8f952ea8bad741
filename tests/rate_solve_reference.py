"""ratetable.choose_bits_total restated in NumPy (its 60-step loop over
rate_reference.choose_bits), and the crafted tables, targets and ranges on which
tests/test_rate_solve.py (CPU: csrc/cwq_rate_solve.h) and
tests/test_rate_total_gpu.py (cwq_choose_bits_total) hold the device solver to
it.  A helper; not a test, nothing in the product imports it.
"""
import numpy as np

import rate_reference as R

F32 = np.float32
FLT_MAX = np.finfo(F32).max
NB = (1, 65, 257, 300)
BITS = (0, 5, 8, 16, 30)


def total_at(value, lam, lo, hi):
    return int(R.choose_bits(value, lam, lo, hi).sum(dtype=np.int64))


def choose_bits_total(value, total_bits, lo=0, hi=None, strict=False):
    """(bits int32 [nb], lam float, total) of ratetable.choose_bits_total.
    ``strict``: the wrong walk, ``<`` in place of ``<=`` (to show that a case
    tells the two apart)."""
    v = np.asarray(value, F32)
    hi = v.shape[1] - 1 if hi is None else min(int(hi), v.shape[1] - 1)
    T = int(total_bits)
    assert 0 <= lo <= hi and v.shape[0] * lo <= T
    fits = (lambda t: t < T) if strict else (lambda t: t <= T)
    lam_hi = 0.0
    if not total_at(v, 0.0, lo, hi) <= T:
        span = v[:, lo:hi + 1].astype(np.float64) - v[:, lo:lo + 1].astype(np.float64)
        lam_lo, lam_hi = 0.0, float(span.max())
        for _ in range(60):
            mid = 0.5 * (lam_lo + lam_hi)
            if fits(total_at(v, mid, lo, hi)):
                lam_hi = mid
            else:
                lam_lo = mid
    bits = R.choose_bits(v, lam_hi, lo, hi)
    return bits, lam_hi, int(bits.sum(dtype=np.int64))


def lam_bits(lam):
    """A price as its float64 bit pattern."""
    return int(np.float64(lam).view(np.uint64))


def crafted_table(nb, B, clamp=False, seed=0):
    """Rows of a negative base plus a concave-ish cumulative gain plus noise.
    ``clamp``: row 0 is -FLT_MAX throughout and, from three blocks on, row 2
    ends at +FLT_MAX (lam_hi is then about 3.4e38)."""
    rng = np.random.Generator(np.random.PCG64(1000 * nb + 10 * B + seed))
    base = -np.abs(rng.standard_normal((nb, 1))) * 30
    gains = np.cumsum(rng.exponential(1.0, (nb, B + 1)) * (0.8 ** np.arange(B + 1)) * 3, axis=1)
    v = (base + gains + 0.3 * rng.standard_normal((nb, B + 1))).astype(F32)
    if clamp:
        v[0, :] = -FLT_MAX
        if nb > 2:
            v[2, B] = FLT_MAX
    return np.ascontiguousarray(v)


def ranges(B):
    """(lo, hi): the whole table, an inner range, and lo = hi."""
    out = [(0, B)]
    if B >= 2:
        out.append((1, B - 1))
    out.append((B // 2, B // 2))
    return out


def targets(value, lo, hi):
    """nb lo, nb lo + 1, free // 3, free // 2, free - 1, free, free + 5 with
    free = total(0); those below nb lo (which the call refuses) left out."""
    nb = value.shape[0]
    free = total_at(value, 0.0, lo, hi)
    want = [nb * lo, nb * lo + 1, free // 3, free // 2, free - 1, free, free + 5]
    return sorted({t for t in want if t >= nb * lo})


def cases(nbs=NB, bits=BITS):
    """(table, lo, hi, target) over the crafted tables."""
    for nb in nbs:
        for B in bits:
            for clamp in (False, True):
                if clamp and B not in (5, 16):
                    continue
                v = crafted_table(nb, B, clamp)
                for lo, hi in ranges(B):
                    for T in targets(v, lo, hi):
                        yield v, lo, hi, T
