"""The screening bound itself (csrc/cwq_screen.h), on the host.

The GPU tests compare outputs, and survivors of the screen are re-scored
exactly, so a wrong bound constant would rarely change an output.  These two
tests check the inequalities the pruning proof rests on, on the very functions
the kernels compile (tests/native/mathcheck.cpp builds the header for the
host), and assert zero violations.
"""
import ctypes

import numpy as np

F32 = np.float32


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _consts(mc):
    mc.mc_screen_ez.restype = ctypes.c_double
    mc.mc_screen_sqrt2ln2.restype = ctypes.c_double
    return mc.mc_screen_ez(), mc.mc_screen_sqrt2ln2()


def _pm(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)


def _y(z, ls, ss, mu, sg, bb, step0):
    """The exact float chain RN(RN(RN(RN(ss z) + ls) [+ bb]) - mu) / sg)."""
    t = ss * z
    t = ls + t
    tv = np.where(step0, t, bb + t)
    return (tv - mu) / sg


def _zprime(rng, z, ez, k, extremes):
    """Screening normal z' = float((z + delta) / sqrt(2 ln 2)), |delta| <= Ez - 3e-7
    (3e-7: z' 's own float rounding, |z'| < 4.9); `extremes`: delta at +-max."""
    dmax = ez - 3.0e-7
    delta = rng.uniform(-dmax, dmax, z.shape)
    delta = np.where(extremes == 1, dmax, np.where(extremes == 2, -dmax, delta))
    return ((z.astype(np.float64) + delta) / k).astype(F32)


def test_per_dim_inequality(mathcheck):
    """0.5 y^2 (1 - 2^-24) >= a^2 - C for every gated-in draw."""
    mc = mathcheck
    ez, k = _consts(mc)
    rng = np.random.default_rng(20240601)
    n = 2_400_000
    q = n // 4
    U = rng.uniform

    def p2(lo, hi, m):
        return np.exp2(U(lo, hi, m))

    fam = {
        "moderate": (_pm(rng, q) * p2(-3, 3, q), p2(-6, 1, q), _pm(rng, q) * p2(-3, 3, q),
                     p2(-8, 2, q), _pm(rng, q) * p2(-3, 3, q)),
        "wide": (_pm(rng, q) * p2(-30, 30, q), p2(-40, 30, q), _pm(rng, q) * p2(-30, 30, q),
                 p2(-59, 59, q), _pm(rng, q) * p2(-30, 30, q)),
        "c2": (U(-.5, .5, q), U(.05, 1.05, q), U(-2, 2, q), U(.01, .31, q), U(-1, 1, q)),
        "prior": (np.zeros(q), np.ones(q), U(-3, 3, q), np.exp2(-U(0, 10, q)), np.zeros(q)),
    }
    ls, ss, mu, sg, bb = (np.concatenate([fam[f][i] for f in fam]).astype(F32) for i in range(5))
    step0 = (np.arange(n) % 2 == 0)
    bb = np.where(step0, F32(0), bb).astype(F32)
    c = np.zeros(n, F32)
    out = np.empty((n, 5), F32)
    s0 = step0.astype(np.uint8)
    mc.mc_screen_dim_many(ctypes.c_int64(n), _p(s0), _p(ls), _p(ss), _p(mu), _p(sg), _p(c), _p(bb),
                          _p(out))
    # the single-dim entry point agrees with the batched one
    one = np.empty(5, F32)
    for i in (0, 1, q, q + 1, 2 * q + 5, 3 * q + 2):
        mc.mc_screen_dim(int(s0[i]), *(ctypes.c_float(float(v[i])) for v in (ls, ss, mu, sg, c, bb)),
                         _p(one))
        assert one.tobytes() == out[i].tobytes()
    ok = out[:, 4] == 1.0
    gated = 1.0 - ok.mean()
    print(f"gated out: {gated:.4f} of {n} draws")
    assert gated <= 0.10
    z = U(-5.68, 5.68, n).astype(F32)
    r8 = rng.integers(0, 8, n)
    extremes = np.where(r8 < 2, 1 + r8, 0)  # a quarter of the draws at +-max
    zp = _zprime(rng, z, ez, k, extremes)
    sa, sb = np.ascontiguousarray(out[:, 0]), np.ascontiguousarray(out[:, 1])
    a = np.empty(n, F32)
    mc.mc_fmaf_many(ctypes.c_int64(n), _p(sa), _p(zp), _p(sb), _p(a))  # a = fmaf(sA, z', sB)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        y = _y(z, ls, ss, mu, sg, bb, step0)
        lhs = 0.5 * y.astype(np.float64) ** 2 * (1.0 - 2.0 ** -24)
        rhs = a.astype(np.float64) ** 2 - out[:, 3].astype(np.float64)
        bad = ok & ~(lhs >= rhs)
        pos = ok & (rhs > 0)
        print(f"checked {int(ok.sum())}, violations {int(bad.sum())}, "
              f"min lhs/rhs {np.min(lhs[pos] / rhs[pos]):.9f}")
    assert int(bad.sum()) == 0


def test_row_bracket(mathcheck):
    """screen_row_lower <= E <= screen_row_upper for completed rows."""
    mc = mathcheck
    mc.mc_screen_row_bounds.restype = ctypes.c_int
    ez, k = _consts(mc)
    rng = np.random.default_rng(20240602)
    U = rng.uniform
    rows, reps = 64, 40
    nblocks = ngated = nrows = bad_u = bad_l = 0
    min_up = min_lo = np.inf
    for d in (1, 2, 3, 5, 8, 9, 17, 31, 64, 65, 300, 1025):
        for family in range(3):
            for step0 in (True, False):
                for _ in range(reps):
                    if family == 0:    # standard prior
                        ls, ss = np.zeros(d), np.ones(d)
                        mu, sg = U(-2, 2, d), np.exp2(-U(0, 6, d))
                    elif family == 1:  # C2-like
                        ls, ss = U(-.5, .5, d), U(.05, 1.05, d)
                        mu, sg = U(-2, 2, d), U(.01, .51, d)
                    else:              # large
                        ls, ss = U(-50, 50, d), np.exp2(U(-10, 10, d))
                        mu, sg = U(-50, 50, d), np.exp2(U(-15, 15, d))
                    ls, ss, mu, sg = (v.astype(F32) for v in (ls, ss, mu, sg))
                    bb = (np.zeros(d) if step0 else U(-1.5, 1.5, d)).astype(F32)
                    c = F32(0.9189385) + np.log(sg)  # kHalfLog2Pi + logf(sigma)
                    assert c.dtype == F32
                    u1 = np.maximum(U(0, 1, (rows, d)), 1e-7)
                    z = (np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * U(0, 1, (rows, d)))).astype(F32)
                    z[::8] *= F32(0.05)  # near the mode: the lower bound's tight end
                    r8 = rng.integers(0, 8, (rows, d))
                    zp = _zprime(rng, z, ez, k, np.where(r8 < 2, 1 + r8, 0))
                    y = _y(z, ls, ss, mu, sg, bb, step0)
                    lp = F32(-0.5) * (y * y) - c
                    assert lp.dtype == F32 and zp.dtype == F32
                    lp = np.ascontiguousarray(lp)
                    zp = np.ascontiguousarray(zp)
                    out = np.empty((rows, 3), F32)
                    got = mc.mc_screen_row_bounds(
                        ctypes.c_int(int(step0)), ctypes.c_int64(d), _p(ls), _p(ss), _p(mu), _p(sg),
                        _p(c), _p(bb), ctypes.c_int64(rows), _p(zp), _p(lp), _p(out))
                    if not got:
                        ngated += 1
                        continue
                    nblocks += 1
                    nrows += rows
                    lo, e, up = out[:, 0], out[:, 1], out[:, 2]
                    bad_u += int((~(up >= e)).sum())
                    bad_l += int((~(lo <= e)).sum())
                    min_up = min(min_up, float(np.min(up.astype(np.float64) - e)))
                    min_lo = min(min_lo, float(np.min(e.astype(np.float64) - lo)))
    print(f"blocks {nblocks} gated {ngated} rows {nrows} upper violations {bad_u} "
          f"lower violations {bad_l} min(up - E) {min_up:.3g} min(E - lo) {min_lo:.3g}")
    assert ngated == 0
    assert bad_u == 0 and bad_l == 0
