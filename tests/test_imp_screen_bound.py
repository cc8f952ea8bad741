"""The importance coder's screening bound (csrc/cwq_imp_screen.h, DESIGN.md 8
"Screening pass"), on the host.

k_imp_eval drops candidate rows on a cheap value: per dim the float quadratic
fmaf(fmaf(A, z', B), z', C) in the screening normal z', summed dim by dim,
with a hand-derived error bound per dim (err, mag, umax) and per row (E, the
slack E + |s| 2^-22, the suffix sums dsuf[]).  Survivors are re-scored exactly,
so a constant that is too small changes an output only where the dropped row
was the winner, which the GPU parity tests would almost never see.  These
tests check the inequalities the drop decisions rest on, on the very functions
the kernel compiles (tests/native/mathcheck.cpp builds the header for the
host), in float64 comparisons of float32 quantities, and assert zero
violations.

The exact term is a numpy float32 restatement of the oracle's chain
(cwq_oracle.c, cwqo_importance_encode_block); test_restatement_is_the_oracles
pins it to the oracle bit for bit on 1-dim groups first.
"""
import ctypes

import numpy as np

from test_screen_bound import _consts, _p, _pm, _zprime

F32 = np.float32
HALF_LOG_2PI = F32(0.5 * np.log(2.0 * np.pi))
ROW_DIMS = (1, 2, 4, 5, 8, 9, 17, 64, 65, 255, 256)
ORDINARY = ("standard", "nonstd_normal", "nonstd_wide", "near_2^-12", "near_2^-24")
FAMILIES = ORDINARY + ("wide",)


def lognorm(oracle, scale):
    """cwqo_log_normalization: float(0.5 log 2 pi) + logf(scale)."""
    return (HALF_LOG_2PI + oracle.logf_table(scale)).astype(F32)


def exact_term(z, tl, ts, pl, ps, ct, cp):
    """t = lt - lq of one dim, every operation rounded to float32 as the oracle
    rounds it: x = pl + ps z, y = (x - loc) / scale, log_prob = -0.5 (y y) - c."""
    assert all(a.dtype == F32 for a in (z, tl, ts, pl, ps, ct, cp))
    x = ps * z
    x = pl + x
    yt = (x - tl) / ts
    lt = F32(-0.5) * (yt * yt) - ct
    yq = (x - pl) / ps
    lq = F32(-0.5) * (yq * yq) - cp
    t = lt - lq
    assert t.dtype == F32
    return t


def family(rng, name, n):
    """(tl, ts, pl, ps) float32 [n] of one input family."""
    U = rng.uniform
    if name == "standard":            # informative targets against N(0, 1)
        pl, ps = np.zeros(n), np.ones(n)
        tl, ts = 0.7 * rng.standard_normal(n), U(0.3, 0.95, n)
    elif name in ("nonstd_normal", "nonstd_wide"):
        pl, ps = 0.1 * rng.standard_normal(n), U(0.8, 1.25, n)
        tl = 0.7 * rng.standard_normal(n)
        ts = U(0.3, 0.95, n) if name == "nonstd_normal" else U(1.0, 3.0, n)
    elif name.startswith("near_"):    # target ~ proposal: A, B, C cancel to near 0
        eps = 2.0 ** -12 if name == "near_2^-12" else 2.0 ** -24
        pl, ps = 0.1 * rng.standard_normal(n), U(0.8, 1.25, n)
        ts = ps * (1.0 + eps * U(-1, 1, n))
        tl = pl + ps * eps * rng.standard_normal(n)
    else:                             # scales 2^+-59, locs up to 2^30
        assert name == "wide"
        ps = np.exp2(U(-59, 59, n))
        ts = np.clip(ps * np.exp2(U(-3, 3, n)), 2.0 ** -59, 2.0 ** 59)
        pl = _pm(rng, n) * np.minimum(np.exp2(U(-30, 30, n)), ps * np.exp2(U(-4, 8, n)))
        tl = pl + _pm(rng, n) * ps * np.exp2(U(-6, 3, n))
    return tuple(np.ascontiguousarray(v, dtype=F32) for v in (tl, ts, pl, ps))


def screen_dims(mc, tl, ts, pl, ps, ct, cp):
    """(A, B, C, err, mag, umax, gated in) [n, 7] from the header."""
    out = np.empty((tl.size, 7), F32)
    mc.mc_imp_screen_dim_many(ctypes.c_int64(tl.size), _p(tl), _p(ts), _p(pl), _p(ps), _p(ct),
                              _p(cp), _p(out))
    return out


def test_restatement_is_the_oracles(oracle):
    """exact_term is, bit for bit, the score oracle.importance_scores gives the
    rows of 1-dim groups (the Eigen-order sum of one term is the term), with
    each row's z from importance_decode_block under the standard proposal."""
    rng = np.random.default_rng(20241001)
    rows = np.array([0, 1, 2, 3, 4, 5, 6, 7, 100, 1023, 1024, 4097, 65536, 10 ** 6 + 3], np.int64)
    checked = 0
    for name in FAMILIES:
        tl, ts, pl, ps = family(rng, name, 24)
        ct, cp = lognorm(oracle, ts), lognorm(oracle, ps)
        for i in range(tl.size):
            seed = int(rng.integers(-2 ** 31, 2 ** 31))
            sl = slice(i, i + 1)
            want = oracle.importance_scores(tl[sl], ts[sl], pl[sl], ps[sl], seed, rows)
            z = np.array([oracle.importance_decode_block(int(r), [0.0], [1.0], seed)[0]
                          for r in rows], F32)
            with np.errstate(over="ignore", invalid="ignore"):
                got = exact_term(z, *(np.repeat(a[sl], rows.size) for a in (tl, ts, pl, ps, ct, cp)))
            # t + 0.0f: the sum of one term turns -0 into +0
            assert (got + F32(0)).tobytes() == want.tobytes(), (name, i)
            checked += rows.size
    print(f"restatement: {checked} terms bit-equal to the oracle")


def test_per_dim_inequalities(mathcheck, oracle):
    """For every gated-in draw: |screened - t| <= err, |t| and |screened| <=
    mag, t <= umax."""
    mc = mathcheck
    ez, k = _consts(mc)
    rng = np.random.default_rng(20241002)
    q = 400_000
    for name in FAMILIES:
        tl, ts, pl, ps = family(rng, name, q)
        ct, cp = lognorm(oracle, ts), lognorm(oracle, ps)
        out = screen_dims(mc, tl, ts, pl, ps, ct, cp)
        ok = out[:, 6] == 1.0
        gated = 1.0 - ok.mean()
        if name in ORDINARY:
            assert gated == 0.0, (name, gated)
        else:
            assert gated <= 0.10, (name, gated)
        z = rng.uniform(-5.68, 5.68, q).astype(F32)
        r8 = rng.integers(0, 8, q)
        zp = _zprime(rng, z, ez, k, np.where(r8 < 2, 1 + r8, 0))  # a quarter at +-max
        A, B, C = (np.ascontiguousarray(out[:, i]) for i in range(3))
        scr = np.empty(q, F32)
        mc.mc_imp_screen_term_many(ctypes.c_int64(q), _p(A), _p(B), _p(C), _p(zp), _p(scr))
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            t = exact_term(z, tl, ts, pl, ps, ct, cp).astype(np.float64)
            s = scr.astype(np.float64)
            err, mag, umax = (out[:, i].astype(np.float64) for i in (3, 4, 5))
            assert np.isfinite(t[ok]).all() and np.isfinite(s[ok]).all(), name
            bad_err = ok & ~(np.abs(s - t) <= err)
            bad_mag = ok & ~((np.abs(t) <= mag) & (np.abs(s) <= mag))
            bad_max = ok & ~(t <= umax)
            r_err = float(np.max(np.abs(s - t)[ok] / err[ok]))
            r_mag = float(np.max(np.maximum(np.abs(t), np.abs(s))[ok] / mag[ok]))
            m_max = float(np.min(((umax - t) / err)[ok]))
        print(f"{name}: checked {int(ok.sum())}, gated out {gated:.4f}, violations "
              f"{int(bad_err.sum())}/{int(bad_mag.sum())}/{int(bad_max.sum())}, "
              f"max |scr - t| / err {r_err:.4f}, max(|t|, |scr|) / mag {r_mag:.4f}, "
              f"min (umax - t) / err {m_max:.4f}")
        assert int(bad_err.sum()) == 0 and int(bad_mag.sum()) == 0 and int(bad_max.sum()) == 0, name


def test_row_bound_and_prune_test(mathcheck, oracle):
    """Completed rows: |s - exact| <= E + |s| 2^-22, s summed in the kernel's
    order, exact = the Eigen-order sum of the exact terms.  Partial rows: at
    every prefix length j the pruned loop can stop at (the Philox-block
    boundaries for each row alignment 0..3), exact <= (s_j + slack_j) + dsuf[j]
    in the kernel's float order."""
    mc = mathcheck
    mc.mc_imp_screen_row_bounds.restype = ctypes.c_int
    ez, k = _consts(mc)
    rng = np.random.default_rng(20241003)
    rows, reps = 32, 12
    for name in FAMILIES:
        ngroups = ngated = nrows = bad_row = bad_pre = 0
        r_row, m_pre = 0.0, np.inf
        for d in ROW_DIMS:
            for _ in range(reps):
                tl, ts, pl, ps = family(rng, name, d)
                ct, cp = lognorm(oracle, ts), lognorm(oracle, ps)
                u1 = np.maximum(rng.uniform(0, 1, (rows, d)), 1e-7)
                z = (np.sqrt(-2 * np.log(u1)) *
                     np.sin(2 * np.pi * rng.uniform(0, 1, (rows, d)))).astype(F32)
                z[::8] *= F32(0.05)
                z[1::8] = np.clip(z[1::8] * F32(3), -5.68, 5.68)  # the tails, where umax binds
                r8 = rng.integers(0, 8, (rows, d))
                zp = np.ascontiguousarray(_zprime(rng, z, ez, k, np.where(r8 < 2, 1 + r8, 0)))
                with np.errstate(over="ignore", invalid="ignore"):
                    tx = np.ascontiguousarray(exact_term(z, tl, ts, pl, ps, ct, cp))
                out = np.empty((rows, 4), F32)
                pre = np.empty((rows, 4), np.float64)
                dsuf = np.empty(d + 1, F32)
                got = mc.mc_imp_screen_row_bounds(
                    ctypes.c_int64(d), _p(tl), _p(ts), _p(pl), _p(ps), _p(ct), _p(cp),
                    ctypes.c_int64(rows), _p(zp), _p(tx), _p(out), _p(pre), _p(dsuf))
                ngroups += 1
                if not got:
                    ngated += 1
                    continue
                nrows += rows
                s, slack, exact = (out[:, i].astype(np.float64) for i in range(3))
                # the shim's Eigen-order sum is the oracle's
                want = np.array([oracle.eigen_rowsum(tx[r]) for r in range(rows)], F32)
                assert want.tobytes() == out[:, 2].tobytes()
                assert dsuf[d] == 0.0
                bad_row += int((~(np.abs(s - exact) <= slack)).sum())
                r_row = max(r_row, float(np.max(np.abs(s - exact) / slack)))
                # stops exist for alignment a iff 4 - a < d (a = 0: 4 < d)
                for a in range(4):
                    first = 4 - a
                    col = pre[:, a]
                    if first < d:
                        assert np.isfinite(col).all()
                        bad_pre += int((~(col >= 0.0)).sum())
                        m_pre = min(m_pre, float(np.min(col / slack)))
                    else:
                        assert np.isinf(col).all()
        print(f"{name}: groups {ngroups} gated out {ngated} rows {nrows} row violations "
              f"{bad_row} prefix violations {bad_pre}, max |s - exact| / slack {r_row:.4f}, "
              f"min prefix margin / slack {m_pre:.3f}")
        if name in ORDINARY:
            assert ngated == 0, name
        else:
            assert ngated <= 0.10 * ngroups, name
        assert bad_row == 0 and bad_pre == 0, name
