// cwq_imp_screen.h -- the screening bound of the importance coder (DESIGN.md 8,
// "Screening pass"), defined once for k_imp_eval (cwq_importance.hip) and for
// the host, where tests/test_imp_screen_bound.py checks the inequalities
// directly (tests/native/mathcheck.cpp builds this header).
//
// k_imp_eval's drop decisions are taken on a cheap value of each candidate
// row: per dim the float quadratic fmaf(fmaf(A, z', B), z', C) in the
// screening normal z' = z~ / sqrt(2 ln 2) (|z~ - z| <= kScreenEz), summed dim
// by dim.  A row is dropped when its screened sum plus a slack (and, for a
// partial row, the largest value its unvisited dims can add) lies below the
// best lower bound seen.  Survivors are re-scored exactly, so a constant that
// is too small here would change an output only on the rare input whose true
// winner was dropped: the bound has tests of its own.
//
// Compile with -ffp-contract=off; every helper keeps one expression order on
// host and device, so both compute the same bits.
#pragma once
#include <stdint.h>

#include "cwq_math.h"
#include "cwq_screen.h"  // round_up_f32, kScreenZm, kScreenEz, kSqrt2Ln2

namespace cwq {

// Per-dim screening constants and error bound (host-free, in double).  The
// exact term is t = RN(lt - lq), lt = RN(RN(-0.5 RN(yt^2)) - ct),
// yt = RN(RN(x - tl) / ts), lq likewise with (pl, ps, cp), x = RN(pl + RN(ps z)).
// In real arithmetic t(z) = A z^2 + B z + C with a = ps/ts, b = (pl - tl)/ts,
// A = (1 - a^2)/2, B = -a b, C = cp - ct - b^2/2.  Returns false if the dim
// must not be screened.
struct ImpScreenDim {
  float A, B, C, err, mag, umax;
};
CWQ_HD bool imp_screen_dim(float tl, float ts, float pl, float ps, float ct, float cp,
                           ImpScreenDim& o) {
  if (!(ts >= 0x1p-60f && ts <= 0x1p60f && ps >= 0x1p-60f && ps <= 0x1p60f)) return false;
  if (!(tl - tl == 0.0f && pl - pl == 0.0f && ct - ct == 0.0f && cp - cp == 0.0f)) return false;
  const double u = 0x1p-24, r = 1.0001, Zm = kScreenZm, Ez = kScreenEz;
  const double dtl = tl, dts = ts, dpl = pl, dps = ps, dct = ct, dcp = cp;
  // rounding of the exact chain, bounded with |z| <= Zm
  const double m1 = __builtin_fabs(dps) * Zm;
  const double mx = __builtin_fabs(dpl) + m1;
  const double ex = u * (m1 + mx) * r;
  const double mdt = mx + __builtin_fabs(dtl), mdq = mx + __builtin_fabs(dpl);
  const double Myt = mdt / dts * (1.0 + 4.0 * u), Myq = mdq / dps * (1.0 + 4.0 * u);
  const double eyt = ((ex + u * mdt) / dts + u * Myt) * r;
  const double eyq = ((ex + u * mdq) / dps + u * Myq) * r;
  const double lt_mag = 0.5 * Myt * Myt + __builtin_fabs(dct);
  const double lq_mag = 0.5 * Myq * Myq + __builtin_fabs(dcp);
  const double rho = (0.5 * (2.0 * Myt * eyt + eyt * eyt + u * Myt * Myt) + u * lt_mag +
                      0.5 * (2.0 * Myq * eyq + eyq * eyq + u * Myq * Myq) + u * lq_mag +
                      u * (lt_mag + lq_mag)) * r;
  // the real quadratic in z and its float coefficients in z' = z / sqrt(2 ln 2)
  // (the screening Box-Muller's output): A' = 2 ln2 A, B' = sqrt(2 ln 2) B
  const double a = dps / dts, b = (dpl - dtl) / dts;
  const double A = 0.5 * (1.0 - a * a), B = -a * b, C = dcp - dct - 0.5 * b * b;
  const double A1 = A * (kSqrt2Ln2 * kSqrt2Ln2), B1 = B * kSqrt2Ln2;
  const double Zq = Zm / kSqrt2Ln2 * (1.0 + 4.0 * u);  // bound on |z'|
  o.A = (float)A1;
  o.B = (float)B1;
  o.C = (float)C;
  const double dA = __builtin_fabs((double)o.A - A1) + 0x1p-50 * (1.0 + a * a) * 1.4;
  const double dB = __builtin_fabs((double)o.B - B1) + 0x1p-50 * __builtin_fabs(a * b) * 1.2;
  const double dC = __builtin_fabs((double)o.C - C) +
                    0x1p-50 * (__builtin_fabs(dcp) + __builtin_fabs(dct) + b * b);
  const double fA = __builtin_fabs((double)o.A), fB = __builtin_fabs((double)o.B);
  const double fC = __builtin_fabs((double)o.C);
  const double h1 = fA * Zq + fB;  // |A' z' + B'|
  const double horner = dA * Zq * Zq + dB * Zq + dC + Zq * u * h1 * r + u * (h1 * Zq * r + fC);
  // z~ vs z: |t(z) - t(z~)| <= max|t'| Ez + |A| Ez^2
  const double slope = 2.0 * __builtin_fabs(A) * Zm + __builtin_fabs(B);
  const double e = (rho + slope * Ez + __builtin_fabs(A) * Ez * Ez + horner) * (1.0 + 0x1p-20) +
                   0x1p-140;
  o.err = round_up_f32(e);
  o.mag = round_up_f32(lt_mag + lq_mag + e);  // bounds |t| and |t~|
  // largest exact term over |z| <= Zm (pruning): the real quadratic's maximum
  // on the interval (vertex or an end) plus the chain error
  double qmax = A * Zm * Zm + __builtin_fabs(B) * Zm + C;
  if (A < 0.0) {
    double zv = -B / (2.0 * A);
    zv = zv < -Zm ? -Zm : (zv > Zm ? Zm : zv);
    qmax = A * zv * zv + B * zv + C;
  }
  qmax += 0x1p-40 * (__builtin_fabs(A) * Zm * Zm + __builtin_fabs(B) * Zm + __builtin_fabs(C));
  o.umax = round_up_f32(qmax + e);
  return o.err - o.err == 0.0f && o.mag - o.mag == 0.0f && o.A - o.A == 0.0f &&
         o.B - o.B == 0.0f && o.C - o.C == 0.0f && o.umax - o.umax == 0.0f;
}

// One screened term, and the row's running sum: dim by dim, in this order.
CWQ_HD float imp_screen_term(float A, float B, float C, float zq) {
  return __builtin_fmaf(__builtin_fmaf(A, zq, B), zq, C);
}

// The row bound E of a group of d gated-in dims:
// |screened sum - exact Eigen-order sum| <= sum err_j + 2 gamma_d sum mag_j
// (gamma_d = 1.01 d 2^-24 covers both float summations).  +inf from 1.0e3 up:
// such a group is scored exactly.
CWQ_HD float imp_screen_row_bound(const float* derr, const float* dmag, int64_t d) {
  double es = 0.0, ms = 0.0;
  for (int64_t j = 0; j < d; ++j) {
    es += (double)derr[j];
    ms += (double)dmag[j];
  }
  const double gam = 1.01 * (double)d * 0x1p-24;
  const double et = (es + 2.0 * gam * ms) * (1.0 + 0x1p-20) + 0x1p-126;
  return et < 1.0e3 ? round_up_f32(et) : __builtin_inff();
}

// Pruning: dsuf[j] = an upper bound of the sum of dumax[j..d), the most the
// unvisited dims of a row stopped after j dims can add; dsuf[d] = 0.  The
// factor covers the float adds of the prune test.
CWQ_HD void imp_screen_suffix(const float* dumax, int64_t d, float* dsuf) {
  double suf = 0.0;
  dsuf[d] = 0.0f;
  for (int64_t j = d - 1; j >= 0; --j) {
    suf += (double)dumax[j];
    dsuf[j] = round_up_f32(suf * (1.0 + 0x1p-20) + 0x1p-126);  // covers the test's adds
  }
}

// The slack of a row whose screened sum (over the dims visited so far) is s:
// the exact value of a completed row lies within s +- slack; a row stopped
// after j dims has exact value <= (s + slack) + dsuf[j].
CWQ_HD float imp_screen_slack(float E, float s) { return E + __builtin_fabsf(s) * 0x1p-22f; }
CWQ_HD float imp_screen_upper(float s, float slack, float suffix) { return (s + slack) + suffix; }

}  // namespace cwq
