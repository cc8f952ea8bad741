// cwq_screen.h -- the screening bound of the pruned encoders,
// defined once for every path that prunes (k_encode_prune, k_encode_prune_csr
// with k_csr_prep, k_small_prep + k_small_screen, k_small_prep1 + k_small_one)
// and for the host, where tests/test_screen_bound.py checks the inequalities
// directly.
//
// The drop decisions of those kernels are taken on cheap approximations: z~
// from the hardware transcendentals (|z~ - z| <= kScreenEz for every Philox
// output), and per dim
//     a_j = RN(sA_j z' + sB_j),  z' = z~ / sqrt(2 ln 2),
//     sA_j ~ ss_j K_j sqrt(2 ln 2),  sB_j ~ (best + loc_s - mu)_j K_j,
// K_j = sqrt(phi (1 - 2^-24) / 2) / sigma_j, with the guarantee
//     0.5 y_j^2 (1 - 2^-24)  >=  a_j^2 - C_j
// for the exact standardised value y_j (C_j a tiny per-dim constant).  With s
// the float sum of -a_j^2 over a row's dims, the row's exact Eigen-order value
// E lies in
//     c2 s + As - Pq sqrt(-s)  <=  E  <=  c1 s + B
// (screen_row_lower / screen_row_upper); a partial row takes B over the dims
// visited so far.  Survivors are re-evaluated exactly, so the screening
// arithmetic never reaches the output -- and a wrong constant here would not
// fail an output test either, which is why the bound has tests of its own.
//
// Compile with -ffp-contract=off; every helper keeps one expression order on
// host and device, so both compute the same bits.
#pragma once
#include <stdint.h>

#include "cwq_math.h"

#if defined(__HIPCC__)
#define CWQ_HD_MEMBER __host__ __device__ __forceinline__
#else
#define CWQ_HD_MEMBER inline
#endif

namespace cwq {

// The screening radius is carried without its constant factor: q~ =
// sqrt(-log2 u1) = r~ / sqrt(2 ln 2), so the screening normals arrive as
// z' = z~ / sqrt(2 ln 2) and sA folds the factor in.
constexpr double kSqrt2Ln2 = 1.1774100225154747;  // sqrt(2 ln 2)

// Error constants of the screening Box-Muller.  Measured maxima over all 2^23
// inputs (tools/screen_err.py, re-checked by tests/test_gpu.py):
// |sqrt(2 ln 2) q~ - r| <= 5.82e-7, |sin~ - sin|, |cos~ - cos| <= 2.99e-7
constexpr double kScreenEr = 1.0e-6;
constexpr double kScreenEs = 6.0e-7;
constexpr double kScreenRmax = 5.68;  // r <= sqrt(-2 ln 1e-7) = 5.6777
// |sqrt(2 ln 2) RN(s~ q~) - RN(s r)| <= (1 + Es) Er + Rmax Es + 2^-23 (Rmax + Er)
constexpr double kScreenEz =
    (1.0 + kScreenEs) * kScreenEr + kScreenRmax * kScreenEs + 0x1p-23 * (kScreenRmax + kScreenEr);
constexpr double kScreenZm = 5.7;     // bound on |z| and |z~|

// k_encode_prune's fixed factors (D <= 64); the other paths scale theirs with d
constexpr float kScreenC1 = 1.0f - 0x1p-14f;
constexpr float kScreenC2 = 1.0f + 0x1p-13f;
// split of the additive error: (x-A)^2 >= (1-e)x^2 - (1/e-1)A^2
constexpr double kScreenEps = 0x1p-15;
constexpr double kScreenPhi = (1.0 - kScreenEps) * (1.0 - 0x1p-21);
constexpr double kScreenKappa = 0.7070958018530696;  // sqrt(phi (1 - 2^-24) / 2), rounded down

// smallest float >= b (+inf for non-finite b: such a bound never drops anything)
CWQ_HD float round_up_f32(double b) {
  if (!(b == b) || b > 3.0e38 || b < -3.0e38) return __builtin_inff();
  float f = (float)b;
  if ((double)f < b) {
    const uint32_t u = f2u(f);
    f = (f >= 0.0f) ? u2f(f == 0.0f ? 1u : u + 1u) : u2f(u - 1u);
  }
  return f;
}
CWQ_HD float round_dn_f32(double b) { return -round_up_f32(-b); }

// a denominator div_rn_markstein takes (cwq_device.h)
CWQ_HD bool markstein_ok_den(float b) { return b >= 0x1p-60f && b <= 0x1p60f; }

// ---------------------------------------------------------------------------
// Per-dim constants.
// ---------------------------------------------------------------------------
struct ScreenDim {
  float sa, sb;     // a = RN(sa z' + sb), z' = screening z / sqrt(2 ln 2)
  float A, C;       // additive error (a units) and C_j of the bound
  double M;         // M_j = -c_j: the largest value the dim's log-density takes
  bool ok;          // the range gate: outside it the block is scored exactly
};

// ls, ss: the shard's loc_s, scale_s; mu, sg: the target; c: its normaliser
// kHalfLog2Pi + log(sg); bb: best (ignored at step 0, where best == +0)
template <bool STEP0>
CWQ_HD ScreenDim screen_dim(float ls, float ss, float mu, float sg, float c, float bb) {
  ScreenDim o;
  const double ssa = __builtin_fabs((double)ss), lsa = __builtin_fabs((double)ls);
  const double mua = __builtin_fabs((double)mu);
  const double bba = STEP0 ? 0.0 : __builtin_fabs((double)bb);
  const double zs = kScreenZm * ssa;
  const double mag = bba + lsa + zs + mua;
  // rounding of the exact chain RN(RN(RN(bb +) RN(ls + RN(ss z))) - mu)
  const double rho = 0x1p-24 * 1.0001 * (zs + (lsa + zs) + (STEP0 ? 0.0 : bba + lsa + zs) + mag);
  const double offd = (STEP0 ? 0.0 : (double)bb) + (double)ls - (double)mu;
  const double sig = (double)sg;
  const double kq = kScreenKappa / sig;
  o.sa = (float)((double)ss * kq * kSqrt2Ln2);  // z~ arrives / sqrt(2 ln 2)
  o.sb = (float)(offd * kq);
  const double a0 = (kq * (rho + ssa * kScreenEz) +
                     kq * 0x1p-24 * 1.0001 * (zs + __builtin_fabs(offd))) * (1.0 + 0x1p-20) +
                    0x1p-140;
  o.A = round_up_f32(a0 * 1.0001);
  o.C = round_up_f32((1.0 / kScreenEps - 1.0) * a0 * a0 / kScreenPhi * (1.0 + 0x1p-20));
  o.M = -(double)c;
  o.ok = markstein_ok_den(sg) && mag <= 0x1p100 && mag / sig <= 0x1p50 && o.C <= 0x1p60f &&
         o.sa - o.sa == 0.0f && o.sb - o.sb == 0.0f && c - c == 0.0f;
  return o;
}

// ---------------------------------------------------------------------------
// Per-block sums and constants.
// ---------------------------------------------------------------------------
struct ScreenSums {
  double sm = 0.0, sa = 0.0, sk = 0.0;  // sum M, sum |M|, sum (|M| + M)
  double s2 = 0.0, cs = 0.0, mx = 0.0;  // sum A^2, sum C, max A
  int ok = 1;                           // every dim inside the gate
  CWQ_HD_MEMBER void add(const ScreenDim& o) {
    sm += o.M;
    sa += __builtin_fabs(o.M);
    sk += __builtin_fabs(o.M) + o.M;
    s2 += (double)o.A * (double)o.A;
    cs += (double)o.C;
    mx = (double)o.A > mx ? (double)o.A : mx;
    ok &= o.ok ? 1 : 0;
  }
};

// As: the additive constant of a completed row's lower bound, given the slack
// sl of the float sums
CWQ_HD float screen_as(double sum_m, double sl, double sum_a2) {
  return round_dn_f32(sum_m - sl - 1.01 * sum_a2 * (1.0 + 0x1p-11));
}
// Pq: the factor of sqrt(-s) in that bound (Cauchy-Schwarz over the d dims'
// additive errors); the device's v_sqrt_f32 of -s is within ~1 ulp, inside
// the 0.4% slack taken here
template <class I>
CWQ_HD float screen_pq(double max_a, I d) {
  return round_up_f32(2.01 * max_a * __builtin_sqrt((double)(d > 0 ? d : 1)) * (1.0 + 0x1p-11));
}

struct ScreenBlock {
  double gam, sl;   // gamma at the block's summation depth; slack of the sums
  float c1, c2;     // factors of s in the upper / lower bound
  float as, pq;     // lower bound: c2 s + as - pq sqrt(-s)
  float bf;         // B of a full row: upper bound c1 s + bf
  bool finite;      // as and pq are finite (callers that use bf test it too)
};

// Float summation error of depth h: gamma_h = 1.01 (h + 1) 2^-24 bounds
// |fl(sum) - sum| / sum|x| for any summation tree in which every term passes
// through at most h roundings.  Two sums of d terms enter the bound: the
// screening sum s, whose depth h_s the caller passes (sequential over the row:
// h_s = d; k_encode_prune_csr's cooperative rows: 4 in-lane + 4 butterfly +
// one per 16-unit chunk, <= 16 + d/64), and the exact Eigen-order row value (8
// strided accumulators, predux, tail: <= d/8 + 8).  gamma is taken at the
// larger depth.  The additive margin 2^-20 covers the float rounding of B and
// of the tests' fma (u |B|) and the double roundings of the sums; u |s| is
// covered by the 2^-22 / 2^-14 terms of c1 / c2.
template <class I>
CWQ_HD ScreenBlock screen_block_consts(const ScreenSums& u, I d, double h_s) {
  ScreenBlock o;
  const double h_e = (double)d / 8.0 + 8.0;
  const double gam = 1.01 * ((h_s > h_e ? h_s : h_e) + 1.0) * 0x1p-24;
  const double g3 = 3.0 * gam;
  o.gam = gam;
  o.sl = (g3 + 0x1p-20) * (__builtin_fabs(u.sm) + u.sa + u.sk) + 0x1p-126;
  o.bf = round_up_f32(u.sm + u.cs * (1.0 + 0x1p-20) + o.sl);
  o.c1 = round_dn_f32(1.0 - g3 - 0x1p-22);
  o.c2 = round_up_f32(1.0 + g3 + 0x1p-14);
  o.as = screen_as(u.sm, o.sl, u.s2);
  o.pq = screen_pq(u.mx, d);
  o.finite = o.as - o.as == 0.0f && o.pq - o.pq == 0.0f;
  return o;
}

// ---------------------------------------------------------------------------
// A row's bracket from its screened sum s = fl(sum of -a_j^2): the exact
// Eigen-order value E of every completion of the visited dims is at most
// upper(s, c1, B); a completed row has E >= lower(s, c2, As, Pq).
// ---------------------------------------------------------------------------
CWQ_HD float screen_row_upper(float s, float c1, float B) { return __builtin_fmaf(s, c1, B); }
CWQ_HD float screen_row_lower(float s, float c2, float As, float Pq) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float r = __builtin_amdgcn_sqrtf(-s);
#else
  const float r = __builtin_sqrtf(-s);
#endif
  return __builtin_fmaf(s, c2, As) - Pq * r;
}

}  // namespace cwq
