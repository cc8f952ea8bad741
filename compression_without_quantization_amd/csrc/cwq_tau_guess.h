// cwq_tau_guess.h -- a starting threshold for k_encode_prune's screening pass
// from the law of a tile's screened sums (DESIGN.md 4 "tau guess"), for the
// device and for the host, where tests/test_tau_guess.py checks it against the
// formula in float64 and against Monte Carlo.
//
// A tile's candidates are iid N(0,1) rows by construction, whatever the data.
// The screening pass scores a row by s = -Q,
//     Q = sum_j (alpha_j z_j + beta_j)^2,   z iid N(0,1),
// alpha_j = sA_j / sqrt(2 ln 2) and beta_j = sB_j of the tile's VisitRec: a
// weighted noncentral chi-square whose cumulant function is, with w = alpha^2
// and b2 = beta^2 (= w delta^2 for delta = beta / alpha),
//     K(t) = sum_j [ -1/2 ln(1 - 2 t w_j) + t b2_j / (1 - 2 t w_j) ],   t < 0.
// The best rows are the lower tail of Q.  The Lugannani-Rice formula gives
//     P(Q <= K'(t)) ~ Phi(r) + phi(r) (1/r - 1/u),
//     r = -sqrt(2 (t K'(t) - K(t))),  u = t sqrt(K''(t)),
// and tau_guess_q solves P = m / N for t: q_m = K'(t) is the level that on
// average m of the tile's N candidates fall below.  The kernel starts tau at
// the lower bound of a row at that level.  Nothing here has to be exact or
// even right: the kernel checks at the end of the tile that a real row passed
// the guess and otherwise runs the tile again without it.
//
// f(x) = ln P at t = -e^x falls from ln 1/2 with a slope that steepens to
// -d/2, and -t^2 K''(t) is that slope to leading order (d(-r^2/2)/dt =
// -t K''), so Newton's iteration in x with this slope converges from both
// sides in a handful of steps; a step is held to two e-folds.
#pragma once
#include <math.h>
#include <stdint.h>

#include "cwq_math.h"

#ifndef CWQ_TAU_GUESS_M
#define CWQ_TAU_GUESS_M 6  // rows expected below the guessed level (A/B of 4..16)
#endif

namespace cwq {

constexpr int kTauGuessM = CWQ_TAU_GUESS_M;
constexpr int kTauGuessIters = 12;        // Newton steps at most
constexpr float kTauGuessTol = 0x1p-12f;  // |ln P - ln(m/N)| at which the solve stops
constexpr float kTauNoGuess = -1.0f;      // q_m >= 0: a negative value says "no guess"
// m / N above this: small tiles, where r nears the formula's singular point
// r = 0 and a guess has nothing to gain
constexpr float kTauGuessMaxP = 0x1p-9f;
// sum w and sum b2 outside these: the terms' squares leave the float range
constexpr float kTauGuessWMin = 0x1p-60f, kTauGuessWMax = 0x1p60f;

struct TauGuessSums {
  float k, k1, k2;  // a dim's terms of K, K', K'' (or their sums over the tile's dims)
};

// one dim's terms at t < 0; w = b2 = 0 (a lane without a dim) gives zeros
CWQ_HD TauGuessSums tau_guess_terms(float w, float b2, float t) {
  const float den = 1.0f - 2.0f * t * w;  // >= 1
  const float r = 1.0f / den;
  const float wb = w + b2 * r;
  TauGuessSums o;
  o.k = -0.5f * logf(den) + t * b2 * r;
  o.k1 = r * wb;
  o.k2 = 2.0f * w * r * r * (wb + b2 * r);
  return o;
}

// ln of the Lugannani-Rice lower tail at t < 0 from the sums; NaN or -inf where
// the formula gives no probability
CWQ_HD float tau_guess_logp(const TauGuessSums& s, float t) {
  const float h = t * s.k1 - s.k;           // r^2 / 2
  const float x = sqrtf(2.0f * h);          // -r
  const float au = -t * sqrtf(s.k2);        // -u
  const float phi = 0.3989422804f * expf(-h);
  const float p = 0.5f * erfcf(x * 0.7071067812f) + phi * (1.0f / au - 1.0f / x);
  return logf(p);
}

// Dims: the tile's (w_j, b2_j).  dims.sum(f) returns the sum over the dims of
// f(w_j, b2_j), a TauGuessSums, the same in every thread that takes part: a
// loop on the host (TauGuessHostDims), on the device one dim per lane and a
// butterfly over the wave.  n_cand = N, the tile's candidates.
template <class Dims>
CWQ_HD float tau_guess_q(const Dims& dims, int64_t n_cand, int m) {
  if (m < 1 || n_cand < 1) return kTauNoGuess;
  const float p0 = (float)m / (float)n_cand;
  if (!(p0 <= kTauGuessMaxP)) return kTauNoGuess;
  const TauGuessSums tot =
      dims.sum([](float w, float b2) { return TauGuessSums{w, b2, 0.0f}; });
  const float wsum = tot.k, bsum = tot.k1;
  // zero proposal scale (every row is the same point), NaN, inf, or scales
  // whose squares leave the float range
  if (!(wsum >= kTauGuessWMin && wsum <= kTauGuessWMax && bsum <= kTauGuessWMax))
    return kTauNoGuess;
  const float lp0 = logf(p0);
  // start where 1 - 2 t w is about 9 for a dim of the mean weight
  float x = logf(4.0f * (float)dims.count() / wsum);
  for (int it = 0; it < kTauGuessIters; ++it) {
    const float t = -expf(x);
    const TauGuessSums s = dims.sum([t](float w, float b2) { return tau_guess_terms(w, b2, t); });
    const float f = tau_guess_logp(s, t) - lp0;
    const float slope = t * t * s.k2;  // -df/dx to leading order
    if (!(f - f == 0.0f && slope > 0.0f && slope - slope == 0.0f)) return kTauNoGuess;
    if (__builtin_fabsf(f) <= kTauGuessTol) {
      // the last Newton step taken on q itself: dq = K'' dt, dt = f / (t K'')
      const float q = s.k1 + f / t;
      return (q - q == 0.0f && q >= 0.0f) ? q : kTauNoGuess;
    }
    float dx = f / slope;
    dx = dx > 2.0f ? 2.0f : (dx < -2.0f ? -2.0f : dx);
    x += dx;
  }
  return kTauNoGuess;  // not converged
}

// the host's Dims: alpha and beta of d dims
struct TauGuessHostDims {
  const float* alpha;
  const float* beta;
  int d;
  int count() const { return d; }
  template <class F>
  TauGuessSums sum(F f) const {
    TauGuessSums a{0.0f, 0.0f, 0.0f};
    for (int j = 0; j < d; ++j) {
      const TauGuessSums o = f(alpha[j] * alpha[j], beta[j] * beta[j]);
      a.k += o.k;
      a.k1 += o.k1;
      a.k2 += o.k2;
    }
    return a;
  }
};

}  // namespace cwq
