// Host build of the total solver's plan (csrc/cwq_rate_solve.h) and workspace
// layouts (solve_ws, enc_rate_ws in csrc/cwq_workspace.h) for
// tests/test_rate_solve.py: the tree and the walk of the header driven by a
// plain C++ choose rule, as cwq_ratetable.hip's launches drive them.  Test-only
// shim; not part of the product.
#include <stdint.h>

#include <vector>

#include "../../compression_without_quantization_amd/csrc/cwq_rate_solve.h"
#include "../../compression_without_quantization_amd/csrc/cwq_workspace.h"

namespace {

// k_choose_bits' rule with the products given: column k of prod.
int choose_row(const float* row, const double* prod, int k, int lo, int hi) {
  int best_b = lo;
  double best = (double)row[lo] - prod[cwq::solve_prod_at(lo, k)];
  for (int b = lo + 1; b <= hi; ++b) {
    const double s = (double)row[b] - prod[cwq::solve_prod_at(b, k)];
    if (s > best) best = s, best_b = b;
  }
  return best_b;
}

}  // namespace

extern "C" {

// out: kSolveLevels, kSolveRounds, kSolveSlots, kSolveHalvings, kSolveLaunches, sizeof(SolveState)
void rs_consts(int64_t* out) {
  out[0] = cwq::kSolveLevels;
  out[1] = cwq::kSolveRounds;
  out[2] = cwq::kSolveSlots;
  out[3] = cwq::kSolveHalvings;
  out[4] = cwq::kSolveLaunches;
  out[5] = (int64_t)sizeof(cwq::SolveState);
}

// node k's interval of the tree over (lo, hi), and its mid
void rs_node(double lo, double hi, int k, double* out) {
  const cwq::SolveInterval iv = cwq::solve_node(cwq::SolveInterval{lo, hi}, k);
  out[0] = iv.lo;
  out[1] = iv.hi;
  out[2] = cwq::solve_mid(iv);
}

double rs_span_round_trip(double s) { return cwq::solve_span_of(cwq::solve_span_key(s)); }
uint64_t rs_span_key(double s) { return cwq::solve_span_key(s); }

// The launch sequence of cwq_choose_bits_total on the host: the first sweep,
// then per round a step (start or walk, lay out the tree) and a sweep, the last
// step and the pass at the final lam_hi.
void rs_solve(const float* value, int64_t nb, int n_cols, int64_t target, int lo, int hi,
              int32_t* out_bits, double* out_lam, int64_t* out_total) {
  std::vector<double> prod((size_t)n_cols * cwq::kSolveSlots, -1.0);  // (not zero: the steps fill it)
  std::vector<int64_t> totals(cwq::kSolveSlots, -1);
  int64_t total0 = 0;
  uint64_t span = 0;
  for (int64_t g = 0; g < nb; ++g) {
    const float* row = value + g * n_cols;
    int best_b = lo;
    double best = (double)row[lo] - cwq::solve_product(0.0, lo);
    for (int b = lo + 1; b <= hi; ++b) {
      const double s = (double)row[b] - cwq::solve_product(0.0, b);
      if (s > best) best = s, best_b = b;
      const uint64_t k = cwq::solve_span_key((double)row[b] - (double)row[lo]);
      span = k > span ? k : span;
    }
    total0 += best_b;
  }
  cwq::SolveInterval iv{};
  const bool done = total0 <= target;
  for (int round = 0; round <= cwq::kSolveRounds; ++round) {
    if (round == 0)
      iv = cwq::solve_start(total0, target, cwq::solve_span_of(span));
    else if (!done)
      iv = cwq::solve_walk(iv, totals.data(), target);
    if (round == cwq::kSolveRounds) break;
    for (int k = 0; k < cwq::kSolveSlots; ++k) {
      cwq::solve_fill_node(iv, k, n_cols, prod.data());
      totals[k] = 0;
    }
    if (done) continue;  // the sweeps return at once
    for (int64_t g = 0; g < nb; ++g)
      for (int k = 0; k < cwq::kSolveSlots; ++k)
        totals[k] += choose_row(value + g * n_cols, prod.data(), k, lo, hi);
  }
  *out_lam = iv.hi;
  *out_total = 0;
  for (int64_t g = 0; g < nb; ++g) {
    const float* row = value + g * n_cols;
    int best_b = lo;
    double best = (double)row[lo] - cwq::solve_product(iv.hi, lo);
    for (int b = lo + 1; b <= hi; ++b) {
      const double s = (double)row[b] - cwq::solve_product(iv.hi, b);
      if (s > best) best = s, best_b = b;
    }
    out_bits[g] = best_b;
    *out_total += best_b;
  }
}

// out: (off, bytes) of state, prod, totals; then the total
void rs_solve_ws(int64_t base, int max_bits_table, int64_t* out) {
  const cwq::SolveWs l = cwq::solve_ws((size_t)base, max_bits_table);
  const cwq::Region r[3] = {l.state, l.prod, l.totals};
  for (int i = 0; i < 3; ++i) out[2 * i] = (int64_t)r[i].off, out[2 * i + 1] = (int64_t)r[i].bytes;
  out[6] = (int64_t)l.total;
}

// out: (off, bytes) of rate, tidx, tvalue, solve.state, solve.prod, solve.totals;
// then the total and cwq_rate_table's own (ragged) total
void rs_enc_rate_ws(int64_t nb, int64_t total_dims, int64_t max_block_dim, int max_bits,
                    int64_t* out) {
  const cwq::EncRateWs l = cwq::enc_rate_ws(nb, total_dims, max_block_dim, max_bits);
  const cwq::Region r[6] = {l.rate, l.tidx, l.tvalue, l.solve.state, l.solve.prod, l.solve.totals};
  for (int i = 0; i < 6; ++i) out[2 * i] = (int64_t)r[i].off, out[2 * i + 1] = (int64_t)r[i].bytes;
  out[12] = (int64_t)l.total;
  out[13] = (int64_t)cwq::rate_ws(true, nb, total_dims, max_block_dim, max_bits).total;
}
}
