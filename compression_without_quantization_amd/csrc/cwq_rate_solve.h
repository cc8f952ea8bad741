// cwq_rate_solve.h -- budgets under a bit total, solved without a host wait
// (cwq_choose_bits_total, cwq_ratetable.hip): the bisection of
// ratetable.choose_bits_total taken kSolveLevels halvings at a time.
//
// Sixty halvings of [lam_lo, lam_hi] only ever ask for the total at the nodes of
// a binary tree of intervals.  From the current interval the tree of the next r
// halvings is
//     node 1 = (lam_lo, lam_hi);  node k = (a, b) has mid_k = 0.5 (a + b);
//     node 2k = (a, mid_k);  node 2k + 1 = (mid_k, b),
// the float64 recurrence of the host loop, so mid_k is bit for bit the mid the
// loop computes should it reach node k.  One sweep of the table gives
// total(mid_k) for all 2^r - 1 nodes; the walk then takes r halvings from node
// 1: total_k <= T moves the upper end to mid_k and goes to 2k, anything else
// moves the lower end and goes to 2k + 1.  Nothing is assumed about the totals
// (no monotonicity): the walk reads the same totals the loop would have asked for.
//
// The products mid_k * (double)b that the choose rule subtracts are made here,
// once per node and budget, by the IEEE multiply k_choose_bits does (the sweep
// then only subtracts and compares: they are uniform over the wave).
// tests/test_rate_solve.py drives all of this on the host against a NumPy
// restatement of the loop.  Nothing here needs HIP.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CWQ_SOLVE_HD __host__ __device__ inline
#else
#define CWQ_SOLVE_HD inline
#endif

// Tuning switch: halvings per sweep of the table, a divisor of 60 in [3, 6]
// (tools/bench_choose_total.py measures them).
#ifndef CWQ_SOLVE_LEVELS
#define CWQ_SOLVE_LEVELS 3
#endif

namespace cwq {

constexpr int kSolveHalvings = 60;  // choose_bits_total's
constexpr int kSolveLevels = CWQ_SOLVE_LEVELS;
static_assert(kSolveLevels >= 3 && kSolveLevels <= 6 && kSolveHalvings % kSolveLevels == 0,
              "r divides the 60 halvings; the sweep takes its nodes eight at a time, a wave builds "
              "the tree");
constexpr int kSolveRounds = kSolveHalvings / kSolveLevels;
constexpr int kSolveSlots = 1 << kSolveLevels;  // node slots 0 .. 2^r - 1; slot 0 is no node
constexpr int kSolveBudgets = 31;               // budgets 0 .. CWQ_MAX_BITS_PER_STEP

struct SolveInterval {
  double lo, hi;
};

// The interval of node k >= 1 of the tree over (lo, hi): the path from node 1
// is k's bits below its leading one, most significant first.
CWQ_SOLVE_HD SolveInterval solve_node(SolveInterval iv, int k) {
  int top = 0;
  while ((k >> (top + 1)) != 0) ++top;
  for (int i = top - 1; i >= 0; --i) {
    const double mid = 0.5 * (iv.lo + iv.hi);
    if ((k >> i) & 1)
      iv.lo = mid;
    else
      iv.hi = mid;
  }
  return iv;
}

CWQ_SOLVE_HD double solve_mid(SolveInterval iv) { return 0.5 * (iv.lo + iv.hi); }

// What the choose rule subtracts from value[g][b] at the price `lam`: a float64
// multiply of its own (never fused with the subtract).
CWQ_SOLVE_HD double solve_product(double lam, int b) { return lam * (double)b; }

// Where the products of one tree lie: prod[b * kSolveSlots + k], so that the
// eight nodes the sweep evaluates together are adjacent.  Slot 0 holds 0.
CWQ_SOLVE_HD int solve_prod_at(int b, int k) { return b * kSolveSlots + k; }

// Node k's column of the products, budgets 0 .. n_budgets - 1; k = 0 gives zeros.
CWQ_SOLVE_HD void solve_fill_node(SolveInterval iv, int k, int n_budgets, double* prod) {
  const double mid = k >= 1 ? solve_mid(solve_node(iv, k)) : 0.0;
  for (int b = 0; b < n_budgets; ++b) prod[solve_prod_at(b, k)] = solve_product(mid, b);
}

// What the launches of one call hand each other, in the workspace.
struct SolveState {
  double lo, hi;      // the interval after the rounds so far
  uint64_t span_key;  // solve_span_key's maximum (the first sweep)
  int64_t total0;     // total(0) (the first sweep)
  int32_t done;       // total(0) <= T: the answer is lam = 0, the tree sweeps return at once
  int32_t pad;
};

// The interval the search starts from: total(0) <= T is the answer lam = 0,
// stated as the interval (0, 0), all of whose mids are 0; else (0, span), span
// the largest value[g][b] - value[g][lo] of the table.
CWQ_SOLVE_HD SolveInterval solve_start(int64_t total_at_0, int64_t target, double span) {
  return total_at_0 <= target ? SolveInterval{0.0, 0.0} : SolveInterval{0.0, span};
}

// kSolveLevels halvings from `iv`, given totals[k] = total(mid_k) of its tree.
CWQ_SOLVE_HD SolveInterval solve_walk(SolveInterval iv, const int64_t* totals, int64_t target) {
  int k = 1;
  for (int l = 0; l < kSolveLevels; ++l) {
    const double mid = solve_mid(iv);
    if (totals[k] <= target) {
      iv.hi = mid;
      k = 2 * k;
    } else {
      iv.lo = mid;
      k = 2 * k + 1;
    }
  }
  return iv;
}

// The span's key: value[g][b] - value[g][lo] at b = lo is +0, so the maximum is
// a float64 >= +0, and those order as their bit patterns do: an unsigned
// integer maximum started from 0 is the maximum of the doubles, in any order.
CWQ_SOLVE_HD uint64_t solve_span_key(double s) {
  union {
    double d;
    uint64_t u;
  } c;
  c.d = s > 0.0 ? s : 0.0;  // (a NaN or anything negative: +0)
  return c.u;
}
CWQ_SOLVE_HD double solve_span_of(uint64_t key) {
  union {
    double d;
    uint64_t u;
  } c;
  c.u = key;
  return c.d;
}

// The launches of one call: a reset, the first sweep (lam = 0), then per round a
// one-wave step and a sweep, the last step, and the pass that writes the bits.
constexpr int kSolveLaunches = 2 + 2 * kSolveRounds + 2;

}  // namespace cwq
