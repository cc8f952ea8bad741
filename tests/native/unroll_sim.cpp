// Host replay of the control flow of k_encode_prune's screening loop as it is
// unrolled (CWQ_SHARE_UNROLL, CWQ_PARK_LOOK_MASK;
// csrc/cwq_kernels.hip), together with the descending hand-out of
// tests/native/refill_desc_sim.cpp and the parked completion of park_sim.cpp.
//
// The pass is two loops.  The unrolled one runs trips of U copies of the body
// with no exit inside a trip, while every lane is active and the pool holds
// the 64 U rows that U refills can take at most (cwq_refill.h
// unroll_trip_rows); its copies do not read or write the active mask.  The
// one-copy loop behind it hands out the rest and tests the active mask at its
// end; a lane turns inactive in its pool refill only.  The tau share and the
// look for parked rows fall on the copies that cwq_refill.h unroll_due names.
//
// A row's fate is drawn in advance, as in park_sim.cpp: it drops at unit u in
// 1 .. G, or it reaches the end.  Checked for U in {1, 2, 4, 8}, look masks 3
// and 7, with and without parking, whatever the rows do:
//   * every row of [0, R) is started exactly once, on a Philox block below
//     2^32 (the wave's share may end at block 2^32 exactly);
//   * every row that reaches the end is seen by the keep step exactly once,
//     with all its units and nothing else summed, before the wave leaves; no
//     other row is; a parked row waits for at most the look mask's iterations;
//   * inside a trip of the unrolled loop every refill's rows are in range and
//     every lane stays active;
//   * every copy that runs has an active lane: the wave leaves behind the
//     refill in which its last lane turns inactive, with no further copy run,
//     and a wave that starts with no row runs no copy;
//   * the share falls on every eighth iteration and the look on every
//     (mask + 1)-th, counted over both loops.
// tests/test_unroll_plan.py builds and runs this; it prints "ok" and exits 0,
// or says what broke and exits 1.
#include <cstdint>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "../../compression_without_quantization_amd/csrc/cwq_refill.h"

namespace {

int g_fail = 0;
#define CHECK(c, ...)                    \
  do {                                   \
    if (!(c)) {                          \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
      ++g_fail;                          \
    }                                    \
  } while (0)

constexpr uint32_t kShareMask = 7u;  // CWQ_TAU_SHARE_MASK

struct Wave {
  uint32_t R, G, w0g;
  bool park;
  std::vector<uint32_t> fate, next, started, kept, dropped;
  uint32_t ng[64], kp[64], real[64], waited[64];
  bool active[64], left[64];
  uint32_t ng_end, wnext_g;
  uint32_t iter = 0;       // the kernel's counter
  uint64_t iters = 0;      // iterations run, counted here
  uint64_t copies = 0, fast_copies = 0, shares = 0;

  bool any_active() const {
    for (bool a : active)
      if (a) return true;
    return false;
  }
  bool all_active() const {
    for (bool a : active)
      if (!a) return false;
    return true;
  }
  void start(uint32_t l) {
    const uint32_t row = ng[l] / G;
    CHECK(ng[l] % G == 0u && row < R, "R=%u G=%u lane %u: starts ng = %u", R, G, l, ng[l]);
    if (row < R) ++started[row];
    CHECK((uint64_t)w0g + ng[l] + (G - 1u) < (1ull << 32), "R=%u G=%u: block of row %u wraps", R,
          G, row);
  }

  // copy C of a loop of UU copies; true: its refill turned the last lane inactive
  template <uint32_t UU, uint32_t LOOK, uint32_t C>
  bool copy() {
    constexpr bool FAST = UU > 1u;
    constexpr uint32_t LM = LOOK;
    ++copies;
    ++iters;
    if (FAST) ++fast_copies;
    CHECK(any_active(), "R=%u G=%u U=%u: a copy runs with no active lane", R, G, UU);
    if (FAST) CHECK(all_active(), "R=%u G=%u U=%u: unrolled copy with an inactive lane", R, G, UU);
    constexpr bool COUNTS =
        cwq::unroll_counts<kShareMask, UU>() || (cwq::unroll_counts<LM, UU>());
    if (COUNTS && C + 1u == UU) iter += UU;
    const bool share_due = cwq::unroll_due<kShareMask, UU, C>(iter);
    const bool look_due = cwq::unroll_due<LM, UU, C>(iter);
    CHECK(share_due == ((iters & kShareMask) == 0u), "U=%u copy %u: share at iteration %llu", UU, C,
          (unsigned long long)iters);
    CHECK(look_due == ((iters & LM) == 0u), "U=%u copy %u look mask %u: look at iteration %llu", UU,
          C, LM, (unsigned long long)iters);
    if (share_due) ++shares;

    bool below[64], done[64], pool[64], any_pool = false;
    for (uint32_t l = 0; l < 64; ++l) {
      const uint32_t rec = kp[l];
      below[l] = false;
      bool complete = false;
      if (rec < G) {
        ++real[l];
        if (active[l]) below[l] = fate[ng[l] / G] == real[l];
      } else if (active[l]) {
        ++waited[l];  // at the sentinel: nothing added, never below
      }
      kp[l] = next[rec];
      if (!park) complete = kp[l] == 0u;  // the last record links to 0
      done[l] = below[l] || complete || (FAST ? false : !active[l]);
      if (active[l] && below[l]) {
        ++dropped[ng[l] / G];
        CHECK(rec + 1u == fate[ng[l] / G], "R=%u G=%u: row %u dropped at unit %u, not %u", R, G,
              ng[l] / G, rec + 1u, fate[ng[l] / G]);
      }
      // without parking: the keep step of this iteration
      if (!park && complete && active[l] && !below[l]) keep(l);
    }
    if (park && look_due) {
      for (uint32_t l = 0; l < 64; ++l) {
        if (!(kp[l] == G && (FAST || active[l]) && !below[l])) continue;
        CHECK(waited[l] <= LM, "R=%u G=%u: row %u waited %u iterations (mask %u)", R, G, ng[l] / G,
              waited[l], LM);
        keep(l);
        done[l] = true;
      }
    }
    // the step, the resets and the pool refill
    for (uint32_t l = 0; l < 64; ++l) {
      pool[l] = false;
      if (done[l]) {
        const bool borrow = ng[l] < 64u * G;
        ng[l] -= 64u * G;
        left[l] = left[l] || borrow;
        kp[l] = 0;
        real[l] = 0;
        waited[l] = 0;
        pool[l] = left[l];
      }
      any_pool = any_pool || pool[l];
    }
    bool leave = false;
    if (any_pool) {
      uint32_t rank = 0;
      for (uint32_t l = 0; l < 64; ++l)
        if (pool[l]) ng[l] = wnext_g + (rank++) * G;
      const uint32_t want = wnext_g + rank * G;
      if (FAST) {
        CHECK(want <= ng_end, "R=%u G=%u U=%u: an unrolled refill runs out of rows", R, G, UU);
        wnext_g = want;
      } else if (want <= ng_end) {
        wnext_g = want;
        for (uint32_t l = 0; l < 64; ++l)
          if (pool[l]) active[l] = true;
      } else {
        wnext_g = ng_end;
        for (uint32_t l = 0; l < 64; ++l) active[l] = ng[l] < ng_end;
        leave = !any_active();
      }
    }
    for (uint32_t l = 0; l < 64; ++l)
      if (done[l] && active[l]) start(l);
    return leave;
  }
  void keep(uint32_t l) {
    const uint32_t row = ng[l] / G;
    CHECK(ng[l] % G == 0u && row < R, "R=%u G=%u lane %u: keeps ng = %u", R, G, l, ng[l]);
    if (row >= R) return;
    CHECK(fate[row] == G + 1u, "R=%u G=%u: row %u kept, fate %u", R, G, row, fate[row]);
    CHECK(real[l] == G, "R=%u G=%u: row %u kept with %u of its units", R, G, row, real[l]);
    ++kept[row];
  }
  template <uint32_t U, uint32_t LOOK, uint32_t... I>
  void trip(std::integer_sequence<uint32_t, I...>) {
    (copy<U, LOOK, I>(), ...);
  }
};

// p_reach: share of rows that reach the end; the others drop at a uniform unit
template <uint32_t U, uint32_t LOOK>
void run(uint32_t R, uint32_t G, bool park, bool at_end, double p_reach, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::bernoulli_distribution reach(p_reach);
  Wave w;
  w.R = R;
  w.G = G;
  w.park = park;
  // the wave's first Philox block: its share ends at block 2^32 exactly, or starts at 0
  w.w0g = at_end ? (uint32_t)((1ull << 32) - (uint64_t)R * G) : 0u;
  w.fate.resize(R);
  for (uint32_t r = 0; r < R; ++r) w.fate[r] = reach(rng) ? G + 1u : 1u + (uint32_t)(rng() % G);
  const uint32_t S = cwq::refill_static_rows(R);
  const uint32_t ng_stat = S * G;
  w.ng_end = R * G;
  w.wnext_g = cwq::refill_pool_start(S) * G;
  const uint32_t ng_first = ng_stat != 0u ? ng_stat - 64u * G : 0u;
  // the wave's records: parked, position k links to k + 1 and the sentinel G
  // to itself; otherwise the last links to 0
  w.next.resize(G + 1u);
  for (uint32_t k = 0; k <= G; ++k) w.next[k] = park ? (k < G ? k + 1u : G) : (k + 1u < G ? k + 1u : 0u);
  w.started.assign(R, 0u);
  w.kept.assign(R, 0u);
  w.dropped.assign(R, 0u);
  for (uint32_t l = 0; l < 64; ++l) {
    w.ng[l] = ng_first + l * G;
    w.kp[l] = 0;
    w.real[l] = 0;
    w.waited[l] = 0;
    w.left[l] = ng_stat == 0u;
    w.active[l] = w.ng[l] < w.ng_end;
    if (w.active[l]) w.start(l);
  }
  const uint64_t guard = (uint64_t)R * (G + 9u) + 64u;
  // the unrolled loop
  if (U > 1u) {
    while (w.all_active() && w.wnext_g + cwq::unroll_trip_rows(U) * G <= w.ng_end) {
      w.template trip<U, LOOK>(std::make_integer_sequence<uint32_t, U>{});
      if (w.copies > guard) break;
    }
    CHECK(w.fast_copies % U == 0u, "R=%u G=%u U=%u: left inside a trip", R, G, U);
  }
  // the one-copy loop; only its pool refill changes the active mask
  while (w.any_active()) {
    const bool was_last = w.template copy<1u, LOOK, 0u>();
    CHECK(was_last == !w.any_active(), "R=%u G=%u U=%u: the active mask changed outside a refill", R,
          G, U);
    if (w.copies > guard) break;
  }
  CHECK(w.copies <= guard, "R=%u G=%u U=%u: the loop does not end", R, G, U);
  if (R == 0u) CHECK(w.copies == 0u, "U=%u G=%u: a wave with no row ran %llu copies", U, G,
                     (unsigned long long)w.copies);
  // a share of 4,096 rows or more has 512 pool rows: the unrolled loop must run
  if (U > 1u && R >= 4096u) CHECK(w.fast_copies > 0u, "R=%u G=%u U=%u: no unrolled trip", R, G, U);
  CHECK(w.shares == w.iters / (kShareMask + 1u), "R=%u G=%u U=%u: %llu shares in %llu iterations", R,
        G, U, (unsigned long long)w.shares, (unsigned long long)w.iters);
  for (uint32_t l = 0; l < 64; ++l)
    CHECK(!w.active[l], "R=%u G=%u lane %u: active at the loop's end", R, G, l);
  for (uint32_t r = 0; r < R; ++r) {
    CHECK(w.started[r] == 1u, "R=%u G=%u U=%u p=%.2f: row %u started %u times", R, G, U, p_reach, r,
          w.started[r]);
    const bool reaches = w.fate[r] == G + 1u;
    CHECK(w.kept[r] == (reaches ? 1u : 0u), "R=%u G=%u U=%u p=%.2f: row %u (fate %u) kept %u times",
          R, G, U, p_reach, r, w.fate[r], w.kept[r]);
    CHECK(w.dropped[r] == (reaches ? 0u : 1u),
          "R=%u G=%u U=%u p=%.2f: row %u (fate %u) dropped %u times", R, G, U, p_reach, r, w.fate[r],
          w.dropped[r]);
    if (g_fail > 20) return;
  }
}

template <uint32_t U, uint32_t LOOK>
void sweep(uint64_t& seed) {
  const uint32_t shares[] = {0, 1, 16, 63, 64, 65, 128, 256, 1024, 4096, 4097, 5000, 16384};
  for (uint32_t R : shares)
    for (uint32_t G : {2u, 8u, 16u})
      for (bool park : {true, false})
        for (double p : {0.0, 0.0002, 0.5, 1.0}) {
          if (g_fail > 20) return;
          const uint64_t s = seed++ * 0x9e3779b97f4a7c15ull + R;
          run<U, LOOK>(R, G, park, /*at_end=*/(seed & 1u) != 0u, p, s);
        }
}

}  // namespace

int main() {
  uint64_t seed = 1;
  sweep<1, 7>(seed);
  sweep<2, 7>(seed);
  sweep<4, 7>(seed);
  sweep<8, 7>(seed);
  sweep<1, 3>(seed);
  sweep<2, 3>(seed);
  sweep<4, 3>(seed);
  sweep<8, 3>(seed);
  if (g_fail) return 1;
  std::printf("ok\n");
  return 0;
}
