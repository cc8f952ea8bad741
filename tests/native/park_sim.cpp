// Host replay of the control flow of k_encode_prune's screening loop in its
// PARK instances (CWQ_PARK_COMPLETE; csrc/cwq_kernels.hip, "Parked rows"),
// together with the descending hand-out of tests/native/refill_desc_sim.cpp.
//
// A wave's records are linked: position k to k + 1, the last real one to the
// sentinel, the sentinel to itself.  The loop has no completion test.  A lane
// is finished in an iteration when its row's upper end falls below tau at the
// position it has just visited (never at the sentinel, whose B is +inf) or
// when it is inactive.  Every eighth iteration the lanes whose next
// position is the sentinel, that are active and did not just fall below, take
// the keep step and are finished too.
//
// A row's fate is drawn in advance: it drops at unit u in 1 .. G (u = G: at
// its last real position, so it completes without reaching), or it reaches the
// end.  Checked, whatever the rows do:
//   * every row of [0, R) is started exactly once (the hand-out is unchanged);
//   * every row that reaches the end is seen by the keep step exactly once,
//     with all its G real units summed and none twice (the sentinel adds
//     nothing), and on the lane's own ng; no other row is seen by it;
//   * no lane is left parked when the loop ends, and a parked lane waits for
//     at most 7 iterations after the one that brought it to the sentinel;
//   * a row's drop is taken at the unit drawn for it: parking changes no
//     drop.
// G in {2, 4, 8, 16}; shares of 1 row and up; rows that all reach the end, that
// never do, and mixtures.  tests/test_park_plan.py builds and runs this; it
// prints "ok" and exits 0, or says what broke and exits 1.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../compression_without_quantization_amd/csrc/cwq_refill.h"

namespace {

int g_fail = 0;
#define CHECK(c, ...)                    \
  do {                                   \
    if (!(c)) {                          \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
      if (++g_fail > 20) return;         \
    }                                    \
  } while (0)

constexpr uint32_t kShareMask = 7u;  // CWQ_TAU_SHARE_MASK

// p_reach: share of rows that reach the end; the others drop at a uniform unit
void run(uint32_t R, uint32_t G, double p_reach, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::bernoulli_distribution reach(p_reach);
  std::vector<uint32_t> fate(R);  // unit at which the row drops; G + 1: reaches the end
  for (uint32_t r = 0; r < R; ++r) fate[r] = reach(rng) ? G + 1u : 1u + (uint32_t)(rng() % G);

  const uint32_t S = cwq::refill_static_rows(R);
  const uint32_t ng_end = R * G, ng_stat = S * G;
  uint32_t wnext_g = cwq::refill_pool_start(S) * G;
  const uint32_t ng_first = ng_stat != 0u ? ng_stat - 64u * G : 0u;
  // the wave's records: next[k] for k < G, the sentinel G
  std::vector<uint32_t> next(G + 1u);
  for (uint32_t k = 0; k <= G; ++k) next[k] = k < G ? k + 1u : G;

  std::vector<uint32_t> started(R, 0u), kept(R, 0u), dropped(R, 0u);
  uint32_t ng[64], kp[64], real[64], waited[64];
  bool active[64], left[64];
  bool any = false;
  for (uint32_t l = 0; l < 64; ++l) {
    ng[l] = ng_first + l * G;
    kp[l] = 0;
    real[l] = 0;
    waited[l] = 0;
    left[l] = ng_stat == 0u;
    active[l] = ng[l] < ng_end;
    if (active[l]) ++started[ng[l] / G];
    any = any || active[l];
  }
  uint32_t iter = 0;
  uint64_t guard = 0;
  while (any) {
    CHECK(++guard <= (uint64_t)R * (G + 9u) + 64u, "R=%u G=%u: the loop does not end", R, G);
    bool below[64], done[64], pool[64], any_pool = false;
    // the visit and the drop test
    for (uint32_t l = 0; l < 64; ++l) {
      const uint32_t rec = kp[l];
      below[l] = false;
      if (rec < G) {
        ++real[l];
        if (active[l]) below[l] = fate[ng[l] / G] == real[l];
      } else if (active[l]) {
        ++waited[l];  // at the sentinel: nothing added, never below
      }
      kp[l] = next[rec];
      done[l] = below[l] || !active[l];
      if (active[l] && below[l]) {
        ++dropped[ng[l] / G];
        CHECK(rec + 1u == fate[ng[l] / G], "R=%u G=%u: row %u dropped at unit %u, not %u", R, G,
              ng[l] / G, rec + 1u, fate[ng[l] / G]);
      }
    }
    // every eighth iteration: the parked lanes take the keep step
    if (((++iter) & kShareMask) == 0u) {
      for (uint32_t l = 0; l < 64; ++l) {
        if (!(kp[l] == G && active[l] && !below[l])) continue;
        const uint32_t row = ng[l] / G;
        CHECK(ng[l] % G == 0u && row < R, "R=%u G=%u lane %u: keeps ng = %u", R, G, l, ng[l]);
        CHECK(fate[row] == G + 1u, "R=%u G=%u: row %u kept, fate %u", R, G, row, fate[row]);
        CHECK(real[l] == G, "R=%u G=%u: row %u kept with %u of its units", R, G, row, real[l]);
        CHECK(waited[l] <= kShareMask, "R=%u G=%u: row %u waited %u iterations", R, G, row,
              waited[l]);
        ++kept[row];
        done[l] = true;
      }
    }
    // the step, the resets and the pool refill (refill_desc_sim.cpp)
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
    if (any_pool) {
      uint32_t rank = 0;
      for (uint32_t l = 0; l < 64; ++l)
        if (pool[l]) ng[l] = wnext_g + (rank++) * G;
      const uint32_t want = wnext_g + rank * G;
      if (want <= ng_end) {
        wnext_g = want;
        for (uint32_t l = 0; l < 64; ++l)
          if (pool[l]) active[l] = true;
      } else {
        wnext_g = ng_end;
        for (uint32_t l = 0; l < 64; ++l) active[l] = ng[l] < ng_end;
      }
    }
    any = false;
    for (uint32_t l = 0; l < 64; ++l) {
      any = any || active[l];
      CHECK(!active[l] || ng[l] < ng_end, "R=%u G=%u lane %u: active out of range", R, G, l);
      if (done[l] && active[l]) ++started[ng[l] / G];
    }
  }
  // the loop has ended: nothing is parked, every row has met its fate once
  for (uint32_t l = 0; l < 64; ++l)
    CHECK(!active[l], "R=%u G=%u lane %u: active at the loop's end", R, G, l);
  for (uint32_t r = 0; r < R; ++r) {
    CHECK(started[r] == 1u, "R=%u G=%u p=%.2f: row %u started %u times", R, G, p_reach, r,
          started[r]);
    const bool reaches = fate[r] == G + 1u;
    CHECK(kept[r] == (reaches ? 1u : 0u), "R=%u G=%u p=%.2f: row %u (fate %u) kept %u times", R, G,
          p_reach, r, fate[r], kept[r]);
    CHECK(dropped[r] == (reaches ? 0u : 1u), "R=%u G=%u p=%.2f: row %u (fate %u) dropped %u times",
          R, G, p_reach, r, fate[r], dropped[r]);
  }
}

}  // namespace

int main() {
  const uint32_t shares[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 255, 256, 1000, 2048, 16384};
  uint64_t seed = 1;
  for (uint32_t R : shares)
    for (uint32_t G : {2u, 4u, 8u, 16u})
      for (double p : {0.0, 0.0002, 0.05, 0.5, 1.0})
        for (int rep = 0; rep < 3; ++rep) run(R, G, p, seed++ * 0x9e3779b97f4a7c15ull + R);
  if (g_fail) return 1;
  std::printf("ok\n");
  return 0;
}
