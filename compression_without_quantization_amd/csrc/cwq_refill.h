// cwq_refill.h -- how the rows of one wave's share are handed to its 64 lanes
// in k_encode_prune's loops (cwq_kernels.hip), as row arithmetic that the
// kernel and the host share: tests/test_refill_plan.py drives refill_sim.cpp,
// which replays the hand-out on the CPU (DESIGN.md 4 "static-stride refill").
//
// A wave's share is the rows [0, R) relative to its first row.  The first
// S = refill_static_rows(R) of them are the static region: lane l owns rows
// l, l + 64, ... below S and moves on with one add.  The rows [S, R) are the
// dynamic pool: a finished lane whose static rows are used up takes the next
// pool row by its rank among such lanes, from a wave-uniform counter.
//
// Pure integer functions; nothing from HIP is included.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CWQ_REFILL_HD __host__ __device__ __forceinline__
#else
#define CWQ_REFILL_HD inline
#endif

namespace cwq {

constexpr uint32_t kRefillLanes = 64;
// shares below this many rows have no static region (the lanes' first rows
// apart): with fewer than two rows per lane there is no add to save
constexpr uint32_t kRefillMinRows = 128;

// S(R): the largest multiple of 64 not above 7 R / 8; 0 below 128 rows.  The
// last eighth (at least) stays in the pool, which evens out the lanes' static
// quotas: these differ by tens of iterations in hundreds.
CWQ_REFILL_HD uint32_t refill_static_rows(uint32_t R) {
  if (R < kRefillMinRows) return 0u;
  const uint32_t s = (uint32_t)(((uint64_t)R * 7u) >> 3);
  return s & ~(kRefillLanes - 1u);
}

// First pool row handed out by rank.  Every lane starts on row `lane`: in the
// static region when S >= 64, and otherwise (S = 0) the pool starts behind
// those 64 first rows, as it did before there was a static region.
CWQ_REFILL_HD uint32_t refill_pool_start(uint32_t S) { return S < kRefillLanes ? kRefillLanes : S; }

// The unrolled loop (k_encode_prune, CWQ_SHARE_UNROLL).  The loop's body stands
// U times in the loop; an event of period M + 1 iterations (the tau share, the
// look for parked rows; M + 1 a power of two) falls on the iterations whose
// number, counted from 1, is a multiple of M + 1.  With M + 1 <= U that is a
// property of the copy C alone, and nothing is counted.  Otherwise only the
// last copy can hold the event: it adds U to the iteration counter and tests
// it, once per trip.  With U = 1 that is the test of every iteration.
// `iters`: the iterations up to and including this trip.
template <uint32_t M, uint32_t U, uint32_t C>
CWQ_REFILL_HD bool unroll_due(uint32_t iters) {
  static_assert((M & (M + 1u)) == 0u && (U & (U - 1u)) == 0u && U >= 1u && C < U,
                "unroll_due: M + 1 and U are powers of two, C < U");
  if constexpr (M + 1u <= U)
    return ((C + 1u) & M) == 0u;
  else if constexpr (C + 1u != U)
    return false;
  else
    return (iters & M) == 0u;
}
// whether the last copy counts the iterations for an event of period M + 1
template <uint32_t M, uint32_t U>
constexpr bool unroll_counts() { return M + 1u > U; }
// pool rows that must be left for a trip of U copies to be sure of its rows:
// a refill hands out at most a row per lane
constexpr uint32_t unroll_trip_rows(uint32_t U) { return U * kRefillLanes; }

}  // namespace cwq
