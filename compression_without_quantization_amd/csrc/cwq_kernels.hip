// cwq_kernels.hip -- gfx950 kernels of the greedy coded sampler.
//
// Hot path: for every block (the reference's "group")
// and every step, 2^b candidates are drawn from the proposal shard with the
// stateless Philox stream, scored by the target log-density and reduced to
// the argmax; the decoder regenerates only the selected row.
//
// Mapping:
//   * one "tile" = (block g, candidate range [n0, n1)), one 256-thread
//     workgroup per tile; a block whose 2^b candidates would leave the chip
//     idle is split over several tiles and merged with one 64-bit atomicMax
//     per workgroup on an orderable (value, ~index) key.
//   * inside a workgroup, wave v owns the candidates n == n0 + v (mod 4), so
//     the Philox word alignment (n*d) mod 4 is uniform within a wave and the
//     "start a new Philox block" branch is a scalar branch even for odd d.
//   * candidates are never materialised: each lane regenerates its row's
//     normals in registers (Philox -> Box-Muller -> shard -> log-prob) and
//     accumulates them in the Eigen AVX summation order.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <stdint.h>

#include "cwq_device.h"
#include "cwq_kernels.h"
#include "cwq_refill.h"
#include "cwq_tau_guess.h"

namespace cwq {

// ---------------------------------------------------------------------------
// Per-dimension constants of a step (coded_greedy_sampler.py:42-48).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_prep_dims(
    const float* __restrict__ t_scale, const float* __restrict__ p_loc,
    const float* __restrict__ p_scale, int64_t n, float nst, float sdiv, float rho,
    float* __restrict__ loc_s, float* __restrict__ scale_s, float* __restrict__ lognorm,
    float* __restrict__ out_sample, unsigned long long* __restrict__ keys, int64_t nb) {
  // step 0's argmax keys start at 0 (one launch less than a memset)
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < nb;
       g += (int64_t)gridDim.x * blockDim.x)
    keys[g] = 0ull;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float ls, ss;
    shard_consts(p_loc[i], p_scale[i], nst, sdiv, rho, ls, ss);
    loc_s[i] = ls;
    scale_s[i] = ss;
    lognorm[i] = lognorm_of(t_scale[i]);
    out_sample[i] = 0.0f;  // best_sample = tf.zeros (:68)
  }
}

// ---------------------------------------------------------------------------
// One candidate row: sum_j log N(best_j + loc_s_j + scale_s_j z_j; mu_j, s_j)
// in the Eigen 3.3 AVX inner-dim reduction order.
//   kbase = n*d (flat index of the row's first normal), align = kbase & 3
//   (wave-uniform).  DC > 0: compile-time dimension (DC % 4 == 0 -> align 0).
// ---------------------------------------------------------------------------
// Greedy candidate row (coded_greedy_sampler.py:57-59).
template <int DC, bool STEP0>
__device__ __forceinline__ float eval_row(const PhiloxStream& st, uint64_t kbase, int64_t d_rt,
                                          int align_rt, const float* __restrict__ loc_s,
                                          const float* __restrict__ scale_s,
                                          const float* __restrict__ mu,
                                          const float* __restrict__ sg,
                                          const float* __restrict__ lognorm,
                                          const float* __restrict__ best,
                                          const double* logtab) {
  return eval_row_f<DC>(st, kbase, d_rt, align_rt, logtab, [&](int64_t e, float zz) -> float {
    float s = scale_s[e] * zz;  // misc.py:14
    s = loc_s[e] + s;           // misc.py:15
    const float tv = STEP0 ? s : best[e] + s;  // :57 (best == +0 at step 0)
    return log_prob(tv, mu[e], sg[e], lognorm[e]);
  });
}

// ---------------------------------------------------------------------------
// Encoder, one step: every tile scores its candidate range and folds its best
// (value, index) into keys[g] with one atomicMax.
// ---------------------------------------------------------------------------
template <int DC, bool STEP0>
__global__ void __launch_bounds__(256) k_encode_eval(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const float* __restrict__ best,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t ntiles, int64_t tiles_per_block,
    int64_t cand_per_tile, int64_t n_cand, SeedSpec sd, int32_t step,
    unsigned long long* __restrict__ keys) {
  __shared__ double logtab[32];
  __shared__ unsigned long long wkey[4];
  fill_logtab(logtab);
  const uint32_t wv = wave_id();
  const uint32_t lane = threadIdx.x & 63u;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t g = tile / tiles_per_block;
    const int64_t tt = tile - g * tiles_per_block;
    const BlockSpan sp = block_span(block_off, ud, g);
    const int64_t n0 = tt * cand_per_tile;
    const int64_t n1 = (n0 + cand_per_tile < n_cand) ? n0 + cand_per_tile : n_cand;
    const PhiloxStream st =
        generate_key(step_seed(sd.of(g), step), 42);
    const int align = (int)(((uint64_t)(n0 + wv) * (uint64_t)sp.d) & 3u);

    uint64_t bestk = 0;
    for (int64_t n = n0 + 4 * (int64_t)lane + wv; n < n1; n += 256) {
      const float v = eval_row<DC, STEP0>(st, (uint64_t)n * (uint64_t)sp.d, sp.d, align,
                                          loc_s + sp.off, scale_s + sp.off, t_loc + sp.off,
                                          t_scale + sp.off, lognorm + sp.off,
                                          STEP0 ? nullptr : best + sp.off, logtab);
      const uint64_t k = argmax_key(v, (uint32_t)n);
      bestk = k > bestk ? k : bestk;
    }
    bestk = wave_max_u64(bestk);
    if (lane == 0) wkey[wv] = bestk;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t m = wkey[0];
      for (int i = 1; i < 4; ++i) m = wkey[i] > m ? wkey[i] : m;
      if (m) atomicMax(&keys[g], (unsigned long long)m);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Pruned encoder for uniform blocks, D % 8 == 0, D <= 64 (the C1/C4/C5 shapes).
//
// Same result as k_encode_eval, less work: a candidate whose log-density can
// no longer reach a value already achieved in this tile is dropped before its
// remaining dims are generated.
//
// Order: each block's D/4 Philox groups are visited in decreasing order of
// their expected log-density deficit under the proposal shard (the dims that
// discriminate most first), one group (4 dims, one Philox block) per step.
//
// Drop rule ("pruning bound"): after the first k visited groups,
// with float running sum s of their log-densities, candidate n is dropped iff
//     s + 2^-14 |s| + B_k  <  tau
// where B_k >= sum_{unvisited j} f(M_j) + 2^-14 K_k (+ float evaluation
// margin), M_j = -c_j is the largest value the float log-density of dim j can
// take, f(x) = x + g|x| with g >= gamma_{D-1} + gamma_{D}, and K_k sums
// |M_j| + M_j over the visited dims.  The left side bounds from above the
// float Eigen-order value of every completion of the row; tau is a lower
// bound of the exact value of a candidate already completed in this tile.  So
// a dropped candidate is strictly worse than an existing one: neither the
// argmax nor a tie.
//
// Completion: after all groups, s brackets the exact value within
// [s - 2^-14|s| - L, s + 2^-14|s| + B_D].  Candidates whose upper end reaches
// tau go to an LDS survivor list; at the end of the tile the survivors whose
// upper end reaches the final tau are re-evaluated exactly (natural order,
// Eigen summation: eval_row's value, computed with a lane per Philox block by
// score_rows_wave) and only those produce argmax keys.
//
// Lanes keep one candidate each and take another when theirs completes or is
// dropped, so waves stay full even though candidates stop after different
// numbers of groups: first the lane's own rows of the wave's share, a stride
// of 64 apart, then rows of a common pool from a per-wave counter with
// ballot/mbcnt (cwq_refill.h).
// ---------------------------------------------------------------------------
constexpr float kPruneC1 = 0x1p-14f;
#ifndef CWQ_PRUNE_MIN_WAVES
#define CWQ_PRUNE_MIN_WAVES 6  // waves/SIMD the register allocator must allow (tools/variants.sh)
#endif
#ifndef CWQ_DEFER_MIN_WAVES
// ... for the screening-only form (FORM 1), which holds no exact arithmetic;
// its tile queue grid is 256 CUs x this many resident workgroups
#define CWQ_DEFER_MIN_WAVES 8
#endif
#ifndef CWQ_XCD_BALANCE
#define CWQ_XCD_BALANCE 1 // INTER tiles: each XCD runs every block (see k_encode_prune)
#endif
#ifndef CWQ_TAU_SHARE_MASK
// k_encode_prune shares tau across the workgroup every 8 units: a share is one
// returning LDS max and two VALU instructions (tau_share_wave).  Every 16: C4
// 280.9 against 279.6 ms, C5 33.40 against 33.45 (DESIGN.md 4 "VALU budget")
#define CWQ_TAU_SHARE_MASK 7u
#endif
#ifndef CWQ_CSR_TAU_SHARE_MASK
#define CWQ_CSR_TAU_SHARE_MASK 15u  // k_encode_prune_csr: a wave reduce per share, every 16 units
#endif
#ifndef CWQ_SURVIVOR_CAP
#define CWQ_SURVIVOR_CAP 1024
#endif
#ifndef CWQ_LINKED_VISIT
// the screening loop takes its next visit position from the record it has just
// read (VisitRec::next); 0: it adds the record size (A/B builds)
#define CWQ_LINKED_VISIT 1
#endif
#ifndef CWQ_FOLD_ROUND0
// the screening loop takes a visit's Philox block as (lane's row part) +
// (record's part) inside round 0's multiply-add, from per-wave records
// (VisitRec::add); 0: one record set, the block formed by a v_add3 (A/B builds)
#define CWQ_FOLD_ROUND0 1
#endif
#ifndef CWQ_BORROW_REFILL
// static rows are handed out downwards and the subtract's borrow tells which
// lanes have used theirs up; 0: upwards, with a compare per iteration (A/B builds)
#define CWQ_BORROW_REFILL 1
#endif
#ifndef CWQ_POOL_RANGE_SKIP
// the pool refill leaves out its range compare when the wave's counter shows
// that every row handed out is in range (CWQ_BORROW_REFILL builds); 0: always compares
#define CWQ_POOL_RANGE_SKIP 1
#endif
#ifndef CWQ_PARK_COMPLETE
// in tiles of CWQ_PARK_MIN_ROWS rows or more at d = 32, of as many Philox
// blocks at other d, of blocks of CWQ_PARK_MIN_D dims or more (the kernel's
// PARK instances; the rule is launch_prune_t's) a row that has passed its last visit position is not looked for every
// iteration: it walks on to a sentinel record and waits there for the
// iteration that shares tau, which finds it (k_encode_prune); 0: every tile
// takes the completion compare per iteration (A/B builds)
#define CWQ_PARK_COMPLETE 1
#endif
#ifndef CWQ_PARK_MIN_ROWS
#define CWQ_PARK_MIN_ROWS 8192
#endif
#ifndef CWQ_PARK_MIN_D
#define CWQ_PARK_MIN_D 16  // ... and of blocks of at least this many dims (launch_prune_t)
#endif
#if CWQ_PARK_COMPLETE && !(CWQ_LINKED_VISIT && CWQ_BORROW_REFILL)
#error "CWQ_PARK_COMPLETE needs CWQ_LINKED_VISIT and CWQ_BORROW_REFILL"
#endif
#ifndef CWQ_SHARE_UNROLL
// While a wave's pool holds the rows that a trip can take at most, the
// screening loop runs trips of this many copies of its body (1, 2, 4 or 8)
// with no exit and no test of the active mask inside a trip, the tau share in
// the last copy: at 8 = CWQ_TAU_SHARE_MASK + 1 no iteration counts or tests a
// counter (cwq_refill.h unroll_due, unroll_trip_rows).  The one-copy loop
// behind it hands out the rest.  1: that loop alone (A/B builds).  C4 against
// 1: at 2 +0.4 ms, at 4 -1.4 ms, at 8 -3.8 ms of 255.5
#define CWQ_SHARE_UNROLL 8
#endif
#ifndef CWQ_PARK_LOOK_MASK
// PARK instances look for parked rows every CWQ_PARK_LOOK_MASK + 1 iterations
// (a v_cmp and a scalar test each; a parked row idles for at most that many).
// Every 4th (3u) in copies 4 and 8: C4 +2.7 ms against every 8th
#define CWQ_PARK_LOOK_MASK CWQ_TAU_SHARE_MASK
#endif
#if CWQ_SHARE_UNROLL != 1 && CWQ_SHARE_UNROLL != 2 && CWQ_SHARE_UNROLL != 4 && CWQ_SHARE_UNROLL != 8
#error "CWQ_SHARE_UNROLL is 1, 2, 4 or 8"
#endif

// best + (loc_s + scale_s z) - mu  (misc.py:14-15, coded_greedy_sampler.py:57, TFP _z numerator)
template <bool STEP0>
__device__ __forceinline__ float cand_diff(float z, float ls, float ss, float mu, float bb) {
  const float s = shard_sample(ls, ss, z);
  const float tv = STEP0 ? s : bb + s;
  return tv - mu;
}
__device__ __forceinline__ float lp_from_z(float z, float cc) {
  const float u = -0.5f * (z * z);
  return u - cc;
}

// Screening pass (cwq_screen.h, DESIGN.md "screening bound").  On tiles whose
// constants pass the range gate, the drop decisions are taken on the screened
// sum s of -a_j^2 over the visited dims: every completion of the row has an
// exact Eigen-order value
//     E  <=  (1 - 2^-14) s + Bs_k,    Bs_k ~ sum_j M_j + sum_{visited} C_j,
// and a completed row has E >= (1 + 2^-13) s + As - Pq sqrt(-s), which
// feeds tau.  Survivors are re-evaluated exactly as in the exact pass.

// What the screening loop reads at one visit position, in one LDS record: the
// loop carries the record's byte offset, so the three reads share one address
// register and differ in their immediate offsets only.
//
// With CWQ_FOLD_ROUND0 every wave has its own G records.  A lane carries its
// row as ng = (n - w0) G, relative to its wave's first row w0, and the Philox
// block of a visit, ng + w0 G + g_k, is never formed: the record holds
// add = M0 (w0 G + g_k), and round 0's product is M0 ng + add, the multiply
// round 0 needs anyway with the record's pair as its addend
// (cwq_philox_lo.h; ng + w0 G + g_k is a real block index below 2^32, so the
// 64-bit sum does not wrap).  The part w0 G is the wave's own, hence a record
// set per wave.  Without the fold add is g_k itself.
struct VisitRec {
  float4 sa, sb;     // a_j = RN(sa z' + sb) of the group's four dims
  uint32_t add[2];   // round 0's addend (low, high word), or {g_k, 0}
  int bk;            // bits of B_{k+1}
  int next;          // byte offset of the next visit position's record; 0 in the last
};
static_assert(sizeof(VisitRec) == 48, "VisitRec: 48 bytes");

// Up to RW = min(64 / G, 8) survivor rows of a D-dim block (G = D / 4) scored
// exactly by one wave (a lane per row would run a whole row's arithmetic with
// the other 63 idle when, as usual, a tile has one such row).  Lane l <
// cnt * G computes the four terms of Philox block l % G of row rows[l / G]
// into buf; lane 8 r + a then sums row r's terms a, a + 8, ... in order: the
// eight accumulators of eval_row_f, whose tail sum stays the +0 it starts from
// since D % 8 == 0.  Returns to every lane of 8 r .. 8 r + 7 the value of row
// r < cnt, eval_row<D, STEP0>'s bit for bit.  Full exec mask; cnt is uniform.
//
// The two halves are functions of their own, which k_score_survivors shares:
// there the rows of one pass come from different blocks, so the stream and the
// constants are the lane's.
// The four terms of Philox block u of `row` into rowterms[4 u .. 4 u + 3]
// (rowterms: the row's D terms; the constants: the row's block).
template <int D, bool STEP0>
__device__ __forceinline__ void score_block_terms(
    const PhiloxStream& st, uint32_t row, uint32_t u, const float* __restrict__ loc_s,
    const float* __restrict__ scale_s, const float* __restrict__ mu,
    const float* __restrict__ sg, const float* __restrict__ lognorm,
    const float* __restrict__ best, const double* logtab, float* rowterms) {
  constexpr uint32_t G = D / 4;
  const F4 z = normal4_dev(st, (uint64_t)row * G + u, logtab);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t j = 4u * u + (uint32_t)t;
    const float zz = t == 0 ? z.a : (t == 1 ? z.b : (t == 2 ? z.c : z.d));
    float v = scale_s[j] * zz;  // misc.py:14
    v = loc_s[j] + v;           // misc.py:15
    const float tv = STEP0 ? v : best[j] + v;
    rowterms[j] = log_prob(tv, mu[j], sg[j], lognorm[j]);
  }
}
// The Eigen-order sum of the rows' terms in buf (row r's at buf + r D): lanes
// 8 r .. 8 r + 7 get row r's value where `valid` (the same in those eight
// lanes).  Waits for the wave's writes of buf first.  Full exec mask.
template <int D>
__device__ __forceinline__ float score_fold8(const float* buf, uint32_t lane, bool valid) {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float acc = 0.0f;
  const uint32_t fr = lane >> 3;
  if (valid)
    for (uint32_t e = lane & 7u; e < (uint32_t)D; e += 8u) acc = acc + buf[fr * D + e];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float p[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) p[l] = __shfl(acc, (int)((lane & ~7u) + (uint32_t)l), 64);
  return eigen_fold8(p, 0.0f);
}
template <int D, bool STEP0>
__device__ __forceinline__ float score_rows_wave(
    const PhiloxStream& st, const uint32_t* rows, uint32_t cnt, const float* __restrict__ loc_s,
    const float* __restrict__ scale_s, const float* __restrict__ mu,
    const float* __restrict__ sg, const float* __restrict__ lognorm,
    const float* __restrict__ best, const double* logtab, float* buf, uint32_t lane) {
  constexpr uint32_t G = D / 4;
  const uint32_t r = lane / G, u = lane - r * G;
  if (r < cnt)
    score_block_terms<D, STEP0>(st, rows[r], u, loc_s, scale_s, mu, sg, lognorm, best, logtab,
                                buf + r * D);
  return score_fold8<D>(buf, lane, (lane >> 3) < cnt);
}

// What the screening-only form of k_encode_prune (FORM 1) and the launch over
// the deferred list (FORM 2) take beyond the kernel's own arguments; the
// single-launch form (FORM 0) takes nothing.
template <int FORM>
struct DeferArgs {
  uint32_t* surv;    // [nb][kDeferSlots]
  uint32_t* count;   // [nb]
  uint32_t* list;    // [nb]
  uint32_t* dcount;  // the list's length
  int q;             // Q in [0, kDeferSlots]; -1: every tile is deferred (tests)
};
template <>
struct DeferArgs<0> {};

#ifdef CWQ_TILE_TIMES
// timing builds only (tools/tile_times.py): per tile of k_encode_prune its
// start / end wall clock (s_memrealtime, 100 MHz) and the workgroup that ran it
constexpr int kTileTimes = 1 << 18;
__device__ unsigned long long g_tile_t0[kTileTimes], g_tile_t1[kTileTimes];
__device__ unsigned int g_tile_wg[kTileTimes];
#endif
#ifdef CWQ_PRUNE_STATS
// tuning builds only (tools/prune_stats.py): [0..64] candidates finished after
// k units, [65] completed rows, [66] survivors pushed, [67] screened tiles,
// [70] wave-iterations that took the pool refill, [71] wave-iterations,
// [50] tiles started from a tau guess, [51] tiles run again without it;
// general kernel (tools/csr_stats.py): [40]/[41] screened/exact tiles, [42] rows
// finished, [43] dims screened, [44] rows completed, [45] survivors pushed,
// [46] list-full exact rows, [47] survivors re-evaluated, [48] lane-iterations
__device__ unsigned long long g_prune_stats[72];
// "oracle tau" experiment: each tile's best key is saved; with g_seed_tau set
// the next launch starts every tile at the exact best value of the last one
constexpr int kDbgBlocks = 1 << 20;
__device__ unsigned long long g_dbg_best[kDbgBlocks];
__device__ int g_seed_tau;
#endif

// cwq_tau_guess.h's Dims on the device: a dim per lane (w = b2 = 0 in the
// other lanes), summed by a butterfly that leaves the same bits in every lane.
// Full exec mask.
struct TauGuessWaveDims {
  float w, b2;
  int d;
  __device__ __forceinline__ int count() const { return d; }
  template <class F>
  __device__ __forceinline__ cwq::TauGuessSums sum(F f) const {
    cwq::TauGuessSums o = f(w, b2);
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
      o.k += __shfl_xor(o.k, sh, 64);
      o.k1 += __shfl_xor(o.k1, sh, 64);
      o.k2 += __shfl_xor(o.k2, sh, 64);
    }
    return o;
  }
};
// a 64-bit value that is in scalar registers already, marked wave-uniform
__device__ __forceinline__ uint64_t sgpr_pair_uniform(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
// qm_cell's test value (allow_screen bits 1-2 == 2): tau_g = FLT_MAX, which no
// row reaches, so every screened tile takes the retry
constexpr float kTauForceRetry = -2.0f;
// tau_g from the cell: the lower bound of a completed row whose screened sum
// is -q_m; -inf without a guess (never NaN)
__device__ __forceinline__ float tau_guess_of(float qm, float As, float Pq) {
  if (qm == kTauForceRetry) return 3.402823466e+38f;
  if (!(qm >= 0.0f)) return -__builtin_inff();
  const float tg = cwq::screen_row_lower(-qm, cwq::kScreenC2, As, Pq);
  return tg == tg ? tg : -__builtin_inff();
}

// one trip of an unrolled loop: the body's copies 0 .. U - 1 in turn
template <class F, uint32_t... I>
__device__ __forceinline__ void unroll_each(F& f, std::integer_sequence<uint32_t, I...>) {
  (f(std::integral_constant<uint32_t, I>{}, std::integral_constant<uint32_t, (uint32_t)sizeof...(I)>{}), ...);
}

// PARK: the screening loop without its per-iteration completion test
// (CWQ_PARK_COMPLETE; chosen per launch from the rows per tile, launch_prune_t)
//
// FORM (one tile per block, INTER = false; DESIGN.md 4 "Deferral"):
//   0  the whole of the above in one launch.
//   1  screening only.  The loop, the set-up, the guess and its retry are the
//      same; at the tile's end the rows of the survivor list that reach
//      tau_final go to the block's slots in the workspace (DeferArgs::surv,
//      count) and k_score_survivors scores them.  A tile that fails the
//      screening gate, whose list overflows or that has more than Q such rows
//      writes count 0 and its block to the deferred list instead: it runs
//      again under FORM 2.  Every tile writes its count; keys is not touched.
//      Nothing here scores a row exactly, so the f64 code and its registers
//      are not in this form (CWQ_DEFER_MIN_WAVES).
//   2  FORM 0 over the deferred list: tile t is block list[t], t < *dcount.
template <int D, bool STEP0, bool INTER, bool PARK, int FORM = 0>
__global__ void __launch_bounds__(256, FORM == 1 ? CWQ_DEFER_MIN_WAVES : CWQ_PRUNE_MIN_WAVES)
k_encode_prune(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const float* __restrict__ best, int64_t ntiles_arg,
    int64_t tiles_per_block, int64_t cand_per_tile, int64_t n_cand, SeedSpec sd, int32_t step,
    int allow_screen, unsigned long long* __restrict__ keys, int64_t tail_from, int tail_div,
    uint32_t* __restrict__ tq, DeferArgs<FORM> df) {
  static_assert(D % 8 == 0 && D >= 8 && D <= 64, "pruned path: D % 8 == 0, D <= 64");
  static_assert(!PARK || CWQ_PARK_COMPLETE, "PARK instances exist in CWQ_PARK_COMPLETE builds only");
  static_assert(FORM == 0 || !INTER, "deferral: one tile per block");
  constexpr int G = D / 4;
  constexpr int NF = STEP0 ? 6 : 7;  // loc_s, scale_s, mu, sigma, c, 1/sigma[, best]
  // survivor rows one wave scores per pass: a lane per Philox block of a row,
  // eight lanes per row in the fold (score_rows_wave)
  constexpr int RW = (64 / G) < 8 ? (64 / G) : 8;
  __shared__ double logtab[32];
  __shared__ float4 cst[G * NF];     // constants of the k-th visited group
  // screening pass: all it reads at the k-th visited group; set w is wave w's
  constexpr int NREC = CWQ_FOLD_ROUND0 ? 4 : 1;
  // PARK: each set ends in a sentinel record, which the last visit position
  // links to and which links to itself.  Its sa and sb are 0, so a visit
  // leaves s as it is (a = fma(0, z', 0) = 0 for the finite z', s = fma(-0, 0,
  // s) = s), and its B is +inf, so upper = fma(s, c1, +inf) = +inf is below no
  // tau (s is finite): a row that gets there has completed, and waits with its
  // s and its ng until it is found.
  constexpr int RPW = G + (PARK ? 1 : 0);  // records per set
  __shared__ VisitRec vrec[NREC * RPW];
  __shared__ uint32_t w0g_cell[4];   // per wave: its first row's Philox block (the loops' rare paths)
  __shared__ int2 meta[G];           // {Philox group of visit k, bits of B_{k+1}}
  __shared__ float rowbuf[4][RW * D];  // per wave: the terms of RW survivor rows
  __shared__ float dscore[D];
  __shared__ float dA[D];            // screening: A_j (additive error, a units)
  __shared__ float dC[D];            // screening: C_j
  __shared__ float gscore[G];
  __shared__ int gpos[G];
  __shared__ float lowc;             // L: lower-end constant of a completed row
  __shared__ float scr_a, scr_pq;    // screening: As, Pq
  __shared__ float tau_cell;         // the workgroup's tau (a float, never NaN: LDS float max)
  __shared__ float tau_seed_cell;    // what the tile really starts from: -inf or keys[g]'s value
  __shared__ float qm_cell;          // tau guess: q_m, kTauNoGuess or kTauForceRetry (tau_guess_of)
  __shared__ uint32_t sq_cnt;
  __shared__ uint32_t sq_n[CWQ_SURVIVOR_CAP];
  __shared__ float sq_ub[CWQ_SURVIVOR_CAP];
  __shared__ unsigned long long wkey[4];
  __shared__ uint32_t s_next;
#ifdef CWQ_PRUNE_STATS
  // per-workgroup counters (LDS atomics), added to g_prune_stats once per tile:
  // one global atomic per finished candidate made C5-sized runs take minutes
  __shared__ uint32_t s_ps[72];
  for (int i = threadIdx.x; i < 72; i += blockDim.x) s_ps[i] = 0u;
#endif
  __shared__ uint32_t dq_cnt;  // FORM 1: the list's rows that reach tau_final
  // (FORM 1 scores nothing: no table, no rowbuf, no wkey)
  if constexpr (FORM != 1) fill_logtab(logtab);
  int64_t ntiles = ntiles_arg;
  if constexpr (FORM == 2) {  // the deferred list's length: uniform, and at most nb < 2^31
    ntiles = (int64_t)__builtin_amdgcn_readfirstlane((int)*df.dcount);
    if (ntiles > ntiles_arg) ntiles = ntiles_arg;
  }
  const uint32_t wv = wave_id();
  const uint32_t lane = threadIdx.x & 63u;

  // INTER (several tiles per block, high rates): tiles run block-interleaved
  // (tile t is tile t / nb of block t % nb), so a block's later tiles start
  // after its first ones have finished and begin from the exact best value
  // they left in keys[g] instead of from -inf
  constexpr bool inter = INTER;
  const int64_t nbt = INTER ? ntiles / tiles_per_block : 0;
  // tile queue (tq != nullptr): a workgroup's first tile is its id, later ones
  // come from one atomic counter, so workgroups stay resident until the queue
  // is empty.  With one tile per workgroup the resident count fell from 1,514
  // to 1,414 of 1,536 slots over a C5 launch as finished workgroups were
  // replaced (tools/tile_times.py); the queue keeps every slot busy to the end.
  auto next_tile = [&](int64_t cur) -> int64_t {
    if (tq == nullptr) return cur + gridDim.x;
    __syncthreads();
    if (threadIdx.x == 0) s_next = gridDim.x + atomicAdd(tq, 1u);
    __syncthreads();
    return (int64_t)s_next;
  };
  for (int64_t tile = blockIdx.x; tile < ntiles; tile = next_tile(tile)) {
    // thread index re-derived per tile behind an opaque move: the per-thread
    // addresses below are then recomputed (cheap) instead of hoisted out of the
    // tile loop and spilled under the 6-waves/SIMD register budget
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
#ifdef CWQ_TILE_TIMES
    if (tid == 0 && tile < kTileTimes) {
      g_tile_t0[tile] = __builtin_amdgcn_s_memrealtime();
      // HW_REG_XCC_ID (hwreg 20), bits [3:0]: the XCD this workgroup runs on
      const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg((20) | (0 << 6) | ((4 - 1) << 11));
      g_tile_wg[tile] = (xcc << 24) | (blockIdx.x & 0xffffffu);
    }
#endif
    // XCD balance (INTER): workgroups go to the 8 XCDs round-robin by id, so
    // with the block-interleaved order XCD x would run only the blocks == x
    // (mod 8), and with few blocks per XCD their uneven pruning left XCDs idle
    // at the end (tools/tile_times.py: 84% of the slots busy on 128 blocks).
    // XCD x instead runs the x-th eighth of the interleaved order: every block,
    // a contiguous range of its tiles.
    // Only the full-size tiles are spread so: the short tail tiles (below) come
    // last in their natural order, so every XCD gets its share of them too.
    int64_t tord = tile;
    const int64_t treg = inter ? nbt * tail_from : 0;  // full-size tiles
    if (inter && CWQ_XCD_BALANCE && tq == nullptr && tile < treg && (treg & 7) == 0 &&
        (gridDim.x & 7u) == 0)
      tord = (tile & 7) * (treg >> 3) + (tile >> 3);
    int64_t g = inter ? tord % nbt : tile / tiles_per_block;
    int64_t tt = inter ? tord / nbt : tile - g * tiles_per_block;
    if constexpr (FORM == 2) {  // the tile of a listed block (tile < *dcount <= nb)
      g = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)df.list[tile]);
      tt = 0;
    }
    const int64_t off = g * D;
    // a block's tiles from tail_from on are tail_div times smaller: the last
    // rounds of the launch drain in short tiles (INTER; tail_div 1: no tail)
    int64_t n0, csz;
    if (tt < tail_from) {
      n0 = tt * cand_per_tile;
      csz = cand_per_tile;
    } else {
      csz = cand_per_tile / tail_div;
      n0 = tail_from * cand_per_tile + (tt - tail_from) * csz;
    }
    const int64_t n1 = (n0 + csz < n_cand) ? n0 + csz : n_cand;
    if (n0 >= n1) continue;  // (uniform) a tail piece past the block's candidates
    const PhiloxStream st =
        generate_key(step_seed(sd.of(g), step), 42);

    // (a) expected deficit of dim j under the proposal shard:
    //     E[0.5((T - mu)/sigma)^2], T ~ N(best + loc_s, scale_s^2)
    if (tid < D) {
      const int j = tid;
      const float ls = loc_s[off + j], ss = scale_s[off + j], mu = t_loc[off + j];
      const float rs = 1.0f / t_scale[off + j];
      const float m = (STEP0 ? ls : best[off + j] + ls) - mu;
      float e = 0.5f * (ss * ss + m * m) * (rs * rs);
      dscore[j] = (e == e) ? e : -1.0f;
    }
    __syncthreads();
    // (b) group scores, (c) visit order: rank by decreasing score, ties by index
    if (tid < G) {
      const int q = tid;
      gscore[q] = ((dscore[4 * q] + dscore[4 * q + 1]) + dscore[4 * q + 2]) + dscore[4 * q + 3];
    }
    __syncthreads();
    if (tid < G) {
      const int q = tid;
      const float sq = gscore[q];
      int r = 0;
      for (int q2 = 0; q2 < G; ++q2) {
        const float s2 = gscore[q2];
        r += (s2 > sq || (s2 == sq && q2 < q)) ? 1 : 0;
      }
      gpos[q] = r;
      meta[r].x = q;
#pragma unroll
      for (int w = 0; w < NREC; ++w) {
        // wave w's first row is n0 + w per_wave (as below); a wave whose share
        // is empty reads no record, so a product that wraps there is harmless
        const uint32_t wg = (uint32_t)(n0 + (int64_t)w * ((n1 - n0 + 3) / 4)) * (uint32_t)G;
        const uint64_t add =
            CWQ_FOLD_ROUND0 ? cwq::philox_round0_addend(wg + (uint32_t)q) : (uint64_t)q;
        VisitRec& v = vrec[w * RPW + r];
        v.add[0] = (uint32_t)add;
        v.add[1] = (uint32_t)(add >> 32);
        // the last position links to 0, or to the set's sentinel (PARK)
        v.next = (r + 1 < G || PARK) ? (w * RPW + r + 1) * (int)sizeof(VisitRec) : 0;
      }
    }
    if (PARK && tid >= 64 && tid < 64 + NREC) {  // the sentinels (any Philox block will do: add 0)
      VisitRec& v = vrec[(tid - 64) * RPW + G];
      v.sa = float4{0.f, 0.f, 0.f, 0.f};
      v.sb = float4{0.f, 0.f, 0.f, 0.f};
      v.add[0] = 0u;
      v.add[1] = 0u;
      v.bk = (int)f2u(__builtin_inff());
      v.next = (int)((tid - 64) * RPW + G) * (int)sizeof(VisitRec);
    }
    __syncthreads();
    // (d) constants in visit order (reloaded: nothing is held across the syncs)
    int den_ok = 1, scr_ok = 1;
    if (tid < D) {
      const int j = tid, k = gpos[j >> 2], w = j & 3;
      float fj[7];
      const float sgj = t_scale[off + j];
      fj[0] = loc_s[off + j];
      fj[1] = scale_s[off + j];
      fj[2] = t_loc[off + j];
      fj[3] = sgj;
      fj[4] = lognorm[off + j];
      fj[5] = 1.0f / sgj;
      fj[6] = STEP0 ? 0.0f : best[off + j];
      float* c = reinterpret_cast<float*>(cst);
#pragma unroll
      for (int f = 0; f < NF; ++f) c[(k * NF + f) * 4 + w] = fj[f];
      den_ok = markstein_ok_den(sgj) ? 1 : 0;
      // screening constants; the gate includes den_ok's test of sigma
      const ScreenDim o = screen_dim<STEP0>(fj[0], fj[1], fj[2], sgj, fj[4], fj[6]);
#pragma unroll
      for (int c = 0; c < NREC; ++c) {
        float* sc = reinterpret_cast<float*>(&vrec[c * RPW + k]);
        sc[w] = o.sa;
        sc[4 + w] = o.sb;
      }
      dA[j] = o.A;
      dC[j] = o.C;
      scr_ok = o.ok ? 1 : 0;
    }
    const bool fastdiv = __syncthreads_and(den_ok) != 0;
    const bool scr_all = __syncthreads_and(scr_ok) != 0;
    // (e) drop bounds: thread k computes B_k for the first k visited groups
    //     (exact or screening form); thread G + 1 the screening constants
    bool screen = (allow_screen & 1) && scr_all;
    if constexpr (FORM == 1) screen = screen && df.q >= 0;  // (q < 0: every tile deferred)
    // tau guess (cwq_tau_guess.h): while wave 0 sums the bounds below, wave 1
    // solves for q_m, a dim per lane, from the records (d) has just written
    if (wv == 1u) {
      const int gmode = (allow_screen >> 1) & 3;
      float qm = cwq::kTauNoGuess;
      if (screen && gmode == 1) {
        float w = 0.0f, b2 = 0.0f;
        if (lane < (uint32_t)D) {
          const float* sc = reinterpret_cast<const float*>(&vrec[lane >> 2]);
          const float al = sc[lane & 3u] * (float)(1.0 / cwq::kSqrt2Ln2);
          const float be = sc[4u + (lane & 3u)];
          w = al * al;
          b2 = be * be;
        }
        qm = cwq::tau_guess_q(TauGuessWaveDims{w, b2, D}, n1 - n0, cwq::kTauGuessM);
      } else if (screen && gmode == 2) {
        qm = kTauForceRetry;
      }
      if (lane == 0) qm_cell = qm;
    }
    if (tid <= G + 1) {
      const int kb = tid;
      const float* c = reinterpret_cast<const float*>(cst);
      double rf = 0.0, kk = 0.0, asum = 0.0, msum = 0.0, kall = 0.0, cvis = 0.0, a2 = 0.0,
             amax = 0.0;
#pragma unroll 1
      for (int p = 0; p < D; ++p) {  // p = 4 * (visit position) + w
        const double mj = -(double)c[((p >> 2) * NF + 4) * 4 + (p & 3)];  // M_j = -c_j
        const double aj = __builtin_fabs(mj);
        asum += aj;
        msum += mj;
        kall += aj + mj;
        if (p >= 4 * kb) {
          rf += mj + 0x1p-17 * aj;
        } else {
          kk += aj + mj;
          if (screen) cvis += (double)dC[(meta[p >> 2].x << 2) + (p & 3)];
        }
        if (screen && kb == G + 1) {
          const double av = (double)dA[p];
          a2 += av * av;
          amax = av > amax ? av : amax;
        }
      }
      const double marg = 0x1p-20 * (__builtin_fabs(rf) + asum) + 0x1p-126;
      const double sl = 0x1p-14 * (__builtin_fabs(msum) + asum + kall) + 0x1p-126;
      if (kb <= G) {
        const float bk = screen ? round_up_f32(msum + cvis * (1.0 + 0x1p-20) + sl)
                                : round_up_f32(rf + 0x1p-14 * kk + marg);
        if (kb >= 1) {
          meta[kb - 1].y = (int)f2u(bk);
#pragma unroll
          for (int c = 0; c < NREC; ++c) vrec[c * RPW + kb - 1].bk = (int)f2u(bk);
        }
        if (kb == G) lowc = round_up_f32(0x1p-14 * kk + marg);
      } else if (screen) {  // As, Pq with this kernel's fixed 2^-14 slack
        scr_a = screen_as(msum, sl, a2);
        scr_pq = screen_pq(amax, D);
      }
      if (kb == 0) {
        // the cell holds tau as a float; the keys' order is undone here, once
        // per tile
        float t0 = -__builtin_inff();
        if (inter) {  // an actual row's exact value: no larger than the block's best
          const unsigned long long kv =
              __hip_atomic_load(&keys[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if ((uint32_t)(kv >> 32) > kArgmaxClampOrd) t0 = unord_f32((uint32_t)(kv >> 32));
        }
#ifdef CWQ_PRUNE_STATS
        if (g_seed_tau && g < kDbgBlocks && (g_dbg_best[g] >> 32) > kArgmaxClampOrd)
          t0 = unord_f32((uint32_t)(g_dbg_best[g] >> 32));
#endif
        tau_cell = t0;
        tau_seed_cell = t0;
        sq_cnt = 0u;
      }
    }
    __syncthreads();
    const float lc = lowc;
#ifdef CWQ_PRUNE_STATS
    const float tau_seed = tau_cell;
#endif
    const float sA = scr_a, sPq = scr_pq;

    // this wave's contiguous share of the tile's candidates
    const int64_t per_wave = (n1 - n0 + 3) / 4;
    const int64_t w0 = n0 + (int64_t)wv * per_wave;
    const int64_t w1 = (w0 + per_wave < n1) ? w0 + per_wave : n1;
    // A lane carries its row as ng = (n - w0) * G, the row's first Philox block
    // relative to the wave's.  The block of a visit, ng + w0g + group, is
    // formed inside round 0's multiply-add from the wave's records (VisitRec;
    // without CWQ_FOLD_ROUND0 by one v_add3), the range test is one compare
    // with ng_end, and the refill one mad.  Rows and Philox blocks stay below
    // 2^32 in this kernel (launch_prune_t); ng itself stays below
    // (per_wave + 128) * G, far below 2^32 (a wave's share is a quarter of a
    // tile), except in a lane that has just run out of static rows (below).
    // The wave-uniform values are made scalar once per tile, so the loop's
    // counters run on the SALU.  w0g is kept in LDS for the places that need
    // it outside the screening loop's common path (a survivor's row, the
    // exact pass), so that it holds no scalar register across the loop.
    const uint32_t w0g =
        (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)w0 * (uint32_t)G));
    if (lane == 0) w0g_cell[wv] = w0g;  // read by this wave only: LDS keeps a wave's order
    const uint32_t wrows = w1 > w0 ? (uint32_t)(w1 - w0) : 0u;  // R, the wave's share
    const uint32_t ng_end =
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(wrows * (uint32_t)G));
    // Static-stride refill (cwq_refill.h).  The first S = refill_static_rows(R)
    // rows of the share are handed out without any lane arithmetic: lane l
    // owns rows l, l + 64, ... below S.  The rows [S, R) are the dynamic pool,
    // handed to finished lanes by rank from the wave-uniform counter wnext_g,
    // which starts at refill_pool_start(S) * G.  ng_stat = S * G.
    //
    // CWQ_BORROW_REFILL: a lane takes its static rows from the last one down.
    // It starts on row l + S - 64 (row l when S = 0) and a finished lane moves
    // on with ng -= 64 G; the subtract borrows exactly when ng was below 64 G,
    // that is on row l, the lane's last static row.  The borrow bits of the
    // finished lanes go into the scalar mask `left` of the lanes that have
    // left the static region (all ones from the start when S = 0), and the
    // finished lanes of `left` take pool rows in the same iteration.
    //   * Every row of [0, R) is started by exactly one lane, and no row
    //     outside it: the static rows of different lanes are disjoint by
    //     construction (S is a multiple of 64, so each lane owns S / 64 of
    //     them, and walks them all: l + S - 64, ..., l + 64, l), a lane enters
    //     `left` only when its row l is done, and from then on it takes pool
    //     rows only, which the rank arithmetic hands out once each
    //     (tests/native/refill_desc_sim.cpp replays this on the host).  A row
    //     at or past ng_end makes its lane inactive.
    //   * The only wrap is that borrow.  Outside `left` ng >= 64 G before
    //     every subtract but the last, which leaves ng + 2^32 - 64 G in a lane
    //     that is then in `left` and finished, so the pool branch of the same
    //     iteration overwrites it before anything reads it.  Inside `left` a
    //     finished lane's subtract may wrap too (an inactive lane's ng_end
    //     below 64 G; pool rows are not): such a lane is again finished and in
    //     `left`, and overwritten likewise; its borrow bit changes nothing.
    //     The subtract's carry-out is ANDed with the finished lanes' mask: what
    //     it holds for the other lanes is not relied on.
    //   * wnext_g is kept at or below ng_end (rows from there on are out of
    //     range alike), so a pool row is below ng_end + 64 G: ng_end is at most
    //     a quarter of a tile's Philox blocks, far below 2^32.  Only a pool
    //     row can be out of range (static rows are below ng_stat <= ng_end),
    //     so the range test is taken in the pool branch only.
    //   * Which lane scores a row, and when, changes nothing else: tau stays
    //     wave-uniform (the keep branch and the share are as they were), and
    //     a survivor's row is n = (w0g + ng) / G as before.
    // Without CWQ_BORROW_REFILL the static rows go upwards (ng += 64 G from
    // row l) and a compare with ng_stat per iteration finds the lanes past them.
    const uint32_t ng_stat = (uint32_t)__builtin_amdgcn_readfirstlane(
        (int)(cwq::refill_static_rows(wrows) * (uint32_t)G));
    const uint32_t ng_pool0 = (uint32_t)__builtin_amdgcn_readfirstlane(
        (int)(cwq::refill_pool_start(cwq::refill_static_rows(wrows)) * (uint32_t)G));
    // lane 0's first row: S - 64 going down (0 when S = 0), 0 going up
    const uint32_t ng_first =
        (CWQ_BORROW_REFILL && ng_stat != 0u) ? ng_stat - 64u * (uint32_t)G : 0u;
    // the wave's records start here (bytes)
    const uint32_t kbase = CWQ_FOLD_ROUND0 ? wv * (uint32_t)(RPW * sizeof(VisitRec)) : 0u;
#ifndef CWQ_TAU_FROM_KEYS
#define CWQ_TAU_FROM_KEYS 1  // INTER: start the lanes' tau at keys[g]'s value, not at the first share
#endif
    // tau is wave-uniform from here to the end of the tile: it starts so, and
    // the keep branch and the share below both leave the same value in every lane
    //
    // Tau guess.  The screening pass starts tau at the larger of the tile's
    // real start (-inf, or the keys[g] value in INTER: the seed) and tau_g,
    // the lower bound of a row at the predicted level q_m; it is not written to
    // the cell, which the first share raises.  tau_g is no row's bound, so the
    // arguments at the drop tests below hold only once a real row has passed
    // it, which is checked after the pass: see "the guess held" there.
    float tau = (INTER && CWQ_TAU_FROM_KEYS) ? tau_cell : -__builtin_inff();
#ifdef CWQ_PRUNE_STATS
    tau = tau_seed;
    if (tid == 0 && qm_cell >= 0.0f) atomicAdd(&g_prune_stats[50], 1ull);
#endif
    tau = max_f32_quiet(tau, tau_guess_of(qm_cell, sA, sPq));
    uint64_t bestk = 0;

    const PhiloxLo lok = philox_lo_key(st);  // block indices < 2^32 (launch_prune_t)
    auto pass = [&](auto screen_tag) {
      constexpr bool SCREEN = decltype(screen_tag)::value;
      // visit position: the screening pass carries it as the byte offset of
      // its VisitRec, the exact pass as the index k of meta[k] and cst
      constexpr uint32_t KS = SCREEN ? (uint32_t)sizeof(VisitRec) : 1u;
      constexpr bool LINKED = SCREEN && CWQ_LINKED_VISIT;
      // the screening pass of a PARK instance: completed rows wait at the
      // sentinel record (see "Parked rows" in the loop)
      constexpr bool PARKED = SCREEN && PARK && CWQ_PARK_COMPLETE;
      uint32_t ng = ng_first + lane * (uint32_t)G;
      uint32_t wnext_g = ng_pool0;  // (next unassigned pool row - w0) * G: wave-uniform
      // lanes that have left the static region (CWQ_BORROW_REFILL): wave-uniform
      // (opaque, so that it starts in scalar registers: begun in a VGPR pair,
      // the whole chain of ORs and ANDs below was moved to the VALU)
      uint64_t left;
      asm volatile("s_cmp_eq_u32 %1, 0\n\ts_cselect_b64 %0, -1, 0" : "=s"(left) : "s"(ng_stat) : "scc");
      const uint32_t kb = SCREEN ? kbase : 0u;  // the first visit position
      uint32_t kp = kb;
      float s = 0.0f;
      uint32_t iter = 0;
      // the exact pass forms its blocks with a plain add
      uint32_t w0g_x = 0u;
      if constexpr (!SCREEN || !CWQ_FOLD_ROUND0) w0g_x = w0g;
      // a lane is active while its row is in the wave's range: the compare is
      // taken in the pool refill only (static rows are in range), its mask
      // carried in SGPRs.  Each loop's only exit is at its end, so its
      // wave-uniform counters (iter, wnext_g) stay scalar.
      bool active = ng < ng_end;
      uint64_t m_act = __builtin_amdgcn_ballot_w64(active);
      // The body of one iteration, written once: copy C of a loop of UU
      // copies (the unrolled screening loop of a PARK instance: UU =
      // CWQ_SHARE_UNROLL; the loop behind it, the other instances' screening
      // loop and the exact pass: 1).
      //   * Between two pool refills no lane's bit of m_act changes.  m_act is
      //     assigned in the refill and nowhere else: a static row is in range,
      //     a parked lane stays active, and a lane that finishes a row either
      //     steps to a static row or is in m_pool in the same iteration.
      //   * In the unrolled loop (FAST) no refill changes it either (see the
      //     loops below): every lane is active, so the copies neither read
      //     m_act nor write it.
      // Only the PARK instances unroll: the others run shares of 4,096 rows,
      // the fewest with an unrolled trip at U = 8, at d = 8 alone
      // (launch_prune_t), and their keep step, which every copy would hold
      // with its list-full row scoring, made them 84 KB of code against 33.
      constexpr uint32_t U = PARKED ? (uint32_t)CWQ_SHARE_UNROLL : 1u;
      constexpr uint32_t LOOK_MASK = PARKED ? (uint32_t)(CWQ_PARK_LOOK_MASK) : 0u;
      static_assert(LOOK_MASK <= CWQ_TAU_SHARE_MASK, "a look at least as often as a share");
      auto body = [&](auto copy_tag, auto unroll_tag) {
        constexpr uint32_t C = decltype(copy_tag)::value;
        constexpr uint32_t UU = decltype(unroll_tag)::value;  // copies in this loop
        constexpr bool FAST = UU > 1u;
        // iter counts the iterations, a trip at a time, in a loop with a test that needs it
        constexpr bool COUNTS = cwq::unroll_counts<CWQ_TAU_SHARE_MASK, UU>() ||
                                cwq::unroll_counts<LOOK_MASK, UU>();
        if constexpr (COUNTS && C + 1u == UU) iter += UU;
        const bool share_due = cwq::unroll_due<CWQ_TAU_SHARE_MASK, UU, C>(iter);
#ifdef CWQ_PRUNE_STATS
        if (lane == 0) atomicAdd(&s_ps[71], 1u);
#endif
        int2 mt;
        float4 sa, sb;
        uint32_t kp_next = 0;
        uint64_t p0;  // round 0's product of this visit's Philox block
#ifdef CWQ_PRUNE_STATS
        const uint32_t kp_was = kp;
#endif
        if constexpr (SCREEN) {
          const char* rp = reinterpret_cast<const char*>(vrec) + kp;
          sa = *reinterpret_cast<const float4*>(rp);
          sb = *reinterpret_cast<const float4*>(rp + 16);
          typedef int v4i __attribute__((ext_vector_type(4)));
          v4i lk = *reinterpret_cast<const v4i*>(rp + 32);
          // the four words through an opaque move: where the addend is seen
          // as one 64-bit value, the 16-byte read is split in two 8-byte
          // ones, whose offsets no longer fit the record's address register
          if constexpr (CWQ_FOLD_ROUND0) asm volatile("" : "+v"(lk));
          mt = int2{lk.x, lk.z};
          kp_next = (uint32_t)lk.w;
          if constexpr (CWQ_FOLD_ROUND0) {
            p0 = cwq::philox_round0_product(
                ng, (uint64_t)(uint32_t)lk.x | ((uint64_t)(uint32_t)lk.y << 32));
          } else {
            p0 = (uint64_t)kPhiloxM0 * ((ng + (uint32_t)mt.x) + w0g_x);
          }
        } else {
          mt = meta[kp];
          p0 = (uint64_t)kPhiloxM0 * ((ng + (uint32_t)mt.x) + w0g_x);
        }
        // the key through an opaque move each iteration: the fourteen round
        // keys are then formed here by scalar adds, not held in SGPRs across
        // the loop, where they pushed the loop's lane masks and counters out
        // into VGPR lanes (v_writelane / v_readlane every iteration).  Today's
        // loop has room for them (without the copy every instance still builds
        // at 106 SGPRs with no lane move in its loops, the keys formed once
        // per pass), but it is no faster for the 17 scalar instructions less:
        // C4 the same in the one-copy loop and 3.8 ms slower in the unrolled
        // one, at equal clock and VALU count.  The copy stays.
        uint32_t pk0 = st.k0, pk1 = st.k1;
        asm volatile("" : "+s"(pk0), "+s"(pk1));
        const U4 x = philox10_lo_p0(p0, lok, pk0, pk1);
        float z0, z1, z2, z3;
        float upper;
        if constexpr (SCREEN) {
          box_muller_screen(x.x, x.y, z0, z1);
          box_muller_screen(x.z, x.w, z2, z3);
          const float a0 = __builtin_fmaf(sa.x, z0, sb.x);
          const float a1 = __builtin_fmaf(sa.y, z1, sb.y);
          const float a2 = __builtin_fmaf(sa.z, z2, sb.z);
          const float a3 = __builtin_fmaf(sa.w, z3, sb.w);
          s = __builtin_fmaf(-a0, a0, s);
          s = __builtin_fmaf(-a1, a1, s);
          s = __builtin_fmaf(-a2, a2, s);
          s = __builtin_fmaf(-a3, a3, s);
          upper = screen_row_upper(s, kScreenC1, u2f((uint32_t)mt.y));
        } else {
          box_muller_dev(x.x, x.y, logtab, z0, z1);
          box_muller_dev(x.z, x.w, logtab, z2, z3);
          const float4* cq = cst + kp * NF;
          const float4 ls = cq[0], ss = cq[1], mu = cq[2], sg = cq[3], cc = cq[4], ry = cq[5];
          const float4 bb = STEP0 ? float4{0.f, 0.f, 0.f, 0.f} : cq[6];
          const float d0 = cand_diff<STEP0>(z0, ls.x, ss.x, mu.x, bb.x);
          const float d1 = cand_diff<STEP0>(z1, ls.y, ss.y, mu.y, bb.y);
          const float d2 = cand_diff<STEP0>(z2, ls.z, ss.z, mu.z, bb.z);
          const float d3 = cand_diff<STEP0>(z3, ls.w, ss.w, mu.w, bb.w);
          // fast correctly rounded quotients; lanes whose operands leave the
          // Markstein ranges (never, for sane inputs) redo them with IEEE division
          // inside a wave-uniform branch, so the common path issues no fallback.
          float y0 = div_rn_markstein(d0, sg.x, ry.x);
          float y1 = div_rn_markstein(d1, sg.y, ry.y);
          float y2 = div_rn_markstein(d2, sg.z, ry.z);
          float y3 = div_rn_markstein(d3, sg.w, ry.w);
          const bool ok = fastdiv & markstein_ok4(d0, d1, d2, d3);
          if (__builtin_expect(__ballot(!ok) != 0ull, 0)) {
            if (!ok) {
              y0 = d0 / sg.x;
              y1 = d1 / sg.y;
              y2 = d2 / sg.z;
              y3 = d3 / sg.w;
            }
          }
          s = s + lp_from_z(y0, cc.x);
          s = s + lp_from_z(y1, cc.y);
          s = s + lp_from_z(y2, cc.z);
          s = s + lp_from_z(y3, cc.w);
          upper = (s + __builtin_fabsf(s) * kPruneC1) + u2f((uint32_t)mt.y);
        }
        // the screening pass follows the records' links (the last one's is 0:
        // the completion test), the exact pass counts
        if constexpr (LINKED)
          kp = kp_next;
        else
          kp += KS;
        // (PARKED: the last position links to the sentinel and no lane tests
        // for it here; see "Parked rows" below)
        const bool complete =
            PARKED ? false : (LINKED ? (kp == 0u) : (kp == kb + KS * (uint32_t)G));
        const bool below = upper < tau;
        // Screening pass: one compare of (upper, tau) serves the drop test and
        // the keep test, !(upper < tau) == (upper >= tau), because neither is
        // NaN there.  upper = fma(s, c1, B_k): behind the gate sa and sb are
        // finite with |sa|, |sb| < 2^51 (screen_dim: mag / sigma <= 2^50), z'
        // is finite with |z'| < 5 for every Philox word (u1 is clamped to
        // [1e-7, 1], sin and cos take an angle in [1, 2)), so |a| < 2^54 and s,
        // a sum of at most 64 terms -a^2, is finite; B_k is finite or +inf,
        // never NaN (round_up_f32).  tau starts at -inf, at a clamped key's
        // value or at tau_g (tau_guess_of: never NaN) and only ever takes a
        // max with a lower bound that is not NaN
        // (tau_raise_wave leaves a NaN out) or with the workgroup's cell, which
        // holds such values only.  The exact pass, whose s may be NaN, keeps
        // both compares: a NaN row is neither dropped early nor kept.
        const bool reach = SCREEN ? !below : (upper >= tau);
#ifdef CWQ_PRUNE_STATS
        // (PARKED: the stats build keeps a completion compare of its own, true
        // in the iteration in which the row leaves its last real position)
        const bool complete_st =
            PARKED ? (kp == kb + KS * (uint32_t)G && kp_was != kb + KS * (uint32_t)G) : complete;
        const bool prune = !complete_st && below;
        const uint32_t k = (LINKED && complete_st) ? (uint32_t)G : (kp - kb) / KS;
#endif
        const bool done = complete || below || !active;
        // the finished lanes' mask from the compares' own masks (SALU).  The
        // empty asm keeps it here, in the compares' block: moved behind the
        // branch below, each ballot is rebuilt there with a v_cndmask + v_cmp.
        // The keep mask (complete, active, reaching tau) is formed the same
        // way, for the same reason: as the ballot of a bool it cost a second
        // compare of (upper, tau), a v_cndmask and a v_cmp every iteration.
        const uint64_t m_cpl = __builtin_amdgcn_ballot_w64(complete);
        const uint64_t m_below = __builtin_amdgcn_fcmpf(upper, tau, 4 /* olt */);
        // (FAST: every lane is active)
        uint64_t m = m_cpl | m_below;
        if constexpr (!FAST) m |= __builtin_amdgcn_read_exec() & ~m_act;
        uint64_t m_keep =
            m_cpl & (FAST ? ~0ull : m_act) &
            (SCREEN ? ~m_below : (uint64_t)__builtin_amdgcn_fcmpf(upper, tau, 3 /* oge */));
        // (A copy of the unrolled PARKED loop with no look has no branch
        // between the compares and the step, so nothing to pin: without the
        // asm it loses the s_nop behind it; PARKED never reads m_keep, which
        // through the asm cost a move of 0 into a scalar pair.)
        constexpr bool LOOK_HERE =
            PARKED && (C + 1u == UU || (LOOK_MASK + 1u <= UU && ((C + 1u) & LOOK_MASK) == 0u));
        if constexpr (!PARKED)
          asm volatile("" : "+s"(m), "+s"(m_keep));
        else if constexpr (!FAST || LOOK_HERE)
          asm volatile("" : "+s"(m));
        // Rows that completed and may be the best.  The branch is taken by the
        // whole wave (on the scalar m_keep, so the exec mask stays full for the
        // wave max): tau is raised to the largest lower end among these rows in
        // every lane at once, and of these rows only those whose upper end
        // reaches the raised tau go to the survivor list.
        //   * tau stays a lower bound of the exact value of a row completed in
        //     this tile: each `lower` is one (screening bound / kPruneC1).
        //   * A row with upper < tau has an exact value <= upper < tau <= the
        //     exact value of a completed row: neither the argmax nor a tie.
        //   * A row whose exact value E equals the best row's has upper >= E >=
        //     every lower bound of every row, so upper >= tau: ties reach the
        //     list, the best row among them, whatever the order of completion.
        //   * Exact pass: keep is false for a row with a NaN upper (reach is the
        //     ordered compare), so it is neither dropped above nor pushed here; a
        //     NaN lower (s = +inf) is left out of the max and the row, whose
        //     upper is +inf, is pushed.
        //
        // Parked rows (PARKED).  The loop has no completion test: a row that
        // passes its last real position without falling below tau there (the
        // ordinary test, with the full row's B) walks on to the sentinel and
        // stays there, active, with its s and ng unchanged, its upper end +inf
        // and so never below.  Every (CWQ_PARK_LOOK_MASK + 1)-th iteration,
        // which with the mask of the tau share is the one that shares tau
        // (the unrolled loop's last copy), compares kp with the sentinel's offset:
        // the lanes at it that are active and did not just drop are the
        // completed rows not yet seen (a lane that dropped at its last real
        // position has kp there too and is in m_below: it is finished the
        // ordinary way).  They take this same keep step, each exactly once,
        // and are ORed into that iteration's done mask, so the step and the
        // resets below move them on.  A wave cannot leave the loop with a row
        // parked, since a parked lane is active, and the pass's final share
        // comes after the loop, so after the last of these steps.  With tau
        // raised up to CWQ_PARK_LOOK_MASK iterations later than before:
        //   * tau is still only raised to lower ends of rows completed in this
        //     tile, later: it stays a lower bound of such a row's exact value;
        //   * a row is dropped on upper < tau at a real position only, as
        //     before, against a tau that is at most what it was before there;
        //   * a row whose exact value equals the best row's has upper >= every
        //     tau of the pass, so it is dropped nowhere, parks, and is pushed
        //     when found, whichever tau the wave has by then;
        //   * which rows are pushed may differ (a later push meets a higher
        //     tau); the survivors' exact values, and so the result, do not.
        // A parked lane idles for at most CWQ_PARK_LOOK_MASK iterations, over
        // both loops: the unrolled one leaves iter a multiple of its trip.
        auto keep_rows = [&](const uint64_t mk) {
          // (going down, `active` is carried as the scalar m_act alone: the
          // lane's bit of mk is complete && active && reach)
          const bool keep = CWQ_BORROW_REFILL ? ((mk >> lane) & 1ull) != 0ull
                                              : (complete && active && reach);
          float lower;
          if constexpr (SCREEN)
            lower = screen_row_lower(s, kScreenC2, sA, sPq);
          else
            lower = (s - __builtin_fabsf(s) * kPruneC1) - lc;
          // PARKED: the completed row's upper end (the loop's is the
          // sentinel's +inf by now), from the full row's B in meta (through an
          // opaque index: read here, not held across the loop) and the row's
          // s, which nothing has touched since its last unit: the value the
          // loop formed there
          if constexpr (PARKED) {
            uint32_t kf = (uint32_t)G - 1u;
            asm volatile("" : "+v"(kf));
            upper = screen_row_upper(s, kScreenC1, u2f((uint32_t)meta[kf].y));
          }
          tau = tau_raise_wave(tau, keep, lower);
          if (__builtin_expect(keep && upper >= tau, 0)) {
            // the row, n = (w0g + ng) / G (exact: n * G < 2^32), from an opaque
            // copy of ng, so that w0g + ng is not shared with the loop's grp,
            // and w0g from the wave's cell, not from a register held across
            // the loop
            uint32_t ngc = ng;
            asm volatile("" : "+v"(ngc));
            const uint32_t n =
                (*const_cast<const volatile uint32_t*>(&w0g_cell[wv]) + ngc) / (uint32_t)G;
#ifdef CWQ_PRUNE_STATS
            atomicAdd(&s_ps[66], 1u);
#endif
            const uint32_t slot = atomicAdd(&sq_cnt, 1u);
            if (slot < CWQ_SURVIVOR_CAP) {
              sq_n[slot] = (uint32_t)n;
              sq_ub[slot] = upper;
            } else if constexpr (FORM != 1) {  // list full (near-ties everywhere): evaluate exactly now
              // (FORM 1: sq_cnt has passed the cap, which defers the tile)
#ifdef CWQ_PRUNE_STATS
              atomicAdd(&g_prune_stats[69], 1ull);
#endif
              const float v = eval_row<D, STEP0>(st, (uint64_t)n * D, D, 0, loc_s + off,
                                                 scale_s + off, t_loc + off, t_scale + off,
                                                 lognorm + off, STEP0 ? nullptr : best + off, logtab);
              const uint64_t kv = argmax_key(v, (uint32_t)n);
              bestk = kv > bestk ? kv : bestk;
            }
          }
        };
        if constexpr (!PARKED) {
          if (__builtin_expect(m_keep != 0ull, 0)) keep_rows(m_keep);
        } else {
          // the share first, so that the parked rows meet the freshest tau
          if (share_due) tau = tau_share_wave(&tau_cell, tau);
          if (cwq::unroll_due<LOOK_MASK, UU, C>(iter)) {
            const uint64_t m_park = __builtin_amdgcn_uicmp(kp, kb + KS * (uint32_t)G, 32 /* eq */) &
                                    (FAST ? ~0ull : m_act) & ~m_below;
            if (__builtin_expect(m_park != 0ull, 0)) keep_rows(m_park);
            m |= m_park;
          }
        }
#ifdef CWQ_PRUNE_STATS
        const bool act_l = ((m_act >> lane) & 1ull) != 0ull;
        if (act_l && (complete_st || prune)) atomicAdd(&s_ps[k], 1u);
        if (act_l && complete_st) atomicAdd(&s_ps[65], 1u);
#endif
        uint64_t m_pool;
        if constexpr (CWQ_BORROW_REFILL) {
          // a finished lane steps down to its next static row: one subtract
          // and two moves with the exec mask set to the finished lanes (full
          // on entry, as everywhere in this loop).  Written out, because the
          // subtract's borrow is wanted as a scalar pair: it marks the lanes
          // that were on their last static row.  Only the finished lanes'
          // bits of it are used (the first s_and_b64).  `left` and m_pool are
          // formed here too: left as C++ ORs and ANDs, the chain was moved to
          // the VALU (two v_or, two v_and, a 64-bit v_cmp, two v_readfirstlane).
          // The exec mask is full here, so it is set back to -1, not saved.
          asm volatile(
              "s_mov_b64 exec, %[m]\n\t"
              "v_subrev_co_u32 %[ng], vcc, %[c], %[ng]\n\t"
              "v_mov_b32 %[kp], %[kb]\n\t"
              "v_mov_b32 %[s], 0\n\t"
              "s_mov_b64 exec, -1\n\t"
              "s_and_b64 %[mp], vcc, %[m]\n\t"
              "s_or_b64 %[left], %[left], %[mp]\n\t"
              "s_and_b64 %[mp], %[left], %[m]"
              : [ng] "+v"(ng), [kp] "+v"(kp), [s] "+v"(s), [mp] "=&s"(m_pool),
                [left] "+s"(left)
              : [m] "s"(m), [c] "n"(64 * G), [kb] "s"(kb)
              : "vcc", "scc");
          // the compiler takes a scalar output of a statement that also has
          // vector outputs for a per-lane value once it crosses a block (a
          // 64-bit v_cmp for the branch below, the masks in VGPRs);
          // readfirstlane tells it otherwise and folds to a scalar copy
          left = sgpr_pair_uniform(left);
          m_pool = sgpr_pair_uniform(m_pool);
        } else {
          // a finished lane steps to its next static row.  The empty asm keeps
          // this a branch on the exec mask (one add and two moves under it):
          // turned into selects it is an add and three v_cndmask for all lanes
          if (done) {
            asm volatile("" : "+v"(ng));
            ng += 64u * (uint32_t)G;
            kp = kb;
            s = 0.0f;
          }
          m_pool = 0ull;
        }
        // share tau across the workgroup's waves: it is wave-uniform already,
        // so one returning LDS max by lane 0 and one v_max, no reduce (and no
        // "raised since the last share" flag: both of its arms would be this)
        // (PARKED: shared above, with the look for parked rows)
        if (!PARKED && share_due) {
          tau = tau_share_wave(&tau_cell, tau);
        }
        // Pool refill, taken by the whole wave when a finished lane has left
        // its static rows (or was in the pool, or inactive): those lanes take
        // pool rows by rank, and the range test, which only a pool row can
        // fail, is taken here.  Lanes still on a row keep their ng: static
        // rows are below ng_stat <= ng_end, pool rows in progress passed the
        // test when they were handed out, inactive lanes are all finished
        // lanes (and in `left`: a lane becomes inactive on a pool row, or
        // starts so when S = 0), so the compare gives every lane's `active`
        // anew.  wnext_g is kept at or below ng_end (rows from there on are
        // out of range alike), which bounds ng however long lanes stay inactive.
        if constexpr (CWQ_BORROW_REFILL) {
          // (FAST: the refill out of line, so that a copy falls through to the next)
          if (FAST ? __builtin_expect(m_pool != 0ull, 0) : (m_pool != 0ull)) {
#ifdef CWQ_PRUNE_STATS
            if (lane == 0) atomicAdd(&s_ps[70], 1u);
#endif
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
                (uint32_t)(m_pool >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_pool, 0u));
            // ng = wnext_g + rank G in the lanes of m_pool, the others' kept:
            // one mad under that exec mask (rank <= 63 and G <= 16: 24-bit
            // factors), instead of a mad for all lanes and a select
            asm volatile(
                "s_mov_b64 exec, %[mp]\n\t"
                "v_mad_u32_u24 %[ng], %[rank], %[g], %[wn]\n\t"
                "s_mov_b64 exec, -1"
                : [ng] "+v"(ng)
                : [mp] "s"(m_pool), [rank] "v"(rank), [g] "n"(G), [wn] "s"(wnext_g));
            // the rows handed out are wnext_g .. want - G: all in range when
            // want <= ng_end, and then the lanes of m_pool are active and the
            // other lanes' state is what it was (no compare)
            const uint32_t want = wnext_g + (uint32_t)__builtin_popcountll(m_pool) * (uint32_t)G;
            if constexpr (FAST) {
              // want <= ng_end by the loop's entry test: the rows are in range
              // and every lane stays active, so m_act is not touched
              wnext_g = want;
            } else if (CWQ_POOL_RANGE_SKIP && want <= ng_end) {
              wnext_g = want;
              m_act |= m_pool;
            } else {
              wnext_g = want < ng_end ? want : ng_end;
              m_act = __builtin_amdgcn_uicmp(ng, ng_end, 36 /* ult */);
            }
          }
        } else {
          m_pool = m & __builtin_amdgcn_uicmp(ng, ng_stat, 35 /* uge */);
          if (m_pool != 0ull) {
#ifdef CWQ_PRUNE_STATS
            if (lane == 0) atomicAdd(&s_ps[70], 1u);
#endif
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
                (uint32_t)(m_pool >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_pool, 0u));
            if (done && ng >= ng_stat) ng = wnext_g + rank * (uint32_t)G;
            wnext_g += (uint32_t)__builtin_popcountll(m_pool) * (uint32_t)G;
            wnext_g = wnext_g < ng_end ? wnext_g : ng_end;
            active = ng < ng_end;
            m_act = __builtin_amdgcn_ballot_w64(active);
          }
        }
      };
      constexpr std::integral_constant<uint32_t, 0u> c0{};
      constexpr std::integral_constant<uint32_t, 1u> u1{};
      // The unrolled loop: U copies of the body per trip and no exit but at
      // the trip's end.  It runs while every lane is active and the pool holds
      // the 64 U rows that U refills can take at most, so that inside a trip
      //   * every pool row handed out is in range (want <= ng_end),
      //   * no lane turns inactive: m_act stays all ones and is not read,
      //   * and the wave cannot run out of rows, so no copy tests for it.
      // It leaves on a trip boundary, with iter a multiple of the trip, and in
      // the state the one-copy loop below expects, which hands out the rest
      // and is the whole pass of a wave with a small share (below 4,096 rows
      // at U = 8) or without a row.
      if constexpr (U > 1u) {
        while (m_act == ~0ull && wnext_g + cwq::unroll_trip_rows(U) * (uint32_t)G <= ng_end)
          unroll_each(body, std::make_integer_sequence<uint32_t, U>{});
      }
      // (Leaving this loop from the refill that clears the last bit of m_act,
      // with no test at its end, was built and measured: C4 -1.2 ms alone,
      // -0.2 ms behind the unrolled loop, neither five times the parent's
      // spread: not kept)
      while (m_act != 0ull) body(c0, u1);
    };
#ifdef CWQ_PRUNE_STATS
    if (screen && tid == 0) atomicAdd(&g_prune_stats[67], 1ull);
#endif
    // The pass, and once more with the guess off where the guess did not hold
    // (one loop around the one inlined screening pass; the branch is taken by
    // the whole workgroup on values read from LDS, made scalar).
    //
    // The guess held iff tau_final > tau_g or seed >= tau_g.  Then tau_final
    // is a lower bound of a real row's exact value (a completed row of this
    // tile, or the row behind keys[g]): only such bounds and tau_g enter the
    // maxima that make it, and it exceeds tau_g (or the seed alone is one).
    // Every drop of the pass was taken against a tau <= tau_final (tau only
    // rises, and the final share puts every wave's tau into the cell), so a
    // dropped row's exact value is below that of a real row: it is neither
    // the argmax nor a tie.  A row whose exact value equals the best row's
    // has upper >= that value >= tau_final >= every tau of the pass, so it
    // was kept and its upper end reaches tau_final below.  If the guess did
    // not hold, rows may have been dropped against a tau no real row backs:
    // the survivor list and the cell are reset to the seed and the pass runs
    // again from there, as it would have without a guess.  bestk keeps the
    // exact keys it has (list-full rows): they belong to real rows.
    float tau_final;
    if (screen) {
      for (;;) {
        pass(std::true_type{});
        tau_share_wave(&tau_cell, tau);
        __syncthreads();
        tau_final = tau_cell;
        const float tg = tau_guess_of(qm_cell, sA, sPq);
        const float seed = INTER ? tau_seed_cell : -__builtin_inff();
        const bool held = tau_final > tg || seed >= tg;
        if (__builtin_amdgcn_readfirstlane(held ? 1 : 0) != 0) break;
        __syncthreads();  // every thread has read the cells
        if (tid == 0) {
          tau_cell = seed;
          sq_cnt = 0u;
          qm_cell = cwq::kTauNoGuess;
#ifdef CWQ_PRUNE_STATS
          atomicAdd(&g_prune_stats[51], 1ull);
#endif
        }
        __syncthreads();
        tau = (INTER && CWQ_TAU_FROM_KEYS) ? seed : -__builtin_inff();
      }
    } else if constexpr (FORM == 1) {  // gate failed: the tile is deferred (below)
      tau_final = tau;
    } else {  // the exact pass takes no guess (qm_cell: kTauNoGuess)
      pass(std::false_type{});
      tau_share_wave(&tau_cell, tau);
      __syncthreads();
      tau_final = tau_cell;
    }
    if constexpr (FORM == 1) {
      // The rows that reach tau_final into the block's slots, their number
      // into its count word; with more than Q of them, a list past its cap or
      // no screening pass, count 0 and the block onto the deferred list.  The
      // slots' order is the order of arrival: k_score_survivors takes a max.
      // (sq_cnt and screen are the workgroup's: the branches are uniform.)
      const uint32_t pushed = sq_cnt;
      const bool listed = screen && pushed <= (uint32_t)CWQ_SURVIVOR_CAP;
      const uint32_t qmax = df.q > 0 ? (uint32_t)df.q : 0u;  // <= kDeferSlots (launch_prune_t)
      if (tid == 0) dq_cnt = 0u;
      __syncthreads();
      if (listed) {
        for (uint32_t i = tid; i < pushed; i += 256u) {
          if (sq_ub[i] >= tau_final) {
            const uint32_t slot = atomicAdd(&dq_cnt, 1u);
            if (slot < qmax) df.surv[cwq::defer_slot(g, (int)slot)] = sq_n[i];
          }
        }
      }
      __syncthreads();
      if (tid == 0) {
        const uint32_t c = dq_cnt;
        const bool deferred = !listed || c > qmax;
        df.count[g] = deferred ? 0u : cwq::defer_count_word(c, (int)qmax);
        if (deferred) {  // (a block is listed once, so the slot is below nb: the test guards the store)
          const uint32_t at = atomicAdd(df.dcount, 1u);
          if ((int64_t)at < ntiles_arg) df.list[at] = (uint32_t)g;
        }
      }
      __syncthreads();
    } else {
      // exact evaluation of the survivors that can still reach the final tau
      const uint32_t nsurv = sq_cnt < CWQ_SURVIVOR_CAP ? sq_cnt : CWQ_SURVIVOR_CAP;
      // A wave takes the list 64 entries at a time, packs those that reach
      // tau_final to the front of its 64 (in place: every lane has read its
      // entry before any writes) and scores them RW rows per pass, a lane per
      // Philox block (score_rows_wave).  All of it is wave-uniform.  The lane
      // comes from the tile's opaque tid, so that the rows' per-lane addresses
      // are not hoisted out of the tile loop and spilled.
      const uint32_t nsurv_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)nsurv);
      const uint32_t sl = tid & 63u;
      for (uint32_t c0 = wv * 64u; c0 < nsurv_u; c0 += 256u) {
        const uint32_t i = c0 + sl;
        const bool q = i < nsurv_u && sq_ub[i] >= tau_final;
        const uint32_t nn = i < nsurv_u ? sq_n[i] : 0u;
        const uint64_t qm = __builtin_amdgcn_ballot_w64(q);
        if (qm == 0ull) continue;
#ifdef CWQ_PRUNE_STATS
        if (q) atomicAdd(&g_prune_stats[68], 1ull);
#endif
        const uint32_t qr = __builtin_amdgcn_mbcnt_hi((uint32_t)(qm >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)qm, 0u));
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (q) sq_n[c0 + qr] = nn;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t qn = (uint32_t)__builtin_popcountll(qm);
        for (uint32_t b = 0; b < qn; b += (uint32_t)RW) {
          const uint32_t cnt = qn - b < (uint32_t)RW ? qn - b : (uint32_t)RW;
          const float v = score_rows_wave<D, STEP0>(
              st, sq_n + c0 + b, cnt, loc_s + off, scale_s + off, t_loc + off, t_scale + off,
              lognorm + off, STEP0 ? nullptr : best + off, logtab, rowbuf[wv], sl);
          if ((sl & 7u) == 0u && (sl >> 3) < cnt) {
            const uint64_t kv = argmax_key(v, sq_n[c0 + b + (sl >> 3)]);
            bestk = kv > bestk ? kv : bestk;
          }
        }
      }

      bestk = wave_max_u64(bestk);
      if (lane == 0) wkey[wv] = bestk;
      __syncthreads();
      if (tid == 0) {
        uint64_t mk = wkey[0];
        for (int i = 1; i < 4; ++i) mk = wkey[i] > mk ? wkey[i] : mk;
        if (mk) atomicMax(&keys[g], (unsigned long long)mk);
#ifdef CWQ_PRUNE_STATS
        if (!g_seed_tau && g < kDbgBlocks) g_dbg_best[g] = mk;
#endif
#ifdef CWQ_TILE_TIMES
        if (tile < kTileTimes) g_tile_t1[tile] = __builtin_amdgcn_s_memrealtime();
#endif
      }
    }  // FORM != 1
#ifdef CWQ_PRUNE_STATS
    if (tid < 72) {
      if (s_ps[tid]) atomicAdd(&g_prune_stats[tid], (unsigned long long)s_ps[tid]);
      s_ps[tid] = 0u;
    }
#endif
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// The rows k_encode_prune's screening-only form listed (FORM 1), scored
// exactly: eval_row<D, STEP0>'s value bit for bit (score_block_terms and
// score_fold8 are score_rows_wave's halves), folded into keys[g] by atomicMax.
//
// A wave takes RW = min(64 / G, 8) consecutive blocks, the first row of each in
// one pass: lane l computes Philox block l % G of block l / G's row, with that
// block's stream and constants, and lanes 8 r .. 8 r + 7 sum block r's terms
// (eight lanes per row in the fold, hence at most 8 rows; at d <= 24 the lanes
// past 8 G idle).  Rows past a block's first go in further passes, over the
// slot index, as long as any block of the wave has one: the loop is uniform.
// A count word is at most kDeferSlots (k_encode_prune writes min(c, Q) or 0);
// it is clamped here all the same, so that the slots read stay the block's.
// ---------------------------------------------------------------------------
// The one-word counters of a scoring launch, zeroed before it: the deferred
// list's length and the tile queue's next tile (either may be null).  And the
// argmax keys of a step after the first.  Launches, not memsets: the encode
// sequence is kernels only, so that a captured call holds no memset node
// between its kernel nodes: replays of such nodes did not write the zeros
// that were captured (DESIGN.md 4 "Graph replay").
__global__ void k_counters_reset(uint32_t* __restrict__ dcount, uint32_t* __restrict__ tq) {
  if (threadIdx.x == 0) {
    if (dcount) *dcount = 0u;
    if (tq) *tq = 0u;
  }
}

__global__ void __launch_bounds__(256) k_keys_reset(unsigned long long* __restrict__ keys,
                                                    int64_t nb) {
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < nb;
       g += (int64_t)gridDim.x * blockDim.x)
    keys[g] = 0ull;
}

template <int D, bool STEP0>
__global__ void __launch_bounds__(256) k_score_survivors(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const float* __restrict__ best, int64_t nb, SeedSpec sd,
    int32_t step, const uint32_t* __restrict__ surv, const uint32_t* __restrict__ count,
    unsigned long long* __restrict__ keys) {
  constexpr uint32_t G = D / 4;
  constexpr uint32_t RW = (64 / G) < 8 ? (64 / G) : 8;
  __shared__ double logtab[32];
  __shared__ float rowbuf[4][RW * D];
  fill_logtab(logtab);
  const uint32_t wv = wave_id();
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t g0 = ((int64_t)blockIdx.x * 4 + wv) * RW;
  // the lane's block as a term lane (r, u) and as a fold lane (fr)
  const uint32_t r = lane / G, u = lane - r * G, fr = lane >> 3;
  const int64_t g = g0 + r, gf = g0 + fr;
  const bool term_lane = r < RW && g < nb, fold_lane = fr < RW && gf < nb;
  uint32_t cnt = term_lane ? count[g] : 0u, cntf = fold_lane ? count[gf] : 0u;
  cnt = cnt < (uint32_t)cwq::kDeferSlots ? cnt : (uint32_t)cwq::kDeferSlots;
  cntf = cntf < (uint32_t)cwq::kDeferSlots ? cntf : (uint32_t)cwq::kDeferSlots;
  if (__builtin_amdgcn_ballot_w64(cnt != 0u) == 0ull) return;  // (uniform)
  PhiloxStream st{};
  if (cnt != 0u) st = generate_key(step_seed(sd.of(g), step), 42);
  const int64_t off = g * D;
  for (uint32_t q = 0; q < (uint32_t)cwq::kDeferSlots; ++q) {
    if (__builtin_amdgcn_ballot_w64(q < cnt) == 0ull) break;  // (uniform)
    if (q < cnt)
      score_block_terms<D, STEP0>(st, surv[cwq::defer_slot(g, (int)q)], u, loc_s + off,
                                  scale_s + off, t_loc + off, t_scale + off, lognorm + off,
                                  STEP0 ? nullptr : best + off, logtab, rowbuf[wv] + r * D);
    const float v = score_fold8<D>(rowbuf[wv], lane, q < cntf);
    if ((lane & 7u) == 0u && q < cntf) {
      const uint64_t kv = argmax_key(v, surv[cwq::defer_slot(gf, (int)q)]);
      if (kv) atomicMax(&keys[gf], (unsigned long long)kv);
    }
  }
}

// ---------------------------------------------------------------------------
// General pruned encoder: any block dimension, CSR or uniform (the greedy
// coder's ragged groups, coded_greedy_sampler.py:207-284).  Same screening
// bound as k_encode_prune (DESIGN.md "screening bound"), with three changes:
//   * dims are visited in natural order (a candidate row starts at any word of
//     a Philox block: each lane walks its row one Philox block at a time);
//   * the per-dim constants live in global memory, computed once per step by
//     k_csr_prep (one workgroup per block), with the float-summation factors
//     of the bound scaled for the block's d (gamma_d = 1.01 (d+1) 2^-24);
//   * tiles of one block share their threshold through gtau[g].
// Blocks whose constants fail the gate are scored exactly.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// Visit order.  A row starting at flat normal k0 = n*d has alignment class
// c = k0 & 3; its Philox blocks ("units") u = 0..U_c-1, U_c = (d + c + 3) / 4,
// hold dims 4u - c + t (t = word 0..3, kept if 0 <= dim < d).  Per block and
// class, k_csr_prep sorts the units by expected a^2 (most informative first,
// so rows cross tau early) and stores for visit position k the unit ord[k] and
// the drop bound bpre[k] (units visited before position k).  Region of block g:
// off + 12 g, class c at c * csr_cls_stride(d), csr_cls_stride(d) =
// (d + 6) / 4 + 1 >= U_c + 1; 4 strides <= d + 10 entries.
__host__ __device__ __forceinline__ int64_t csr_cls_stride(int64_t d) { return (d + 6) / 4 + 1; }
constexpr int64_t kCsrSortUnits = 2048;  // sorted if U_3 <= this (d <= 8189); else natural order

// Per block: the per-dim constants and sums, then for each alignment class
// its sorted visit order and drop bounds.  Each dim's constants are computed
// once (double arithmetic) into sab (sA, sB) and cdim (C_j) in global memory,
// where the class passes read them back; the prep workgroup keeps a small LDS
// footprint, so it can start on a CU that the other streams' scoring kernels
// occupy.  With few blocks the four classes go to four workgroups
// (blockIdx.y), each computing the block's constants and sums (identical
// values, so their stores to sab / cdim agree), so the sorts run side by
// side; the blockIdx.y == 0 workgroup also writes sab's zero pads and the
// block's gate constants.  Sums and the drop-bound prefix sums are wave
// reductions / scans (a few barriers per block); classes of <= 256 units are
// ordered by a rank sort (one barrier), longer ones by a bitonic sort.
// Blocks longer than lds_dims (whose constants the scoring kernel reads from
// global memory, not LDS) also get abp: for visit position k of class c the
// (sa, sb) of unit ord[k]'s four words in one 32-byte record, so the scoring
// lanes of a slot read consecutive records instead of gathering.
template <bool STEP0>
__global__ void __launch_bounds__(256) k_csr_prep(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const float* __restrict__ best,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t nb, float2* __restrict__ sab,
    float* __restrict__ cdim, float* __restrict__ bpre, uint32_t* __restrict__ ordu,
    float4* __restrict__ grp, uint32_t* __restrict__ gtau, float4* __restrict__ abp,
    int64_t lds_dims, int64_t coop_min_d) {
  __shared__ double red[5][4];
  __shared__ double wscan[4];
  __shared__ double ucs[256];  // classes of <= 256 units: unit u's C sum
  __shared__ unsigned long long skey[kCsrSortUnits];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  // gridDim.y == 4: one class per workgroup (few blocks: the four sorts run
  // side by side); gridDim.y == 1: one workgroup walks all four classes (many
  // blocks: the per-dim constants are computed once per block, not per class)
  const bool lead = blockIdx.y == 0;  // writes the block's class-independent outputs
  for (int64_t g = blockIdx.x; g < nb; g += gridDim.x) {
    const BlockSpan sp = block_span(block_off, ud, g);
    const int64_t off = sp.off, d = sp.d;
    ScreenSums u;  // this thread's dims (sum C is taken per visit position below)
    float2* sabg = sab + off + 8 * g + 4;  // 4 zero pads either side (partial units)
    float* cg = cdim + off;
    if (lead && tid < 8) {  // 8 trailing zeros: the last 4 are the next block's
      if (tid < 4) sabg[tid - 4] = float2{0.f, 0.f};  // leading pads (or the slack
      sabg[d + tid] = float2{0.f, 0.f};               // past the last block)
    }
    for (int64_t j = tid; j < d; j += 256) {
      const ScreenDim o =
          screen_dim<STEP0>(loc_s[off + j], scale_s[off + j], t_loc[off + j], t_scale[off + j],
                            lognorm[off + j], STEP0 ? 0.0f : best[off + j]);
      sabg[j] = float2{o.sa, o.sb};
      cg[j] = o.C;
      u.add(o);
    }
    u.sm = wave_sum_f64(u.sm);
    u.sa = wave_sum_f64(u.sa);
    u.sk = wave_sum_f64(u.sk);
    u.s2 = wave_sum_f64(u.s2);
    u.mx = wave_max_f64(u.mx);
    if (lane == 0) {
      red[0][wv] = u.sm;
      red[1][wv] = u.sa;
      red[2][wv] = u.sk;
      red[3][wv] = u.s2;
      red[4][wv] = u.mx;
    }
    // the sab / cdim stores are read back below by other threads: wait for
    // them to complete (they write through to L2) and read them with
    // agent-scope loads, which bypass the CU's L1 (a line another block's
    // workgroup on this CU filled earlier may hold this block's previous-step
    // values at its edges)
    __threadfence_block();
    const bool all_ok = __syncthreads_and(u.ok) != 0;
    ScreenSums S;  // the block's
    S.sm = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    S.sa = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    S.sk = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    S.s2 = ((red[3][0] + red[3][1]) + red[3][2]) + red[3][3];
    S.mx = red[4][0];
    for (int w = 1; w < 4; ++w) S.mx = red[4][w] > S.mx ? red[4][w] : S.mx;
    // depth of the screening sum: cooperative rows 16 + d/64, per-lane rows d
    const bool coop_blk = d >= coop_min_d;
    const ScreenBlock bc =
        screen_block_consts(S, d, coop_blk ? 16.0 + (double)d / 64.0 : (double)d);
    const double SM = S.sm, sl = bc.sl;
    const int64_t reg = off + 12 * g, cs = csr_cls_stride(d);
    const bool recs = abp != nullptr && d > lds_dims;
    auto sab_at = [&](int64_t j) {
      const unsigned long long v = __hip_atomic_load(
          reinterpret_cast<unsigned long long*>(sabg + j), __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_AGENT);
      return float2{u2f((uint32_t)v), u2f((uint32_t)(v >> 32))};
    };
    for (int c = (int)blockIdx.y; c < 4; c += (int)gridDim.y) {
      // word t of unit u of class c is dim 4u - c + t (absent outside [0, d));
      // unit u: its sum of C_j and its expected sum of a_j^2 - C_j
      auto unit = [&](int64_t u, double& csum, double& gain) {
        csum = 0.0;
        gain = 0.0;
        for (int t = 0; t < 4; ++t) {
          const int64_t j = 4 * u - c + t;
          if (j >= 0 && j < d) {
            const float2 ab = sab_at(j);
            const float xc = u2f(__hip_atomic_load(reinterpret_cast<uint32_t*>(cg + j),
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            csum += (double)xc;
            gain += (double)ab.x * (double)ab.x * (0.5 / 0.6931471805599453) +
                    (double)ab.y * (double)ab.y - (double)xc;
          }
        }
      };
      auto key_of = [&](int64_t u) {
        double cu, gu;
        unit(u, cu, gu);
        const float gf = (float)(gu > 0.0 ? gu : 0.0);
        return ((unsigned long long)ord_f32(gf) << 32) | (0xffffffffull - (uint64_t)u);
      };
      const int64_t U = (d + c + 3) / 4;
      const bool sorted = all_ok && U <= kCsrSortUnits;
      const bool small = U <= 256;  // one unit per thread: its C sum kept in LDS
      if (sorted && small) {  // rank sort of (gain desc, u asc) keys: keys are distinct
        unsigned long long key = 0ull;
        if (tid < U) {
          double cu, gu;
          unit(tid, cu, gu);
          ucs[tid] = cu;
          const float gf = (float)(gu > 0.0 ? gu : 0.0);
          key = ((unsigned long long)ord_f32(gf) << 32) | (0xffffffffull - (uint64_t)tid);
          skey[tid] = key;
        }
        __syncthreads();
        int r = 0;
        if (tid < U)
          for (int i = 0; i < (int)U; ++i) r += skey[i] > key ? 1 : 0;
        __syncthreads();
        if (tid < U) skey[r] = key;
        __syncthreads();
      } else if (sorted) {  // bitonic sort of (gain desc, u asc) keys
        int64_t P = 1;
        while (P < U) P <<= 1;
        for (int64_t u = tid; u < P; u += 256) skey[u] = u < U ? key_of(u) : 0ull;
        __syncthreads();
        for (int64_t k = 2; k <= P; k <<= 1) {
          for (int64_t jj = k >> 1; jj > 0; jj >>= 1) {
            for (int64_t i = tid; i < P; i += 256) {
              const int64_t l = i ^ jj;
              if (l > i) {
                const unsigned long long x = skey[i], y = skey[l];
                const bool desc = (i & k) == 0;  // overall descending
                if (desc ? (x < y) : (x > y)) {
                  skey[i] = y;
                  skey[l] = x;
                }
              }
            }
            __syncthreads();
          }
        }
      }
      // drop bounds along the visit order, positions k = 0..U
      double carry = 0.0;
      for (int64_t base = 0; base <= U; base += 256) {
        const int64_t k = base + tid;
        int64_t u = k;
        if (sorted && k < U) u = (int64_t)(0xffffffffull - (skey[k] & 0xffffffffull));
        double cu = 0.0, gu;
        if (all_ok && k < U) {
          if (sorted && small)
            cu = ucs[u];
          else
            unit(u, cu, gu);
        }
        if (recs && k <= U) {  // the unit's four (sa, sb), zero for absent words
          float e[8];          // (position U: the zero record of the pad unit)
          for (int t = 0; t < 4; ++t) {
            const int64_t j = 4 * u - c + t;
            float2 ab = float2{0.f, 0.f};
            if (k < U && j >= 0 && j < d) ab = sab_at(j);
            e[2 * t] = ab.x;
            e[2 * t + 1] = ab.y;
          }
          float4* rr = abp + 2 * (csr_rec_base(off) + c * cs + k);
          rr[0] = float4{e[0], e[1], e[2], e[3]};
          rr[1] = float4{e[4], e[5], e[6], e[7]};
        }
        double v = cu;  // inclusive scan: in the wave, then across the four waves
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const double t = __shfl_up(v, (unsigned)o, 64);
          if (lane >= o) v += t;
        }
        if (lane == 63) wscan[wv] = v;
        __syncthreads();
        double pre = 0.0;
        for (int w = 0; w < wv; ++w) pre += wscan[w];
        const double total = ((wscan[0] + wscan[1]) + wscan[2]) + wscan[3];
        const double excl = carry + (pre + v) - cu;
        if (k <= U) {
          bpre[reg + c * cs + k] = round_up_f32(SM + excl * (1.0 + 0x1p-20) + sl);
          // position U: the pad unit U, whose words all fall on zero constants
          // (sab's and the scoring kernel's LDS pads), so a unit read past a
          // row's end scores exactly 0 without a mask
          ordu[reg + c * cs + k] = (uint32_t)(k < U ? u : U);
        }
        carry += total;
        __syncthreads();
      }
    }
    if (lead && tid == 0) {  // the gate does not look at the full-row B (bpre holds the B_k)
      grp[g] = (all_ok && bc.finite && d > 0) ? float4{bc.c1, bc.c2, bc.as, bc.pq}
                                              : float4{0.f, 0.f, 0.f, 0.f};
      gtau[g * CWQ_CSR_GTAU_STRIDE] = ord_f32(-__builtin_inff());
    }
    __syncthreads();
  }
}

// One candidate row evaluated exactly by a whole wave (the survivors of the
// general pruned kernel; d is large there, so one lane per row would leave the
// other 63 idle for a full row).  Lanes compute the terms of up to 63 Philox
// blocks per 248-dim chunk into LDS; lanes 0-7 then fold them into the eight
// Eigen accumulators and lane 8 into the tail, in exactly eval_row_f's order.
// Every lane returns the row value.
constexpr int kRowChunk = 248;  // multiple of 8; spans <= 63 Philox blocks

template <bool STEP0>
__device__ __forceinline__ float exact_row_wave(
    const PhiloxStream& st, uint64_t kbase, int64_t d, const float* __restrict__ loc_s,
    const float* __restrict__ scale_s, const float* __restrict__ mu,
    const float* __restrict__ sg, const float* __restrict__ lognorm,
    const float* __restrict__ best, const double* logtab, float* buf, uint32_t lane) {
  const int64_t vec = d & ~(int64_t)7;
  float acc = 0.0f;  // lane l < 8: p[l]; lane 8: the tail sum
  for (int64_t j0 = 0; j0 < d; j0 += kRowChunk) {
    const int64_t cnt = (d - j0) < kRowChunk ? d - j0 : kRowChunk;
    const uint64_t k0 = kbase + (uint64_t)j0;
    const uint64_t blk = (k0 >> 2) + lane;
    const int64_t ef = (int64_t)(blk << 2) - (int64_t)k0;  // chunk index of the block's word 0
    if (ef < cnt) {
      const F4 z = normal4_dev(st, blk, logtab);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int64_t e = ef + t;
        if (e >= 0 && e < cnt) {
          const int64_t j = j0 + e;
          const float zz = t == 0 ? z.a : (t == 1 ? z.b : (t == 2 ? z.c : z.d));
          float v = scale_s[j] * zz;  // misc.py:14
          v = loc_s[j] + v;           // misc.py:15
          const float tv = STEP0 ? v : best[j] + v;
          buf[e] = log_prob(tv, mu[j], sg[j], lognorm[j]);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < 8) {
      for (int64_t e = lane; e < cnt && j0 + e < vec; e += 8) acc = acc + buf[e];
    } else if (lane == 8) {
      for (int64_t e = (vec > j0 ? vec - j0 : 0); e < cnt; ++e) acc = acc + buf[e];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  float p[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) p[l] = __shfl(acc, l, 64);
  return eigen_fold8(p, __shfl(acc, 8, 64));
}

// ---------------------------------------------------------------------------
// Encoder, one step, a wave per candidate row: long blocks at few candidates
// (per-group bit budgets), where a lane per row leaves most of
// the chip idle.  Row r = g * n_cand + n of the flattened (block, candidate)
// list goes to wave r mod W of the grid's W waves; every row is scored exactly
// by exact_row_wave (k_encode_eval's values bit for bit, no screening), the
// four keys of a workgroup's iteration are folded through LDS and each block
// they touch gets one atomicMax.  An empty block gets no key: keys[g] stays 0
// and k_encode_finalize writes index 0, as after k_encode_eval.
// ---------------------------------------------------------------------------
template <bool STEP0>
__global__ void __launch_bounds__(256) k_encode_rows_wave(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const float* __restrict__ best,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t nb, int n_bits, SeedSpec sd,
    int32_t step, unsigned long long* __restrict__ keys) {
  __shared__ double logtab[32];
  __shared__ float rowbuf[4][kRowChunk];
  __shared__ unsigned long long wkey[4];
  __shared__ int64_t wblk[4];
  fill_logtab(logtab);
  const uint32_t wv = wave_id();
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t rows = nb << n_bits;
  const int64_t cmask = ((int64_t)1 << n_bits) - 1;
  // the loop is uniform over the workgroup (its barriers) and a wave skips a
  // row as a whole: exact_row_wave runs with all 64 lanes or not at all
  for (int64_t r0 = 4 * (int64_t)blockIdx.x; r0 < rows; r0 += 4 * (int64_t)gridDim.x) {
    const int64_t r = r0 + wv;
    uint64_t k = 0;
    int64_t g = -1;
    if (r < rows) {
      g = r >> n_bits;
      const int64_t n = r & cmask;
      const BlockSpan sp = block_span(block_off, ud, g);
      if (sp.d > 0) {
        const PhiloxStream st = generate_key(step_seed(sd.of(g), step), 42);
        const float v = exact_row_wave<STEP0>(
            st, (uint64_t)n * (uint64_t)sp.d, sp.d, loc_s + sp.off, scale_s + sp.off,
            t_loc + sp.off, t_scale + sp.off, lognorm + sp.off,
            STEP0 ? nullptr : best + sp.off, logtab, rowbuf[wv], lane);
        k = argmax_key(v, (uint32_t)n);
      }
    }
    if (lane == 0) {
      wkey[wv] = k;
      wblk[wv] = g;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      // wave i's key, folded with those of the later waves on the same block;
      // the first wave of each block sends it
      const int i = (int)threadIdx.x;
      uint64_t m = wkey[i];
      bool first = true;
      for (int j = 0; j < 4; ++j) {
        if (j == i || wblk[j] != wblk[i]) continue;
        if (j < i) first = false;
        m = wkey[j] > m ? wkey[j] : m;
      }
      if (first && m) atomicMax(&keys[wblk[i]], (unsigned long long)m);
    }
    __syncthreads();
  }
}

#ifndef CWQ_CSR_GTAU_SHARE
#define CWQ_CSR_GTAU_SHARE 1  // 1: also share tau with the block's other tiles in the loop
#endif
#ifndef CWQ_CSR_GTAU_MASK
#define CWQ_CSR_GTAU_MASK 63u  // ... every CWQ_CSR_GTAU_MASK + 1 iterations
#endif
#ifndef CWQ_CSR_SURVIVOR_CAP
#define CWQ_CSR_SURVIVOR_CAP 512
#endif
#ifndef CWQ_CSR_TILE
#define CWQ_CSR_TILE 1024             // smallest tile (candidates), per-lane rows
#endif
#ifndef CWQ_CSR_TILES
#define CWQ_CSR_TILES 8192            // tiles a launch aims for
#endif
#ifndef CWQ_CSR_COOP_TILE
#define CWQ_CSR_COOP_TILE 128         // smallest tile (candidates) in cooperative launches
#endif
#ifndef CWQ_CSR_COOP_TILES
#define CWQ_CSR_COOP_TILES 6144       // tiles a cooperative launch aims for (4 x 1536 slots)
#endif
#ifndef CWQ_CSR_COOP_CLASS_WAVES
#define CWQ_CSR_COOP_CLASS_WAVES 1    // 1: cooperative rows n = wave (mod 4) per wave
#endif
#ifndef CWQ_CSR_COOP_MIN_WAVES
#define CWQ_CSR_COOP_MIN_WAVES 4      // waves/SIMD the cooperative kernel's registers allow
#endif
#ifndef CWQ_CSR_RUN_MIN_WAVES
#define CWQ_CSR_RUN_MIN_WAVES 6       // waves/SIMD the per-lane kernel's registers allow
#endif
#ifndef CWQ_RUN_UPL
#define CWQ_RUN_UPL 2                 // units per lane per iteration of a per-lane row
#endif
#ifndef CWQ_COOP_UPL
#define CWQ_COOP_UPL 4                // units per lane per iteration of a cooperative row
#endif
#ifndef CWQ_COOP_CLASS_TILES
#define CWQ_COOP_CLASS_TILES 1        // 1: cooperative tiles hold one alignment class (rows n = R mod 4)
#endif
#ifndef CWQ_COOP_LOAD_ORDER
#define CWQ_COOP_LOAD_ORDER 0         // 1: a cooperative iteration's loads issued in unit order
#endif

// element idx of base through an unsigned 32-bit byte offset (base + voffset)
template <class T>
__device__ __forceinline__ T ld_u32off(const T* base, uint32_t idx) {
  return *(const T*)((const char*)base + (uint64_t)(idx * (uint32_t)sizeof(T)));
}

static_assert(CWQ_CSR_COOP_MIN_D <= CWQ_CSR_LDS_DIMS, "short rows of a cooperative launch use LDS");

// COOP: the kernel of cooperative launches (few long rows; blocks of at least
// coop_min_d dims walked by 16-lane slots, shorter ones per lane from LDS);
// otherwise one row per lane for every block.
template <bool STEP0, bool COOP>
__global__ void __launch_bounds__(256, COOP ? CWQ_CSR_COOP_MIN_WAVES : CWQ_CSR_RUN_MIN_WAVES) k_encode_prune_csr(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const float* __restrict__ best,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t ntiles, int64_t tiles_per_block,
    int64_t cand_per_tile, int64_t n_cand, SeedSpec sd, int32_t step,
    const float2* __restrict__ sab, const float* __restrict__ bpre,
    const uint32_t* __restrict__ ordu, const float4* __restrict__ grp,
    uint32_t* __restrict__ gtau, unsigned long long* __restrict__ keys, int64_t coop_min_d,
    const float4* __restrict__ abp) {
  __shared__ double logtab[32];
  __shared__ uint32_t tau_ord;
  __shared__ uint32_t sq_cnt;
  __shared__ uint32_t sq_n[CWQ_CSR_SURVIVOR_CAP];
  __shared__ float sq_ub[CWQ_CSR_SURVIVOR_CAP];
  __shared__ unsigned long long wkey[4];
  // One LDS region, two uses that never overlap in time: a short block's
  // natural-order constants, drop bounds and visit order (l_ab, l_bp, l_ord),
  // and the survivors' exact-row buffers (rowbuf, after the loops).
  constexpr int kNatF4 = (CWQ_CSR_LDS_DIMS + 12) * 2 / 4;   // l_ab in float4s
  constexpr int kIdxF4 = (CWQ_CSR_LDS_DIMS + 12) / 4;       // l_bp, l_ord
  static_assert((CWQ_CSR_LDS_DIMS + 12) % 4 == 0, "LDS sub-arrays in whole float4s");
  constexpr int kUnionF4 = kNatF4 + 2 * kIdxF4;
  static_assert(kUnionF4 * 4 >= 4 * kRowChunk, "rowbuf fits the region");
  __shared__ float4 l_u[kUnionF4];
  float2* const l_ab = reinterpret_cast<float2*>(l_u);
  float* const l_bp = reinterpret_cast<float*>(l_u + kNatF4);
  uint32_t* const l_ord = reinterpret_cast<uint32_t*>(l_u + kNatF4 + kIdxF4);
  float(*const rowbuf)[kRowChunk] = reinterpret_cast<float(*)[kRowChunk]>(l_u);
  fill_logtab(logtab);
  const uint32_t wv = wave_id();
  const uint32_t lane = threadIdx.x & 63u;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    // tile-major order: a block's later tiles start after its first ones have
    // published their threshold in gtau (the loop shares tau inside the
    // workgroup only: per-iteration global atomics cost more than they prune)
    const int64_t nbk = ntiles / tiles_per_block;
    const int64_t tt = tile / nbk;
    const int64_t g = tile - tt * nbk;
    const BlockSpan sp = block_span(block_off, ud, g);
    const int64_t off = sp.off, d = sp.d;
    // the tile's rows: n0 + rstep m, m < nrt
    int64_t n0, nrt;
    uint32_t rlog = 0;  // log2 rstep
#if CWQ_COOP_CLASS_TILES && CWQ_CSR_COOP_CLASS_WAVES
    if (COOP && d >= coop_min_d && (tiles_per_block & 3) == 0) {
      // one alignment class per workgroup: tile tt takes the rows n = R (mod 4)
      // of chunk J (4 tiles' worth of candidates), R = tt mod 4, J = tt / 4, so
      // its four waves read one class's visit-order records, not four
      const int64_t J = tt >> 2, C4 = 4 * cand_per_tile;
      const int64_t lim = (J + 1) * C4 < n_cand ? (J + 1) * C4 : n_cand;
      n0 = J * C4 + (tt & 3);
      nrt = lim > n0 ? (lim - n0 + 3) / 4 : 0;
      rlog = 2;
    } else
#endif
    {
      n0 = tt * cand_per_tile;
      nrt = ((n0 + cand_per_tile < n_cand) ? n0 + cand_per_tile : n_cand) - n0;
    }
    if (nrt <= 0) continue;  // empty tile
    const int64_t n1 = n0 + nrt;  // contiguous tiles (rlog == 0): the rows' end
    const PhiloxStream st =
        generate_key(step_seed(sd.of(g), step), 42);
    const float4 gc = grp[g];
    const bool in_lds = d <= CWQ_CSR_LDS_DIMS;
    const int64_t reg = off + 12 * g, cs = csr_cls_stride(d);
    if (gc.x != 0.0f && in_lds) {
      // 4 zero pads before, 8 after (the pad unit U's words reach d + 7 + 4)
      for (int64_t j = tid; j < d + 12; j += blockDim.x)
        l_ab[j] = j < d + 8 ? sab[off + 8 * g + j] : float2{0.f, 0.f};
      for (int64_t j = tid; j < 4 * cs; j += blockDim.x) {
        l_bp[j] = bpre[reg + j];
        l_ord[j] = ordu[reg + j];
      }
    }
    if (tid == 0) {
      tau_ord = __hip_atomic_load(&gtau[g * CWQ_CSR_GTAU_STRIDE], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);  // earlier tiles of the block
      sq_cnt = 0u;
    }
    __syncthreads();
    uint64_t bestk = 0;
#ifdef CWQ_PRUNE_STATS
    if (tid == 0) atomicAdd(&g_prune_stats[gc.x != 0.0f ? 40 : 41], 1ull);
#endif
    bool exact_tile = gc.x == 0.0f;
    if (!exact_tile) {
      const int64_t per_wave = (n1 - n0 + 3) / 4;
      const int64_t w0 = n0 + (int64_t)wv * per_wave;
      const int64_t w1 = (w0 + per_wave < n1) ? w0 + per_wave : n1;
      // lane state: row n0 + r (class c, first Philox block rb, U units), visit
      // position k.  ab is the padded constant array: entry 4 + j for dim j,
      // zeros for the out-of-row words of a row's first and last unit.
      const uint32_t r0 = (uint32_t)(w0 - n0), r1 = (uint32_t)(w1 - n0);
      const int d32 = (int)d;
      // ab: natural-order (sa, sb) (LDS or global); rec (REC true): the
      // visit-order records of k_csr_prep's abp, read at the lane's position
      // Past-the-end positions read the pad unit's zero constants (LDS, sab or
      // records: k_csr_prep), so their units add exactly 0 without a mask.
      // HI0: every Philox block index of the launch is below 2^32 (counter
      // word 1 is 0, which makes round 2's first product lane-invariant).
      auto run = [&](const float2* ab, const float* bp, const uint32_t* od, const float4* rec,
                     auto REC, auto HI0T) __attribute__((always_inline)) {
        constexpr bool HI0 = decltype(HI0T)::value;
        [[maybe_unused]] const PhiloxLo lok = HI0 ? philox_lo_key(st) : PhiloxLo{};
        uint32_t wnext = r0 + 64u;
        uint32_t r = r0 + lane;
        bool active = r < r1;
        float s = 0.0f;
        float tau = unord_f32(tau_ord);
        uint32_t iter = 0;
        uint64_t rb;
        int c, U, cb;
        auto start_row = [&]() __attribute__((always_inline)) {
          const uint64_t k0 = (uint64_t)(n0 + (int64_t)r) * (uint64_t)d;
          rb = k0 >> 2;
          c = (int)(k0 & 3u);
          U = (d32 + c + 3) >> 2;
          cb = c * (int)cs;
        };
        start_row();
        int k = 0;
        // RUPL units per iteration (positions k .. k + RUPL - 1; a unit past
        // the row end adds exactly 0: its a is forced to 0).  The units of the
        // next positions are loaded one iteration ahead (the Philox counter
        // needs them first thing: a load at the top of the iteration would
        // expose its latency every time); a new row reloads.  Loads index
        // their uniform base with an unsigned 32-bit byte offset.
        constexpr int RUPL = COOP ? 1 : CWQ_RUN_UPL;  // the cooperative kernel: short rows only
        uint32_t u_nx[RUPL];
        auto load_units = [&](int p0) __attribute__((always_inline)) {
#pragma unroll
          for (int i = 0; i < RUPL; ++i) {
            const int pp = p0 + i;
            u_nx[i] = ld_u32off(od, (uint32_t)(cb + (pp < U ? pp : U)));
          }
        };
        load_units(0);
        while (__ballot(active) != 0ull) {
          uint32_t u[RUPL];
#pragma unroll
          for (int i = 0; i < RUPL; ++i) u[i] = u_nx[i];
          load_units(k + RUPL);
          // this iteration's constants and the next drop bound are loaded
          // here, ahead of the opaque key move below, so their latency
          // overlaps the Philox rounds (the compiler otherwise issues them
          // after the transcendentals and waits on them at once)
          float2 e[RUPL][4];
#pragma unroll
          for (int i = 0; i < RUPL; ++i) {
            const int pp = k + i;
            if constexpr (decltype(REC)::value) {
              const uint32_t pc = (uint32_t)(cb + (pp < U ? pp : U));
              const float4 ra = ld_u32off(rec, 2u * pc), rb2 = ld_u32off(rec, 2u * pc + 1u);
              e[i][0] = float2{ra.x, ra.y};
              e[i][1] = float2{ra.z, ra.w};
              e[i][2] = float2{rb2.x, rb2.y};
              e[i][3] = float2{rb2.z, rb2.w};
            } else {
              const uint32_t jp = (uint32_t)(4 * (int)u[i] - c + 4);
              e[i][0] = ld_u32off(ab, jp);  // padded index of word 0
              e[i][1] = ld_u32off(ab, jp + 1u);
              e[i][2] = ld_u32off(ab, jp + 2u);
              e[i][3] = ld_u32off(ab, jp + 3u);
            }
          }
          const int kn = (k + RUPL < U) ? k + RUPL : U;
          const float bnext = ld_u32off(bp, (uint32_t)(cb + kn));
          // round keys recomputed in SALU each iteration (opaque key): keeping
          // all 20 live costs SGPRs the loop then spills into VGPR lanes
          uint32_t kk0 = st.k0, kk1 = st.k1;
          asm volatile("" : "+s"(kk0), "+s"(kk1));
#pragma unroll
          for (int i = 0; i < RUPL; ++i) {
            const uint64_t blk = rb + u[i];
            const U4 x = HI0 ? philox10_lo((uint32_t)blk, lok, kk0, kk1)
                             : philox10_dev((uint32_t)blk, (uint32_t)(blk >> 32), st.c2, st.c3,
                                            kk0, kk1);
            F4 z;
            box_muller_screen(x.x, x.y, z.a, z.b);
            box_muller_screen(x.z, x.w, z.c, z.d);
            const float a0 = __builtin_fmaf(e[i][0].x, z.a, e[i][0].y);
            const float a1 = __builtin_fmaf(e[i][1].x, z.b, e[i][1].y);
            const float a2 = __builtin_fmaf(e[i][2].x, z.c, e[i][2].y);
            const float a3 = __builtin_fmaf(e[i][3].x, z.d, e[i][3].y);
            s = __builtin_fmaf(-a0, a0, s);
            s = __builtin_fmaf(-a1, a1, s);
            s = __builtin_fmaf(-a2, a2, s);
            s = __builtin_fmaf(-a3, a3, s);
#ifdef CWQ_PRUNE_STATS
            if (active && (i == 0 || k + i < U)) atomicAdd(&g_prune_stats[43], 1ull);
#endif
          }
          k = kn;
          const bool complete = k == U;
          const float upper = screen_row_upper(s, gc.x, bnext);
          const bool prune = !complete && (upper < tau);
          if (complete && active && upper >= tau) {  // may be the best: keep it
            const float lower = screen_row_lower(s, gc.y, gc.z, gc.w);
            tau = fmaxf(tau, lower);
            const uint32_t slot = atomicAdd(&sq_cnt, 1u);
            if (slot < CWQ_CSR_SURVIVOR_CAP) {  // else: overflow, the tile is redone
              sq_n[slot] = r;
              sq_ub[slot] = upper;
            }
          }
          const bool done = complete || prune || !active;
#ifdef CWQ_PRUNE_STATS
          if (active && (complete || prune)) atomicAdd(&g_prune_stats[42], 1ull);
          if (active && complete) atomicAdd(&g_prune_stats[44], 1ull);
          if (active && complete && upper >= tau) atomicAdd(&g_prune_stats[45], 1ull);
          atomicAdd(&g_prune_stats[48], 1ull);
#endif
          const uint64_t m = __ballot(done);
          const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
              (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
          if (done) {
            r = wnext + rank;
            start_row();
            k = 0;
            s = 0.0f;
            load_units(0);
          }
          wnext += (uint32_t)__builtin_popcountll(m);
          active = r < r1;
          if (((++iter) & CWQ_CSR_TAU_SHARE_MASK) == 0u) {  // share with the workgroup
            const float tm = wave_max_f32(tau);
            if (lane == 0) atomicMax(&tau_ord, ord_f32(tm));
            uint32_t o = __atomic_load_n(&tau_ord, __ATOMIC_RELAXED);
#if CWQ_CSR_GTAU_SHARE
            if ((iter & CWQ_CSR_GTAU_MASK) == 0u) {
              // publish only an improvement (atomics are rare once tau settles),
              // read the block's threshold every time
              uint32_t* gt = &gtau[g * CWQ_CSR_GTAU_STRIDE];
              const uint32_t o2 = __hip_atomic_load(gt, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
              if (lane == 0 && ord_f32(tm) > o2) atomicMax(gt, ord_f32(tm));
              o = o > o2 ? o : o2;
            }
#endif
            tau = fmaxf(tau, unord_f32(o));
          }
        }
        const float tm = wave_max_f32(tau);
        if (lane == 0) atomicMax(&tau_ord, ord_f32(tm));
      };
      // Cooperative rows (long rows, few rows per lane): each 16-lane DPP row
      // ("slot") walks one candidate row, lane t taking visit position k + t,
      // 16 units per iteration.  The partial sums are added over the slot with
      // a symmetric butterfly (row16_sum_f32), so s, the drop test and the
      // refill are uniform within the slot; the drop test runs every 16 units.
      // The bound's float-summation factor is taken at this tree's depth
      // (k_csr_prep: 4 in-lane + 4 butterfly + one per chunk).
      auto run_coop = [&](const float2* ab, const float* bp, const uint32_t* od,
                          const float4* rec, auto REC, auto HI0T) __attribute__((always_inline)) {
        constexpr bool HI0 = decltype(HI0T)::value;
        [[maybe_unused]] const PhiloxLo lok = HI0 ? philox_lo_key(st) : PhiloxLo{};
        const uint32_t t = lane & 15u, slot = lane >> 4;
        const uint64_t below = (1ull << (slot * 16u)) - 1ull;  // lanes of lower slots
#if CWQ_CSR_COOP_CLASS_WAVES
        // wave wv walks rows wv, wv + 4, wv + 8, ... of the tile: one alignment
        // class per wave, so its slots share one class's visit order
        const uint32_t nrows = (uint32_t)nrt;
        const uint32_t q0 = 0u, q1 = nrows > wv ? (nrows - wv + 3u) / 4u : 0u;
        auto row_of = [&](uint32_t q) { return (wv + 4u * q) << rlog; };
#else
        const uint32_t q0 = r0, q1 = r1;
        auto row_of = [&](uint32_t q) { return q; };
#endif
        uint32_t wnext = q0 + 4u;
        uint32_t q = q0 + slot;
        bool active = q < q1;
        uint32_t r = row_of(q);
        float s = 0.0f;
        float tau = unord_f32(tau_ord);
        uint32_t iter = 0;
        uint64_t rb;
        int c, U, cb;
        auto start_row = [&]() __attribute__((always_inline)) {
          const uint64_t k0 = (uint64_t)(n0 + (int64_t)r) * (uint64_t)d;
          rb = k0 >> 2;
          c = (int)(k0 & 3u);
          U = (d32 + c + 3) >> 2;
          cb = c * (int)cs;
        };
        start_row();
        int k = 0;
        // lane t takes visit positions k + t + 16 i, i < UPL: a slot advances
        // CH = 16 UPL units per iteration.  The units of the next positions
        // are loaded one iteration ahead, as in run.
        constexpr int UPL = CWQ_COOP_UPL, CH = 16 * UPL;
        // Loads index their (uniform) base with an unsigned 32-bit byte offset,
        // so they address as base + voffset: no 64-bit address arithmetic in
        // the loop.  Offsets stay far below 2^32 (a block's region holds
        // d + 10 entries of at most 32 bytes).
        uint32_t u_nx[UPL];
        auto load_units = [&](int p0) __attribute__((always_inline)) {
#pragma unroll
          for (int i = 0; i < UPL; ++i) {
            const int pp = p0 + 16 * i;
            u_nx[i] = ld_u32off(od, (uint32_t)cb + (uint32_t)(pp < U ? pp : U));
          }
        };
        load_units((int)t);
        while (__ballot(active) != 0ull) {
          const int p = k + (int)t;
          float part = 0.0f;
          uint32_t u[UPL];
#pragma unroll
          for (int i = 0; i < UPL; ++i) u[i] = u_nx[i];
          load_units(p + CH);
          // constants and the slot's next drop bound ahead of the Philox
          // rounds, as in run (positions past U clamp to U, the pad unit)
          const int kn = (k + CH < U) ? k + CH : U;
          const float bnext = ld_u32off(bp, (uint32_t)(cb + kn));
          float2 e[UPL][4];
#pragma unroll
          for (int i = 0; i < UPL; ++i) {
            const int pp = p + 16 * i;
            if constexpr (decltype(REC)::value) {
              const uint32_t pc = (uint32_t)(cb + (pp < U ? pp : U));
              const float4 ra = ld_u32off(rec, 2u * pc), rb2 = ld_u32off(rec, 2u * pc + 1u);
              e[i][0] = float2{ra.x, ra.y};
              e[i][1] = float2{ra.z, ra.w};
              e[i][2] = float2{rb2.x, rb2.y};
              e[i][3] = float2{rb2.z, rb2.w};
            } else {
              const uint32_t jp = (uint32_t)(4 * (int)u[i] - c + 4);
              e[i][0] = ld_u32off(ab, jp);
              e[i][1] = ld_u32off(ab, jp + 1u);
              e[i][2] = ld_u32off(ab, jp + 2u);
              e[i][3] = ld_u32off(ab, jp + 3u);
            }
#if CWQ_COOP_LOAD_ORDER
            // issue unit i's loads before unit i + 1's: the first unit's
            // constants then arrive first (loads complete in order), so its
            // wait does not also cover the later units' loads
            asm volatile("" ::: "memory");
#endif
          }
          if (active && p < U) {
            uint32_t kk0 = st.k0, kk1 = st.k1;
            asm volatile("" : "+s"(kk0), "+s"(kk1));
            // the UPL units are independent chains (ILP); a unit past the row
            // end reads the pad unit's zero constants and adds exactly 0
#pragma unroll
            for (int i = 0; i < UPL; ++i) {
              const uint64_t blk = rb + u[i];
              const U4 x = HI0 ? philox10_lo((uint32_t)blk, lok, kk0, kk1)
                               : philox10_dev((uint32_t)blk, (uint32_t)(blk >> 32), st.c2,
                                              st.c3, kk0, kk1);
              F4 z;
              box_muller_screen(x.x, x.y, z.a, z.b);
              box_muller_screen(x.z, x.w, z.c, z.d);
              const float a0 = __builtin_fmaf(e[i][0].x, z.a, e[i][0].y);
              const float a1 = __builtin_fmaf(e[i][1].x, z.b, e[i][1].y);
              const float a2 = __builtin_fmaf(e[i][2].x, z.c, e[i][2].y);
              const float a3 = __builtin_fmaf(e[i][3].x, z.d, e[i][3].y);
              float pu = -(a0 * a0);
              pu = __builtin_fmaf(-a1, a1, pu);
              pu = __builtin_fmaf(-a2, a2, pu);
              pu = __builtin_fmaf(-a3, a3, pu);
              if (i == 0)
                part = pu;
              else
                part = part + pu;
            }
          }
#ifdef CWQ_PRUNE_STATS
#pragma unroll
          for (int i = 0; i < UPL; ++i)
            if (active && p + 16 * i < U) atomicAdd(&g_prune_stats[43], 1ull);
#endif
          s = s + row16_sum_f32(part);
          k = kn;
          const bool complete = k == U;
          const float upper = screen_row_upper(s, gc.x, bnext);
          const bool prune = !complete && (upper < tau);
          if (complete && active && upper >= tau) {  // may be the best: keep it
            const float lower = screen_row_lower(s, gc.y, gc.z, gc.w);
            tau = fmaxf(tau, lower);
            if (t == 0u) {
              const uint32_t sl = atomicAdd(&sq_cnt, 1u);
              if (sl < CWQ_CSR_SURVIVOR_CAP) {  // else: overflow, the tile is redone
                sq_n[sl] = r;
                sq_ub[sl] = upper;
              }
            }
          }
          const bool done = complete || prune || !active;
#ifdef CWQ_PRUNE_STATS
          if (t == 0u && active && (complete || prune)) atomicAdd(&g_prune_stats[42], 1ull);
          if (t == 0u && active && complete) atomicAdd(&g_prune_stats[44], 1ull);
          if (t == 0u && active && complete && upper >= tau) atomicAdd(&g_prune_stats[45], 1ull);
          atomicAdd(&g_prune_stats[48], 1ull);
#endif
          const uint64_t m = __ballot(done);  // 16 bits per finished slot
          if (done) {
            q = wnext + (uint32_t)(__builtin_popcountll(m & below) >> 4);
            r = row_of(q);
            start_row();
            k = 0;
            s = 0.0f;
            load_units((int)t);
          }
          wnext += (uint32_t)(__builtin_popcountll(m) >> 4);
          active = q < q1;
          if (((++iter) & CWQ_CSR_TAU_SHARE_MASK) == 0u) {  // share with the workgroup
            const float tm = wave_max_f32(tau);
            if (lane == 0) atomicMax(&tau_ord, ord_f32(tm));
            tau = fmaxf(tau, unord_f32(__atomic_load_n(&tau_ord, __ATOMIC_RELAXED)));
          }
        }
        const float tm = wave_max_f32(tau);
        if (lane == 0) atomicMax(&tau_ord, ord_f32(tm));
      };
      const bool coop = d >= coop_min_d;
      // the block's largest Philox block index, ((n_cand - 1) d + d - 1) / 4
      const bool lo32 = (uint64_t)n_cand * (uint64_t)d <= (1ull << 34);
      // survivor list overflow (near-ties everywhere, or a weak early tau):
      // redo the pass starting from the final tau, then score exactly
      for (int pass = 0;; ++pass) {
        using NoRec = std::integral_constant<int, 0>;
        using Rec = std::integral_constant<int, 1>;
        using Lo32 = std::integral_constant<bool, true>;   // block indices < 2^32
        using Hi32 = std::integral_constant<bool, false>;
        // each launch mode instantiates only its own loops (register
        // allocation is per kernel: the largest loop sets every loop's budget)
        auto any_run = [&](auto HI0T) __attribute__((always_inline)) {
          if constexpr (COOP) {
            if (coop) {
              if (in_lds)
                run_coop(l_ab, l_bp, l_ord, nullptr, NoRec{}, HI0T);
              else if (abp)
                run_coop(nullptr, bpre + reg, ordu + reg, abp + 2 * csr_rec_base(off), Rec{}, HI0T);
              else
                run_coop(sab + off + 8 * g, bpre + reg, ordu + reg, nullptr, NoRec{}, HI0T);
            } else {  // d < coop_min_d <= CWQ_CSR_LDS_DIMS: the constants are in LDS
              run(l_ab, l_bp, l_ord, nullptr, NoRec{}, HI0T);
            }
          } else if (in_lds)
            run(l_ab, l_bp, l_ord, nullptr, NoRec{}, HI0T);
          else if (abp)
            run(nullptr, bpre + reg, ordu + reg, abp + 2 * csr_rec_base(off), Rec{}, HI0T);
          else
            run(sab + off + 8 * g, bpre + reg, ordu + reg, nullptr, NoRec{}, HI0T);
        };
        if (lo32)
          any_run(Lo32{});
        else
          any_run(Hi32{});
        __syncthreads();
        if (tid == 0) {
          const uint32_t mine = tau_ord;
          const uint32_t prev = atomicMax(&gtau[g * CWQ_CSR_GTAU_STRIDE], mine);
          tau_ord = prev > mine ? prev : mine;
        }
        __syncthreads();
        if (sq_cnt <= CWQ_CSR_SURVIVOR_CAP) break;
#ifdef CWQ_PRUNE_STATS
        if (tid == 0) atomicAdd(&g_prune_stats[46], 1ull);
#endif
        if (pass == 1) {
          exact_tile = true;
          break;
        }
        __syncthreads();
        if (tid == 0) sq_cnt = 0u;
        __syncthreads();
      }
    }
    if (!exact_tile) {
      const float tau_final = unord_f32(tau_ord);
      const uint32_t nsurv = sq_cnt < CWQ_CSR_SURVIVOR_CAP ? sq_cnt : CWQ_CSR_SURVIVOR_CAP;
      for (uint32_t i = wv; i < nsurv; i += 4) {  // one survivor per wave
        if (sq_ub[i] >= tau_final) {
          const int64_t nn = n0 + (int64_t)sq_n[i];
#ifdef CWQ_PRUNE_STATS
          if (lane == 0) atomicAdd(&g_prune_stats[47], 1ull);
#endif
          const float v = exact_row_wave<STEP0>(
              st, (uint64_t)nn * (uint64_t)d, d, loc_s + off, scale_s + off, t_loc + off,
              t_scale + off, lognorm + off, STEP0 ? nullptr : best + off, logtab, rowbuf[wv],
              lane);
          const uint64_t kv = argmax_key(v, (uint32_t)nn);
          bestk = kv > bestk ? kv : bestk;
        }
      }
    } else {
      const int align = (int)(((uint64_t)(n0 + ((int64_t)wv << rlog)) * (uint64_t)d) & 3u);
      for (int64_t m = 4 * (int64_t)lane + wv; m < nrt; m += 256) {
        const int64_t n = n0 + (m << rlog);
        const float v = eval_row<0, STEP0>(st, (uint64_t)n * (uint64_t)d, d, align, loc_s + off,
                                           scale_s + off, t_loc + off, t_scale + off,
                                           lognorm + off, STEP0 ? nullptr : best + off, logtab);
        const uint64_t kv = argmax_key(v, (uint32_t)n);
        bestk = kv > bestk ? kv : bestk;
      }
    }
    bestk = wave_max_u64(bestk);
    if (lane == 0) wkey[wv] = bestk;
    __syncthreads();
    if (tid == 0) {
      uint64_t mk = wkey[0];
      for (int i = 1; i < 4; ++i) mk = wkey[i] > mk ? wkey[i] : mk;
      if (mk) atomicMax(&keys[g], (unsigned long long)mk);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Screened encoder for few candidates (64 <= 2^b < 4096, CSR or uniform d the
// fast kernel does not take): C2/C3's 8-bit groups of ~5 dims.  Every
// candidate is screened -- k_csr_prep's bound with the row summed
// sequentially in natural order, no pruning -- and only survivors are scored
// exactly, densely, in a separate pass:
//   k_small_prep      per block (a lane each for short blocks): per-dim (sA, sB)
//                     into sab, the block's (c1, c2, As, Pq) into grp (c1 == 0:
//                     the block is scored exactly), its full-row bound B and
//                     stream key into bpre[off + 12 g ...]; gtau = -inf; the
//                     survivor count = 0.
//   k_small_screen    a wave per tile, each lane 4 consecutive rows at a time
//                     (d whole Philox blocks): screened value s of each row; tau = the wave's
//                     best lower bound fma(s, c2, As) - Pq sqrt(-s); rows whose
//                     upper bound fma(s, c1, B) reaches tau take one of the
//                     block's CWQ_SLIST_PER_BLOCK slots; tau is published to
//                     gtau[g].  Full slots mark the block exact.
//   k_small_survivors listed rows still reaching gtau[g], scored exactly one
//                     per lane; then every candidate of the blocks marked exact.
// The exact pass costs about 3x a screened row (f64 Box-Muller against the
// hardware transcendentals); survivors are ~1 per block, so the step costs
// about a third of scoring every candidate exactly.
// ---------------------------------------------------------------------------
#ifndef CWQ_SMALL_SCREEN_WAVES
#define CWQ_SMALL_SCREEN_WAVES 8  // waves/SIMD k_small_screen's registers must allow
#endif

// A wave prepares 64 consecutive blocks: lane i block i when it has at most
// kSmallLaneD dims (C2's groups: ~5), sequentially; longer blocks afterwards
// with the whole wave, lanes over dims.  The block's stream key for this step
// (a Philox-10 call) is stored too, so the screening rows do not repeat it.
constexpr int64_t kSmallLaneD = 32;
// Per-block header of the small path, 12 words at bpre + 12 g (bpre holds
// total_dims + 12 nb words; a forked part's bpre moves by 12 g0): [0] the
// full-row bound B, [1..4] the step's stream key, [5..8] grp's (c1, c2, As, Pq),
// [9..10] the block's dim offset, [11] its dims.  The slot count is at
// scnt[12 g].
constexpr int64_t kSmallHdr = 12;
struct SmallHdr {
  float bf;
  PhiloxStream st;
  float4 gc;
  int64_t off;
  int d;
};
__device__ __forceinline__ SmallHdr small_hdr(const float4 h0, const float4 h1, const float4 h2) {
  SmallHdr h;
  h.bf = h0.x;
  h.st = PhiloxStream{f2u(h0.y), f2u(h0.z), f2u(h0.w), f2u(h1.x)};
  h.gc = float4{h1.y, h1.z, h1.w, h2.x};
  h.off = (int64_t)(((uint64_t)f2u(h2.z) << 32) | (uint64_t)f2u(h2.y));
  h.d = (int)f2u(h2.w);
  return h;
}

template <bool STEP0>
__global__ void __launch_bounds__(256) k_small_prep(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const float* __restrict__ best,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t nb, SeedSpec sd, int32_t step,
    float2* __restrict__ sab, float* __restrict__ bpre, float4* __restrict__ grp,
    uint32_t* __restrict__ gtau, uint32_t* __restrict__ scnt) {
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  auto dim = [&](ScreenSums& u, int64_t off, int64_t g, int64_t j) {
    const ScreenDim o = screen_dim<STEP0>(loc_s[off + j], scale_s[off + j], t_loc[off + j],
                                          t_scale[off + j], lognorm[off + j],
                                          STEP0 ? 0.0f : best[off + j]);
    sab[off + 8 * g + 4 + j] = float2{o.sa, o.sb};  // k_csr_prep's padded layout
    u.add(o);
  };
  auto finish = [&](const ScreenSums& u, int64_t off, int64_t g, int64_t d) {
    const ScreenBlock bc = screen_block_consts(u, d, (double)d);  // rows summed sequentially
    const float bf = bc.bf;
    const bool fin = bc.finite && bf - bf == 0.0f;
    const float4 gc = (u.ok && fin && d > 0) ? float4{bc.c1, bc.c2, bc.as, bc.pq}
                                             : float4{0.f, 0.f, 0.f, 0.f};
    grp[g] = gc;
    // the block's header (kSmallHdr), indexed by g alone: the screen reads it
    // with one load level and prefetches the next tile's
    const PhiloxStream st = generate_key(step_seed(sd.of(g), step), 42);
    float4* hg = reinterpret_cast<float4*>(bpre + kSmallHdr * g);
    hg[0] = float4{bf, u2f(st.k0), u2f(st.k1), u2f(st.c2)};
    hg[1] = float4{u2f(st.c3), gc.x, gc.y, gc.z};
    hg[2] = float4{gc.w, u2f((uint32_t)off), u2f((uint32_t)((uint64_t)off >> 32)), u2f((uint32_t)d)};
    scnt[kSmallHdr * g] = 0u;
    gtau[g * CWQ_CSR_GTAU_STRIDE] = ord_f32(-__builtin_inff());
  };
  for (int64_t gb = ((int64_t)blockIdx.x * 4 + wave_id()) * 64; gb < nb; gb += nwaves * 64) {
    const int64_t g = gb + lane;
    bool longb = false;
    if (g < nb) {
      const BlockSpan sp = block_span(block_off, ud, g);
      if (sp.d <= kSmallLaneD) {
        ScreenSums u;
        for (int64_t j = 0; j < sp.d; ++j) dim(u, sp.off, g, j);
        finish(u, sp.off, g, sp.d);
      } else {
        longb = true;
      }
    }
    for (uint64_t m = __ballot(longb); m != 0ull; m &= m - 1ull) {  // the long blocks, a wave each
      const int64_t gl = gb + (int64_t)__builtin_ctzll(m);
      const BlockSpan sp = block_span(block_off, ud, gl);
      ScreenSums u;
      for (int64_t j = lane; j < sp.d; j += 64) dim(u, sp.off, gl, j);
      const bool all_ok = __ballot(u.ok == 0) == 0ull;
      u.sm = wave_sum_f64(u.sm);
      u.sa = wave_sum_f64(u.sa);
      u.sk = wave_sum_f64(u.sk);
      u.s2 = wave_sum_f64(u.s2);
      u.cs = wave_sum_f64(u.cs);
      u.mx = wave_max_f64(u.mx);
      u.ok = all_ok ? 1 : 0;
      if (lane == 0) finish(u, sp.off, gl, sp.d);
    }
  }
}

template <bool STEP0>
__global__ void __launch_bounds__(256, CWQ_SMALL_SCREEN_WAVES) k_small_screen(
    const int64_t* __restrict__ block_off, int64_t ud, int64_t ntiles, int64_t tiles_per_block,
    int64_t cand_per_tile, int64_t n_cand, SeedSpec sd, int32_t step,
    const float2* __restrict__ sab, const float* __restrict__ bpre, float4* __restrict__ grp,
    uint32_t* __restrict__ gtau, uint32_t* __restrict__ scnt, uint2* __restrict__ slist) {
  const uint32_t lane0 = threadIdx.x & 63u;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  // a wave takes a whole tile (the block's header, key and threshold once per
  // tile), 256 rows per round.  The header (k_small_prep) is one load level.
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave_id(); tile < ntiles; tile += nwaves) {
    // the lane index behind an opaque move: the many span variants' lane-derived
    // values are then computed per tile instead of hoisted out of the tile loop
    // (and spilled)
    uint32_t lane = lane0;
    asm volatile("" : "+v"(lane));
    const int64_t g = tiles_per_block == 1 ? tile : tile / tiles_per_block;
    const int64_t tt = tile - g * tiles_per_block;
    const float4* hp = reinterpret_cast<const float4*>(bpre + kSmallHdr * g);
    const SmallHdr h = small_hdr(hp[0], hp[1], hp[2]);
    const float4 gc = h.gc;
    if (gc.x == 0.0f) continue;  // scored exactly by k_small_survivors
    const int64_t off = h.off;
    const int d = h.d;
    const int64_t n0 = tt * cand_per_tile;
    const int64_t n1 = (n0 + cand_per_tile < n_cand) ? n0 + cand_per_tile : n_cand;
    const float bf = h.bf;
    const PhiloxStream st = h.st;
    const float2* ab = sab + off + 8 * g + 4;
    // A block that is one tile (C2/C3's 256 candidates) belongs to this wave
    // alone: its threshold starts at k_small_prep's -inf and its slot count
    // lives in a scalar, both stored once at the end -- no global atomics.
    const bool own = tiles_per_block == 1;
    float tau = own ? -__builtin_inff()
                    : unord_f32(__hip_atomic_load(&gtau[g * CWQ_CSR_GTAU_STRIDE],
                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    uint32_t used = 0;  // own block: slots taken so far (wave-uniform)
    // lane span m: rows n0 + 4 (lane + 64 m) + q, q = 0..3.  n0 is a multiple
    // of 4 (tiles are multiples of 256 candidates), so a span's 4d words are
    // exactly Philox blocks [n d / 4, n d / 4 + d): every block is computed
    // once (a row alone would start and end inside blocks its neighbours also
    // compute), and the dim index of each word is the same in every lane, so
    // the per-dim constants are wave-uniform loads.
    const PhiloxLo K = philox_lo_key(st);
    // tau, survivor slots of one span's four rows (rs: their screened values)
    auto span_tail = [&](int64_t ns, const float (&rs)[4]) __attribute__((always_inline)) {
      uint64_t m[4];
      const uint32_t cnt = span_vote(rs, ns, n1, gc.x, gc.y, gc.z, gc.w, bf, tau, m);
      if (cnt) {
        // the block's slots: this wave's scalar count, or a global counter
        // shared with the block's other tiles
        uint32_t base = used;
        if (own) {
          used += cnt;
        } else {
          if (lane == 0) base = atomicAdd(&scnt[kSmallHdr * g], cnt);
          base = (uint32_t)__shfl((int)base, 0, 64);
        }
        uint32_t pre = base;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const uint64_t mq = m[qq];
          if ((mq >> lane) & 1ull) {
            const uint32_t slot = pre + __builtin_amdgcn_mbcnt_hi(
                                            (uint32_t)(mq >> 32),
                                            __builtin_amdgcn_mbcnt_lo((uint32_t)mq, 0u));
            if (slot < CWQ_SLIST_PER_BLOCK)
              slist[CWQ_SLIST_PER_BLOCK * g + slot] =
                  uint2{(uint32_t)(ns + qq), f2u(screen_row_upper(rs[qq], gc.x, bf))};
          }
          pre += (uint32_t)__builtin_popcountll(mq);
        }
        if (base + cnt > CWQ_SLIST_PER_BLOCK && lane == 0)  // slots full: score the block exactly
          __hip_atomic_store(reinterpret_cast<uint32_t*>(&grp[g].x), 0u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      }
    };
    auto spans = [&](auto lo_tag) __attribute__((always_inline)) {
      constexpr bool LO = decltype(lo_tag)::value;  // every Philox block index < 2^32
      for (int64_t m0 = 0; n0 + 256 * m0 < n1; ++m0) {
        const int64_t ns = n0 + 4 * ((int64_t)lane + 64 * m0);
        const uint64_t b0 = (uint64_t)ns * (uint64_t)d / 4u;
        float rs[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // the span's four row sums
        float cur = 0.0f;  // natural order, sequential sum (h = d), as k_small_prep's bound
        int j = 0, q = 0;
        for (int b = 0; b < d; ++b) {
          const uint64_t blk = b0 + (uint64_t)b;
          const U4 x = LO ? philox10_lo((uint32_t)blk, K, st.k0, st.k1)
                          : philox10_dev((uint32_t)blk, (uint32_t)(blk >> 32), st.c2, st.c3,
                                         st.k0, st.k1);
          float z[4];
          box_muller_screen(x.x, x.y, z[0], z[1]);
          box_muller_screen(x.z, x.w, z[2], z[3]);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float2 e = ab[j];
            const float a = __builtin_fmaf(e.x, z[t], e.y);
            cur = __builtin_fmaf(-a, a, cur);
            if (++j == d) {  // wave-uniform: a row of the span is complete
              if (q == 0) rs[0] = cur;
              else if (q == 1) rs[1] = cur;
              else if (q == 2) rs[2] = cur;
              else rs[3] = cur;
              cur = 0.0f;
              j = 0;
              ++q;
            }
          }
        }
        span_tail(ns, rs);
      }
    };
    const bool lo = (uint64_t)(n1 + 4) * (uint64_t)d / 4u + (uint64_t)d <= 0xffffffffull;
    if (lo) {
      spans(std::true_type{});
    } else {
      spans(std::false_type{});
    }
    if (lane == 0) {
      if (own) {
        scnt[kSmallHdr * g] = used;
        gtau[g * CWQ_CSR_GTAU_STRIDE] = ord_f32(tau);
      } else {
        atomicMax(&gtau[g * CWQ_CSR_GTAU_STRIDE], ord_f32(tau));
      }
    }
  }
}

template <bool STEP0>
__global__ void __launch_bounds__(256) k_small_survivors(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const float* __restrict__ best,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t nb, int64_t n_cand, SeedSpec sd,
    int32_t step, const float4* __restrict__ grp, const uint32_t* __restrict__ gtau,
    const uint32_t* __restrict__ scnt, const uint2* __restrict__ slist,
    const float* __restrict__ bpre, unsigned long long* __restrict__ keys) {
  __shared__ double logtab[32];
  // per wave: the listed rows still reaching their block's final threshold,
  // queued until 64 of them can be scored at once, one per lane (a lane per
  // slot left ~6% of the lanes busy: ~1 survivor per block, 8 slots)
  constexpr int kQueue = 64 + 64 * CWQ_SLIST_PER_BLOCK;
  __shared__ int64_t q_g[4][kQueue];
  __shared__ uint32_t q_n[4][kQueue];
  fill_logtab(logtab);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = wave_id();
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  auto score = [&](int64_t g, uint32_t n) {
    const BlockSpan sp = block_span(block_off, ud, g);
    const float* bg = bpre + kSmallHdr * g;  // k_small_prep's header: the step's stream key
    const PhiloxStream st{f2u(bg[1]), f2u(bg[2]), f2u(bg[3]), f2u(bg[4])};
    const uint64_t k0 = (uint64_t)n * (uint64_t)sp.d;
    const float v = eval_row<0, STEP0>(st, k0, sp.d, (int)(k0 & 3u), loc_s + sp.off,
                                       scale_s + sp.off, t_loc + sp.off, t_scale + sp.off,
                                       lognorm + sp.off, STEP0 ? nullptr : best + sp.off, logtab);
    atomicMax(&keys[g], (unsigned long long)argmax_key(v, n));
  };
  int q = 0;  // wave-uniform queue length
  for (int64_t gb = ((int64_t)blockIdx.x * 4 + wv) * 64; gb < nb; gb += nwaves * 64) {
    const int64_t g = gb + lane;
    uint32_t cnt = 0, keep = 0;  // listed slots; bit s: slot s survives
    if (g < nb && grp[g].x != 0.0f) {  // exact blocks are scored below
      const uint32_t c = scnt[kSmallHdr * g];
      const uint32_t ns = c < CWQ_SLIST_PER_BLOCK ? c : CWQ_SLIST_PER_BLOCK;
      const float tau = unord_f32(gtau[g * CWQ_CSR_GTAU_STRIDE]);
      for (uint32_t sl = 0; sl < ns; ++sl)
        if (u2f(slist[CWQ_SLIST_PER_BLOCK * g + sl].y) >= tau) {
          keep |= 1u << sl;
          ++cnt;
        }
    }
    // exclusive scan of the counts: this lane's first queue position
    uint32_t inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)inc, (unsigned)o, 64);
      if (lane >= (uint32_t)o) inc += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)inc, 63, 64);
    uint32_t pos = (uint32_t)q + inc - cnt;
    for (uint32_t m = keep; m != 0u; m &= m - 1u) {
      const uint32_t sl = (uint32_t)__builtin_ctz(m);
      q_g[wv][pos] = g;
      q_n[wv][pos] = slist[CWQ_SLIST_PER_BLOCK * g + sl].x;
      ++pos;
    }
    q += (int)total;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    while (q >= 64) {  // a full batch: the queue's last 64 entries
      q -= 64;
      const int64_t qg = q_g[wv][q + (int)lane];
      const uint32_t qn = q_n[wv][q + (int)lane];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      score(qg, qn);
    }
    // blocks k_small_screen did not screen (constants failed the gate, or
    // their survivor slots overflowed): every candidate exactly, the wave per block
    for (uint64_t m = __ballot(g < nb && grp[g].x == 0.0f); m != 0ull; m &= m - 1ull) {
      const int64_t ge = gb + (int64_t)__builtin_ctzll(m);
      const BlockSpan sp = block_span(block_off, ud, ge);
      const float* bg = bpre + kSmallHdr * ge;
      const PhiloxStream st{f2u(bg[1]), f2u(bg[2]), f2u(bg[3]), f2u(bg[4])};
      uint64_t bestk = 0;
      for (int r = 0; r < 4; ++r) {  // rows n = r (mod 4): one alignment class per pass
        const int align = (int)(((uint64_t)r * (uint64_t)sp.d) & 3u);
        for (int64_t n = r + 4 * (int64_t)lane; n < n_cand; n += 256) {
          const float v = eval_row<0, STEP0>(st, (uint64_t)n * (uint64_t)sp.d, sp.d, align,
                                             loc_s + sp.off, scale_s + sp.off, t_loc + sp.off,
                                             t_scale + sp.off, lognorm + sp.off,
                                             STEP0 ? nullptr : best + sp.off, logtab);
          const uint64_t k = argmax_key(v, (uint32_t)n);
          bestk = k > bestk ? k : bestk;
        }
      }
      bestk = wave_max_u64(bestk);
      if (lane == 0 && bestk) atomicMax(&keys[ge], (unsigned long long)bestk);
    }
  }
  if ((int)lane < q) score(q_g[wv][lane], q_n[wv][lane]);
}

// ---------------------------------------------------------------------------
// The small-candidate shapes (64 <= 2^b < 4096 candidates, blocks of d <=
// CWQ_FUSED_DMAX): shared pieces of the small pipeline below (k_small_*).
// Round 4 ran these shapes as one kernel (k_small_fused: a wave per four
// blocks doing constants, screen, exact survivors and finalize); round 5
// split it (see "The small-candidate step as a pipeline").
// ---------------------------------------------------------------------------
#ifndef CWQ_FUSED_LIST
#define CWQ_FUSED_LIST 64  // listed rows per block
#endif
#ifndef CWQ_FUSED_STAGE
#define CWQ_FUSED_STAGE 256  // (row, dim) values per exact batch
#endif
#ifndef CWQ_FUSED_WAVES
#define CWQ_FUSED_WAVES 8
#endif
static_assert(CWQ_FUSED_STAGE >= CWQ_FUSED_DMAX, "an exact batch holds at least one row");
static_assert(CWQ_FUSED_LIST <= 64, "one listed row per lane");

// Exact normal k of a block's stream: its Philox block and the one
// Box-Muller pair that holds it (normal4_dev's element k & 3, bit for bit).
#ifndef CWQ_EXACT_NOINLINE
#define CWQ_EXACT_NOINLINE 0  // inline (k_small_one has no loop to hoist its constants out of)
#endif
#if CWQ_EXACT_NOINLINE
__device__ __noinline__
#else
__device__ __forceinline__
#endif
float exact_normal(const PhiloxStream& st, uint64_t k, const double* logtab) {
  const U4 x = philox_block_dev(st, k >> 2);
  const bool hi = (k & 2u) != 0;
  float f0, f1;
  box_muller_dev(hi ? x.z : x.x, hi ? x.w : x.y, logtab, f0, f1);
  return (k & 1u) ? f1 : f0;
}

// LDS written by some lanes of a wave and read by others: order the wave's
// accesses (no workgroup barrier: a wave's LDS is its own)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint32_t lane_rank(uint64_t m) {  // set lanes of m below this one
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// A block for quad_exact_block: its first dim, length and step stream
struct QuadBlk {
  int64_t off;
  uint32_t d, k0, k1, c2, c3;
};
// a block's state in the small pipeline (SmallRec q0.w, then k_small_one's)
constexpr uint32_t kQuadKnown = 0;   // idx decided (empty block, or a single listed row)
constexpr uint32_t kQuadListed = 1;  // screened; listed rows scored exactly
constexpr uint32_t kQuadExact = 2;   // every candidate scored exactly

#ifndef CWQ_FUSED_NOINLINE
#define CWQ_FUSED_NOINLINE 1  // the rare whole-block exact path out of line (its registers)
#endif
#if CWQ_FUSED_NOINLINE
#define CWQ_RARE __device__ __noinline__
#else
#define CWQ_RARE __device__ __forceinline__
#endif
// Every candidate of a block exactly (eval_row, a lane per row): k_small_one's
// fallback for blocks outside the screening gate or with a full list.
// Returns the wave's best argmax key.
template <bool STEP0>
CWQ_RARE unsigned long long quad_exact_block(const QuadBlk r, const float* __restrict__ t_loc,
                                             const float* __restrict__ t_scale,
                                             const float* __restrict__ loc_s,
                                             const float* __restrict__ scale_s,
                                             const float* __restrict__ lognorm,
                                             const float* __restrict__ best, int64_t n_cand,
                                             const double* logtab) {
  const uint32_t lane = threadIdx.x & 63u;
  const PhiloxStream se{r.k0, r.k1, r.c2, r.c3};
  const int64_t ob = r.off;
  const int db = (int)r.d;
  uint64_t bestk = 0;
  for (int rr = 0; rr < 4; ++rr) {  // rows n = rr (mod 4): one alignment class per pass
    const int align = (int)(((uint64_t)rr * (uint64_t)db) & 3u);
    for (int64_t n = rr + 4 * (int64_t)lane; n < n_cand; n += 256) {
      const float v = eval_row<0, STEP0>(se, (uint64_t)n * (uint64_t)db, db, align, loc_s + ob,
                                         scale_s + ob, t_loc + ob, t_scale + ob, lognorm + ob,
                                         STEP0 ? nullptr : best + ob, logtab);
      const uint64_t kk = argmax_key(v, (uint32_t)n);
      bestk = kk > bestk ? kk : bestk;
    }
  }
  return wave_max_u64(bestk);
}

#ifdef CWQ_QUAD_TIMES
// timing builds only (tools/quad_times.py --one): per block of k_small_one the
// wall clock (s_memrealtime, 100 MHz) at its start [0], after its screen [1]
// and at its end [2..5]; info = HW_ID, XCC_ID, listed rows scored exactly,
// exact-block flag | d << 8
constexpr int kQuadTimes = 1 << 16;
__device__ unsigned long long g_quad_t[kQuadTimes][6];
__device__ unsigned int g_quad_info[kQuadTimes][4];
#endif

// ---------------------------------------------------------------------------
// The small-candidate step as a pipeline (round 5): blocks of d <= 64,
// 64 <= 2^b < 4096 candidates (C2/C3's 8-bit groups).  tools/quad_times.py
// showed where k_small_fused's time went on C2 (41.5k groups, 10.4k quads):
// the quads ran at the chip's issue rate while 8 waves shared each SIMD, but
// every quad took ~29 us, so the launch drained for ~35 us of its 62-69 us
// at falling occupancy, and 35% of a quad's time went to its constants phase
// (per-block f64 sums and bounds on 16-lane rows, DPP reductions, the stream
// key).  Here the per-block work runs lane-parallel before the screen, and
// the screen runs a wave per block:
//   k_small_prep1     a workgroup per CWQ_PREP1_BLOCKS blocks, a thread per
//                     dim: the shard constants (step 0, k_prep_dims'
//                     arithmetic) and each dim's screening constants
//                     (csr_dim), summed per block in LDS; then a thread per
//                     block: bounds, stream key -> a 64-byte record; the
//                     dim -> block map
//   k_small_one       a wave per block: screen, exact survivors -> index
//                     (variants measured in DESIGN.md 5e: more blocks per
//                     wave or per workgroup, a striding grid, a second kernel
//                     for the exact paths, the finalize fused in: all slower)
//   k_small_finalize  a thread per dim: best += the winning row (:63), and
//                     at the last step the destandardised sample (:292)
// ---------------------------------------------------------------------------
struct SmallRec {  // 4 x uint4: q0 = (off lo, off hi, d, state), q1 = stream key,
  uint4 q0, q1;    // q2 = (bf, c1, c2, As), q3 = (Pq, -, -, -)
  uint4 q2, q3;
};
static_assert(sizeof(SmallRec) <= 8 * CWQ_SLIST_PER_BLOCK, "a record per block in slist");
// blocks per k_small_prep1 workgroup of CWQ_PREP1_THREADS threads: C2's 41.5k
// blocks make 650 workgroups (with 256 per workgroup 163 of them ran 20 us,
// latency-bound)
#ifndef CWQ_PREP1_BLOCKS
#define CWQ_PREP1_BLOCKS 64
#endif
#ifndef CWQ_PREP1_THREADS
#define CWQ_PREP1_THREADS 256
#endif
constexpr int kSmallPrepBlocks = CWQ_PREP1_BLOCKS;
static_assert(CWQ_PREP1_BLOCKS <= CWQ_PREP1_THREADS, "a thread per block in the block phase");

// The dims of a launch's blocks: [block_off[0], block_off[nb]) (absolute: a
// forked part of a launch passes block_off + g0), or [0, nb ud) for uniform blocks
__device__ __forceinline__ void dims_of(const int64_t* __restrict__ block_off, int64_t ud,
                                        int64_t nb, int64_t& d0, int64_t& d1) {
  d0 = block_off ? block_off[0] : 0;
  d1 = block_off ? block_off[nb] : nb * ud;
}

// FIRST (step 0): also the shard constants and best = 0 (k_prep_dims).  The
// block sums are LDS atomics in no fixed order, which the bounds' slack (far
// above double rounding) covers, so the screen stays exact-safe.
template <bool FIRST>
__global__ void __launch_bounds__(CWQ_PREP1_THREADS) k_small_prep1(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ p_loc, const float* __restrict__ p_scale, float nst, float sdiv,
    float rho, float* __restrict__ loc_s, float* __restrict__ scale_s,
    float* __restrict__ lognorm, float* __restrict__ best, const int64_t* __restrict__ block_off,
    int64_t ud, int64_t nb, SeedSpec sd, int32_t step, float2* __restrict__ pre_ab,
    SmallRec* __restrict__ rec, uint32_t* __restrict__ dmap) {
  constexpr int B = kSmallPrepBlocks;
  constexpr int T = CWQ_PREP1_THREADS;
  __shared__ int64_t boff[B + 1];
  __shared__ double acc[5][B];  // sum M, sum |M|, sum |M| + M, sum A^2, sum C
  __shared__ uint32_t amx[B], abad[B];
  const int t = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * B;
  const int n = (int)(nb - g0 < B ? nb - g0 : B);
  for (int k = t; k <= n; k += T) boff[k] = block_off ? block_off[g0 + k] : (g0 + k) * ud;
  if (t < B) {
    for (int k = 0; k < 5; ++k) acc[k][t] = 0.0;
    amx[t] = 0u;
    abad[t] = 0u;
  }
  __syncthreads();
  const int64_t i0 = boff[0], i1 = boff[n];
  for (int64_t i = i0 + t; i < i1; i += T) {
    int lo = 0, hi = n;  // boff[lo] <= i < boff[hi] (empty blocks are skipped)
    while (hi - lo > 1) {
      const int m = (lo + hi) >> 1;
      if (boff[m] <= i) lo = m; else hi = m;
    }
    float ls, ss, c;
    const float sg = t_scale[i];
    if (FIRST) {  // as k_prep_dims
      shard_consts(p_loc[i], p_scale[i], nst, sdiv, rho, ls, ss);
      c = lognorm_of(sg);
      loc_s[i] = ls;
      scale_s[i] = ss;
      lognorm[i] = c;
    } else {
      ls = loc_s[i];
      ss = scale_s[i];
      c = lognorm[i];
    }
    const ScreenDim o = screen_dim<FIRST>(ls, ss, t_loc[i], sg, c, FIRST ? 0.0f : best[i]);
    pre_ab[i] = float2{o.sa, o.sb};
    atomicAdd(&acc[0][lo], o.M);
    atomicAdd(&acc[1][lo], __builtin_fabs(o.M));
    atomicAdd(&acc[2][lo], __builtin_fabs(o.M) + o.M);
    atomicAdd(&acc[3][lo], (double)o.A * (double)o.A);
    atomicAdd(&acc[4][lo], (double)o.C);
    atomicMax(&amx[lo], f2u(o.A));  // A >= 0: float order is uint order
    if (!o.ok) atomicOr(&abad[lo], 1u);
    dmap[i] = (uint32_t)(g0 + lo);
  }
  __syncthreads();
  if (t >= n) return;
  const int64_t g = g0 + t;
  const int64_t off = boff[t];
  const int d = (int)(boff[t + 1] - off);
  ScreenSums u;
  u.sm = acc[0][t];
  u.sa = acc[1][t];
  u.sk = acc[2][t];
  u.s2 = acc[3][t];
  u.cs = acc[4][t];
  u.mx = (double)u2f(amx[t]);
  const ScreenBlock bc = screen_block_consts(u, d, (double)d);  // rows summed sequentially
  const float bf = bc.bf, c1 = bc.c1, c2 = bc.c2, as = bc.as, pq = bc.pq;
  const bool screen = abad[t] == 0u && d > 0 && d <= CWQ_FUSED_DMAX && bc.finite &&
                      bf - bf == 0.0f && u.mx - u.mx == 0.0;
  const PhiloxStream st = generate_key(step_seed(sd.of(g), step), 42);
  SmallRec r;
  r.q0 = uint4{(uint32_t)off, (uint32_t)((uint64_t)off >> 32), (uint32_t)d,
               d == 0 ? kQuadKnown : (screen ? kQuadListed : kQuadExact)};
  r.q1 = uint4{st.k0, st.k1, st.c2, st.c3};
  r.q2 = uint4{f2u(bf), f2u(c1), f2u(c2), f2u(as)};
  r.q3 = uint4{f2u(pq), 0u, 0u, 0u};
  rec[g] = r;
}

// The exact values of a block's listed rows (k_small_one), lane-parallel over
// (row, dim): each lane computes one normal exactly (its Philox block and the
// one Box-Muller pair holding it) and its log-density into lpv; a lane per row
// then sums in the Eigen order (eval_row's values bit for bit).  Returns the
// wave's best argmax key.  Out of line: its f64 Box-Muller constants would
// otherwise occupy k_small_one's registers for the whole kernel.
template <bool STEP0>
CWQ_RARE unsigned long long small_listed_exact(
    int64_t off, int db, const PhiloxStream sb, uint32_t used, const uint32_t* ln, float* lpv,
    const double* logtab, const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const float* __restrict__ best) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t du = (uint32_t)db;
  const uint32_t per = (uint32_t)CWQ_FUSED_STAGE / du;  // rows per batch (>= 1: d <= 64)
  uint64_t bestk = 0;
  for (uint32_t e0 = 0; e0 < used; e0 += per) {
    const uint32_t e1 = e0 + per < used ? e0 + per : used;
    const uint32_t i1 = (e1 - e0) * du;
    for (uint32_t it = lane; it < i1; it += 64) {
      const uint32_t e = e0 + it / du;
      const uint32_t j = it - (e - e0) * du;
      const int64_t ei = off + j;
      const float zz = exact_normal(sb, (uint64_t)ln[e] * (uint64_t)du + j, logtab);
      const float sc = scale_s[ei];
      const float sv = shard_sample(loc_s[ei], sc, zz);
      const float tv = STEP0 ? sv : best[ei] + sv;  // :57
      lpv[it] = log_prob(tv, t_loc[ei], t_scale[ei], lognorm[ei]);
    }
    wave_lds_sync();
    const uint32_t e = e0 + lane;
    if (e < e1) {  // a lane per row: the Eigen-order sum (eval_row_f)
      const float* x = lpv + (e - e0) * du;
      const int vec = db & ~7;
      float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int jj = 0; jj < vec; jj += 8) {
#pragma unroll
        for (int l = 0; l < 8; ++l) p[l] = p[l] + x[jj + l];
      }
      float sum = 0.0f;
      for (int jj = vec; jj < db; ++jj) sum = sum + x[jj];
      const uint64_t k = argmax_key(eigen_fold8(p, sum), ln[e]);
      bestk = k > bestk ? k : bestk;
    }
    wave_lds_sync();
  }
  return wave_max_u64(bestk);
}

// A wave (a 64-thread workgroup) per block: the screen (k_small_screen's spans)
// and the exact scoring of the listed rows; writes the index (out_idx).  The
// dispatcher hands a slot to the next wave as soon as one ends.  Measured
// alternatives on C2
// (tools/quad_times.py --one): persistent waves drawing blocks from one
// atomic counter, 474 us (41.5k same-address atomics serialise at ~11 ns);
// two blocks per wave in a loop, 69 us against 47 (the loop's spills), or
// as straight-line copies (2 or 4 blocks, 6-8 waves/SIMD): no gain on C2 or
// C3 (C3's scoring 1.11-1.20 ms per step in all five);
// longest blocks first (a counting sort by d), 41 us against 47 but the sort
// cost a launch and a histogram that needed zeroing.
template <bool STEP0>
__global__ void __launch_bounds__(64, CWQ_FUSED_WAVES) k_small_one(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const float* __restrict__ best,
    const SmallRec* __restrict__ rec, const float2* __restrict__ pre_ab, int64_t nb, int64_t u0,
    int64_t n_cand, int32_t step, int n_steps, int32_t* __restrict__ out_idx) {
  __shared__ double logtab[32];
  // the block's (sA, sB) repeated 4 times: a lane's span of 4 rows is 4 d
  // normals, so Philox block b covers abx[4 b .. 4 b + 3] (two b128 reads,
  // issued ahead of the Philox rounds that hide their latency)
  __shared__ float4 abx[2 * CWQ_FUSED_DMAX];
  __shared__ uint32_t ln[CWQ_FUSED_LIST];
  __shared__ float lu[CWQ_FUSED_LIST];
  __shared__ float lpv[CWQ_FUSED_STAGE];
  __shared__ unsigned long long kmax;
  const uint32_t lane = threadIdx.x & 63u;
  if (lane < 32) logtab[lane] = kLogTabConst[lane];
  auto ufirst = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
  auto ffirst = [&](uint32_t v) { return u2f(ufirst(v)); };
  const int64_t g = u0 + blockIdx.x;
  {
#ifdef CWQ_QUAD_TIMES  // tools/quad_times.py --one: per block start, after the screen, end
    if (lane == 0u && g < kQuadTimes) g_quad_t[g][0] = __builtin_amdgcn_s_memrealtime();
#endif
    const uint4 q0 = rec[g].q0, q1 = rec[g].q1;
    const int64_t off = (int64_t)(((uint64_t)ufirst(q0.y) << 32) | ufirst(q0.x));
    const int db = (int)ufirst(q0.z);
    uint32_t state = ufirst(q0.w);
    PhiloxStream sb;
    sb.k0 = ufirst(q1.x);
    sb.k1 = ufirst(q1.y);
    sb.c2 = ufirst(q1.z);
    sb.c3 = ufirst(q1.w);
    uint32_t idx = 0u;
    uint32_t used = 0;
    if (lane == 0) kmax = 0ull;
    wave_lds_sync();
    if (state == kQuadListed) {
      const uint4 q2 = rec[g].q2;
      const float bfb = ffirst(q2.x), c1b = ffirst(q2.y), c2b = ffirst(q2.z);
      const float asb = ffirst(q2.w), pqb = ffirst(rec[g].q3.x);
      if ((int)lane < db) {  // d <= 64 (launch_small)
        const float2 e = pre_ab[off + lane];
        float2* ax = (float2*)abx;
        for (int r = 0; r < 4; ++r) ax[r * db + (int)lane] = e;
      }
      wave_lds_sync();
      const PhiloxLo K = philox_lo_key(sb);  // n_cand * d / 4 < 2^32 (d <= 64, < 4096 rows)
      float tau = -__builtin_inff();
      bool over = false;
      for (int64_t m0 = 0; 256 * m0 < n_cand; ++m0) {
        const int64_t ns = 4 * ((int64_t)lane + 64 * m0);
        const uint32_t b0 = (uint32_t)((uint64_t)ns * (uint64_t)db / 4u);
        float rs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float cur = 0.0f;
        int j = 0, qd = 0;
        for (int b = 0; b < db; ++b) {
          const float4 e01 = abx[2 * b], e23 = abx[2 * b + 1];
          const U4 x = philox10_lo(b0 + (uint32_t)b, K, sb.k0, sb.k1);
          float z[4];
          box_muller_screen(x.x, x.y, z[0], z[1]);
          box_muller_screen(x.z, x.w, z[2], z[3]);
          const float2 ev[4] = {float2{e01.x, e01.y}, float2{e01.z, e01.w},
                                float2{e23.x, e23.y}, float2{e23.z, e23.w}};
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) {
            const float2 e = ev[tt];  // = (sA, sB) of dim j
            const float a = __builtin_fmaf(e.x, z[tt], e.y);
            cur = __builtin_fmaf(-a, a, cur);
            if (++j == db) {  // wave-uniform: a row of the span is complete
              if (qd == 0) rs[0] = cur;
              else if (qd == 1) rs[1] = cur;
              else if (qd == 2) rs[2] = cur;
              else rs[3] = cur;
              cur = 0.0f;
              j = 0;
              ++qd;
            }
          }
        }
        uint64_t m[4];
        const uint32_t cnt = span_vote(rs, ns, n_cand, c1b, c2b, asb, pqb, bfb, tau, m);
        if (cnt == 0) continue;
        if (used + cnt > CWQ_FUSED_LIST) {  // drop the rows the raised tau excludes
          const bool have = lane < used;
          const uint32_t nl = have ? ln[lane] : 0u;
          const float ul = have ? lu[lane] : 0.0f;
          const uint64_t keep = __ballot(have && ul >= tau);
          if ((keep >> lane) & 1ull) {
            const uint32_t r = lane_rank(keep);
            ln[r] = nl;
            lu[r] = ul;
          }
          used = (uint32_t)__builtin_popcountll(keep);
          wave_lds_sync();
        }
        if (used + cnt > CWQ_FUSED_LIST) {  // list full (near-ties): score the block exactly
          over = true;
          break;
        }
        uint32_t at = used;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const uint64_t mq = m[qq];
          if ((mq >> lane) & 1ull) {
            const uint32_t slot_i = at + lane_rank(mq);
            ln[slot_i] = (uint32_t)(ns + qq);
            lu[slot_i] = screen_row_upper(rs[qq], c1b, bfb);
          }
          at += (uint32_t)__builtin_popcountll(mq);
        }
        used = at;
        wave_lds_sync();
      }
      if (over) {
        state = kQuadExact;
        used = 0;
      } else {
        // keep the rows whose upper bound reaches the block's final tau
        const bool have = lane < used;
        const uint32_t nl = have ? ln[lane] : 0u;
        const uint64_t keep = __ballot(have && lu[have ? lane : 0] >= tau);
        const uint32_t nk = (uint32_t)__builtin_popcountll(keep);
        if (nk == 1u) {  // the single listed row is the argmax: no exact value needed
          idx = ufirst((uint32_t)__builtin_amdgcn_readlane((int)nl, __builtin_ctzll(keep)));
          state = kQuadKnown;
          used = 0;
        } else {
          if ((keep >> lane) & 1ull) ln[lane_rank(keep)] = nl;
          used = nk;
          if (nk == 0u) state = kQuadExact;  // (never: the best lower bound's row is listed)
        }
        wave_lds_sync();
      }
    }
#ifdef CWQ_QUAD_TIMES
    if (lane == 0u && g < kQuadTimes) {
      g_quad_t[g][1] = __builtin_amdgcn_s_memrealtime();
      g_quad_info[g][0] = (uint32_t)__builtin_amdgcn_s_getreg((4) | (0 << 6) | ((32 - 1) << 11));
      g_quad_info[g][1] = (uint32_t)__builtin_amdgcn_s_getreg((20) | (0 << 6) | ((4 - 1) << 11));
      g_quad_info[g][2] = used;
      g_quad_info[g][3] = (state == kQuadExact ? 1u : 0u) | ((uint32_t)db << 8);
    }
#endif
    if (state == kQuadListed && used > 0) {  // rare (C2: 0.6% of the blocks): out of line
      const unsigned long long bk = small_listed_exact<STEP0>(
          off, db, sb, used, ln, lpv, logtab, t_loc, t_scale, loc_s, scale_s, lognorm, best);
      if (lane == 0) kmax = bk;
      wave_lds_sync();
    }
    if (state == kQuadExact) {  // every candidate exactly (constants outside the gate, list full)
      QuadBlk r;
      r.off = off;
      r.d = (uint32_t)db;
      r.k0 = sb.k0;
      r.k1 = sb.k1;
      r.c2 = sb.c2;
      r.c3 = sb.c3;
      const unsigned long long bk = quad_exact_block<STEP0>(r, t_loc, t_scale, loc_s, scale_s,
                                                             lognorm, best, n_cand, logtab);
      if (lane == 0) kmax = bk;
      wave_lds_sync();
    }
    if (state != kQuadKnown) idx = key_index(kmax);
    if (lane == 0) out_idx[g * n_steps + step] = (int32_t)idx;
#ifdef CWQ_QUAD_TIMES
    if (lane == 0u && g < kQuadTimes)
      g_quad_t[g][2] = g_quad_t[g][3] = g_quad_t[g][4] = g_quad_t[g][5] =
          __builtin_amdgcn_s_memrealtime();
#endif
  }
}

// A thread per dim of [d0, d0 + n): best += the winning row of its block (:63)
template <bool STEP0>
__global__ void __launch_bounds__(256) k_small_finalize(
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const SmallRec* __restrict__ rec, const uint32_t* __restrict__ dmap,
    const int32_t* __restrict__ out_idx, int32_t step, int n_steps,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t nb, float* __restrict__ best,
    float* __restrict__ ds_out, const float* __restrict__ ds_loc,
    const float* __restrict__ ds_scale) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  int64_t d0, d1;
  dims_of(block_off, ud, nb, d0, d1);
  for (int64_t i = d0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < d1;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t g = dmap[i];
    const uint4 q0 = rec[g].q0, q1 = rec[g].q1;
    const int64_t off = (int64_t)(((uint64_t)q0.y << 32) | q0.x);
    const uint32_t d = q0.z, j = (uint32_t)(i - off);
    const PhiloxStream st{q1.x, q1.y, q1.z, q1.w};
    const uint32_t idx = (uint32_t)out_idx[(int64_t)g * n_steps + step];  // k_small_one's
    const float zz = exact_normal(st, (uint64_t)idx * (uint64_t)d + j, logtab);
    const float sc = scale_s[i];
    const float sv = shard_sample(loc_s[i], sc, zz);
    const float b = (STEP0 ? 0.0f : best[i]) + sv;
    best[i] = b;
    if (ds_out) ds_out[i] = destandardise_1(b, ds_loc[i], ds_scale[i]);  // :292
  }
}

// ---------------------------------------------------------------------------
// Encoder, end of a step: index -> out_idx; best += winning candidate (:63).
// General shapes (CSR groups, uniform d the float4 kernel does not take): one
// thread per flat dim i, which finds its block by binary search in block_off
// and regenerates its own word of the winning row; threads t < nb also write
// block t's index.  Work is spread evenly whatever the group sizes (a few
// 4095-dim groups or 10^5 tiny ones).  The dims covered are
// [block_off[0], block_off[nb]) (absolute: a forked part of a launch passes
// block_off + g0).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int64_t block_of_dim(const int64_t* __restrict__ off, int64_t nb,
                                                int64_t i) {
  int64_t lo = 0, hi = nb;  // off[lo] <= i < off[hi]; empty blocks are skipped
  while (hi - lo > 1) {
    const int64_t m = (lo + hi) >> 1;
    if (off[m] <= i) lo = m; else hi = m;
  }
  return lo;
}

__global__ void __launch_bounds__(256) k_encode_finalize(
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t nb, SeedSpec sd, int32_t step,
    int n_steps,
    const unsigned long long* __restrict__ keys, int32_t* __restrict__ out_idx,
    float* __restrict__ out_sample) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  const int64_t d0 = block_off ? block_off[0] : 0;
  const int64_t d1 = block_off ? block_off[nb] : nb * ud;
  const int64_t nt = (d1 - d0) > nb ? (d1 - d0) : nb;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nt;
       t += (int64_t)gridDim.x * blockDim.x) {
    if (t < nb) out_idx[t * n_steps + step] = (int32_t)key_index(keys[t]);
    const int64_t i = d0 + t;
    if (i >= d1) continue;
    const int64_t g = block_off ? block_of_dim(block_off, nb, i) : i / ud;
    const int64_t off = block_off ? block_off[g] : g * ud;
    const int64_t d = block_off ? block_off[g + 1] - off : ud;
    const uint32_t idx = key_index(keys[g]);
    const PhiloxStream st =
        generate_key(step_seed(sd.of(g), step), 42);
    const uint64_t k = (uint64_t)idx * (uint64_t)d + (uint64_t)(i - off);
    const float zz = f4_word(normal4_dev(st, k >> 2, logtab), (uint32_t)(k & 3u));
    const float sc = scale_s[i];
    const float sv = shard_sample(loc_s[i], sc, zz);
    out_sample[i] = out_sample[i] + sv;
  }
}

// Uniform blocks with d % 4 == 0, d <= 256: every row n*d starts on a Philox
// block, so one lane owns Philox block q of its block's winning row and with
// it dims 4q..4q+3 -- one Philox + two Box-Muller pairs per 4 dims, float4
// loads and stores.  A wave holds 64 / (d/4) whole blocks (lane -> (block,
// q) is fixed per lane: no 64-bit division in the loop); its chunks of blocks
// are strided over the grid's waves.
struct Q4Lane {
  bool active;
  uint32_t lb, q;  // block within the wave's chunk, Philox block within the row
};
__device__ __forceinline__ Q4Lane q4_lane(uint32_t qpb, uint32_t bpw) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t lb = lane / qpb;
  return Q4Lane{lb < bpw, lb, lane - lb * qpb};
}

__global__ void __launch_bounds__(256) k_encode_finalize_q4(
    const float4* __restrict__ loc_s, const float4* __restrict__ scale_s, uint32_t qpb,
    uint32_t bpw, int64_t nb, SeedSpec sd, int32_t step, int n_steps,
    const unsigned long long* __restrict__ keys, int32_t* __restrict__ out_idx,
    float4* __restrict__ out_sample) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  const Q4Lane L = q4_lane(qpb, bpw);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t c = (int64_t)blockIdx.x * 4 + wave_id(); c * bpw < nb; c += nwaves) {
    const int64_t g = c * bpw + L.lb;
    if (!L.active || g >= nb) continue;
    const int64_t t = g * qpb + L.q;
    const uint32_t idx = key_index(keys[g]);
    if (L.q == 0) out_idx[g * n_steps + step] = (int32_t)idx;
    const PhiloxStream st =
        generate_key(step_seed(sd.of(g), step), 42);
    const F4 z = normal4_dev(st, (uint64_t)idx * qpb + L.q, logtab);
    const float4 l = loc_s[t], sc = scale_s[t];
    float4 b = out_sample[t];
    b.x = b.x + shard_sample(l.x, sc.x, z.a);
    b.y = b.y + shard_sample(l.y, sc.y, z.b);
    b.z = b.z + shard_sample(l.z, sc.z, z.c);
    b.w = b.w + shard_sample(l.w, sc.w, z.d);
    out_sample[t] = b;
  }
}

// ---------------------------------------------------------------------------
// Decoder (coded_greedy_sampler.py:93-167), O(n_steps * d) per block: only the
// selected row of each step is regenerated.  General shapes: one thread per
// flat dim, block found as in k_encode_finalize.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_decode(
    const int32_t* __restrict__ idx, const float* __restrict__ p_loc,
    const float* __restrict__ p_scale, const int64_t* __restrict__ block_off, int64_t ud,
    int64_t nb, int n_steps, int64_t n_cand, float nst, float sdiv, float rho, int32_t seed,
    int64_t block_id_base, float* __restrict__ out_sample) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  const int64_t d0 = block_off ? block_off[0] : 0;
  const int64_t d1 = block_off ? block_off[nb] : nb * ud;
  for (int64_t i = d0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < d1;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = block_off ? block_of_dim(block_off, nb, i) : i / ud;
    const int64_t off = block_off ? block_off[g] : g * ud;
    const int64_t d = block_off ? block_off[g + 1] - off : ud;
    const int32_t sg = block_seed(seed, block_id_base + g);
    float ls, ss;
    shard_consts(p_loc[i], p_scale[i], nst, sdiv, rho, ls, ss);
    float v = 0.0f;  // sample = tf.zeros (:143)
    for (int s = 0; s < n_steps; ++s) {
      const int64_t n = idx[g * n_steps + s];
      if (n < 0 || n >= n_cand) {
        v = __builtin_nanf("");
        continue;
      }
      const PhiloxStream st = generate_key(step_seed(sg, s), 42);
      const uint64_t k = (uint64_t)n * (uint64_t)d + (uint64_t)(i - off);
      const F4 z = normal4_dev(st, k >> 2, logtab);
      const uint32_t w = (uint32_t)(k & 3u);
      const float zz = w == 0 ? z.a : (w == 1 ? z.b : (w == 2 ? z.c : z.d));
      v = v + shard_sample(ls, ss, zz);  // :153 tile(sample) + samples, row indices[i]
    }
    out_sample[i] = v;
  }
}

// Decoder for uniform blocks with d % 4 == 0, d <= 256 (the C4/C5 shapes):
// one lane per Philox block of the selected row -- dims 4q..4q+3 of block g,
// the same dims at every step because n*d is a multiple of 4 -- so each lane
// runs one Philox + two Box-Muller pairs per step, and p_loc / p_scale / the
// sample move as float4 (coalesced across the wave).  Lanes map to blocks as
// in k_encode_finalize_q4.  With n_steps == 1 the shard divisions are by 1.0f
// (exact identities; skipped on a uniform branch).
// A wave decodes a group of B = bpw * qpb blocks (<= 64) as qpb chunks of
// bpw blocks, one lane per Philox block of a row (float4 I/O, coalesced).
// Single-step codes: lane i computes the stream key of the group's block i
// once (TF GenerateKey is itself a Philox-10 call, as costly as a row's
// block) and each chunk takes its blocks' keys by lane shuffle, so a group
// pays one key call per block instead of one per lane.  The next chunk's
// inputs are loaded before the current chunk's arithmetic, so HBM reads stay
// in flight while the exact Box-Muller runs.
#ifndef CWQ_DECODE_MIN_WAVES
#define CWQ_DECODE_MIN_WAVES 1  // waves/SIMD the decoder's registers must allow (tuning)
#endif
#ifndef CWQ_DECODE_PROBE
#define CWQ_DECODE_PROBE 0  // tuning builds: 1 = loads/stores only, 2 = arithmetic only
#endif
#ifndef CWQ_DECODE_NT
#define CWQ_DECODE_NT 1  // non-temporal float4 streams: 3-4% faster on C4 (tools/decode_variants.sh)
#endif
__global__ void __launch_bounds__(256, CWQ_DECODE_MIN_WAVES) k_decode_q4(
    const int32_t* __restrict__ idx, const float4* __restrict__ p_loc,
    const float4* __restrict__ p_scale, uint32_t qpb, uint32_t bpw, int64_t nb, int n_steps,
    int64_t n_cand, float nst, float sdiv, float rho, int32_t seed, int64_t block_id_base,
    float4* __restrict__ out_sample) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  const Q4Lane L = q4_lane(qpb, bpw);
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t B = (int64_t)bpw * qpb;
  const int64_t ngroups = (nb + B - 1) / B;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const bool unit = n_steps == 1;  // nst == sdiv == 1.0f
  for (int64_t grp = (int64_t)blockIdx.x * 4 + wave_id(); grp < ngroups; grp += nwaves) {
    const int64_t gb0 = grp * B;
    PhiloxStream kl{0u, 0u, 0u, 0u};
    if (unit)  // lanes past the group (or nb) compute an unused key
      kl = generate_key(step_seed(block_seed(seed, block_id_base + gb0 + lane), 0), 42);
    // chunk inputs: the current ones and the next chunk's, loaded one ahead
    float4 pl = float4{0.f, 0.f, 0.f, 0.f}, ps = pl;
    int32_t n1 = 0;  // single-step index
    auto load = [&](uint32_t j, float4& a, float4& b, int32_t& n) {
      const int64_t g = gb0 + (int64_t)(j * bpw + L.lb);
      if (CWQ_DECODE_PROBE == 2) {  // timing probe only: arithmetic without the loads
        a = float4{0.1f, 0.2f, 0.3f, (float)g};
        b = float4{1.0f, 1.1f, 1.2f, 1.3f};
        n = (int32_t)(g * 7919u) & 0xffff;
        return;
      }
      if (L.active && g < nb) {
        const int64_t t = g * qpb + L.q;
#if CWQ_DECODE_NT  // streamed once: non-temporal loads (tuning builds)
        typedef float nt4 __attribute__((ext_vector_type(4)));
        const nt4 va = __builtin_nontemporal_load(reinterpret_cast<const nt4*>(p_loc) + t);
        const nt4 vb = __builtin_nontemporal_load(reinterpret_cast<const nt4*>(p_scale) + t);
        a = float4{va.x, va.y, va.z, va.w};
        b = float4{vb.x, vb.y, vb.z, vb.w};
#else
        a = p_loc[t];
        b = p_scale[t];
#endif
        if (unit) n = idx[g];
      }
    };
    load(0u, pl, ps, n1);
    for (uint32_t j = 0; j < qpb; ++j) {
      const uint32_t src = j * bpw + L.lb;  // the lane holding this block's key
      const int64_t g = gb0 + (int64_t)src;
      const PhiloxStream ku{(uint32_t)__shfl((int)kl.k0, (int)src, 64),
                            (uint32_t)__shfl((int)kl.k1, (int)src, 64),
                            (uint32_t)__shfl((int)kl.c2, (int)src, 64),
                            (uint32_t)__shfl((int)kl.c3, (int)src, 64)};
      const float4 cl = pl, cs = ps;
      const int32_t cn = n1;
      if (j + 1 < qpb) load(j + 1, pl, ps, n1);
      if (!L.active || g >= nb) continue;
      float ls[4] = {cl.x, cl.y, cl.z, cl.w};
      float ss[4] = {rho * cs.x, rho * cs.y, rho * cs.z, rho * cs.w};
      if (!unit) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          ls[w] = ls[w] / nst;
          ss[w] = ss[w] / sdiv;
        }
      }
      float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sample = tf.zeros (:143)
      const int32_t sg = block_seed(seed, block_id_base + g);
      for (int i = 0; i < n_steps; ++i) {
        const int64_t n = unit ? (int64_t)cn : (int64_t)idx[g * n_steps + i];
        if (n < 0 || n >= n_cand) {
          v[0] = v[1] = v[2] = v[3] = __builtin_nanf("");
          continue;
        }
        const PhiloxStream st = unit ? ku : generate_key(step_seed(sg, i), 42);
#if CWQ_DECODE_PROBE == 1  // timing probe only: memory traffic without the arithmetic
        const F4 z{__builtin_bit_cast(float, st.k0 ^ (uint32_t)n), 1.0f, 1.0f, 1.0f};
#else
        const F4 z = normal4_dev(st, (uint64_t)n * qpb + L.q, logtab);
#endif
        const float zz[4] = {z.a, z.b, z.c, z.d};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          v[w] = v[w] + shard_sample(ls[w], ss[w], zz[w]);  // :153 sample + row indices[i]
        }
      }
#if CWQ_DECODE_NT
      typedef float nt4 __attribute__((ext_vector_type(4)));
      const nt4 vo = {v[0], v[1], v[2], v[3]};
      __builtin_nontemporal_store(vo, reinterpret_cast<nt4*>(out_sample) + g * qpb + L.q);
#else
      out_sample[g * qpb + L.q] = make_float4(v[0], v[1], v[2], v[3]);
#endif
    }
  }
}

// Single-step decode with the chunks' inputs streamed into LDS by LDS-DMA
// (global_load_lds, 16 B per lane; round 4).  The same group / chunk mapping
// as k_decode_q4, but chunk j + 2's p_loc / p_scale / index rows are in
// flight while chunk j's exact Box-Muller runs: the loads hold no VGPRs, so
// the ~90-VGPR arithmetic no longer caps how many are outstanding.  A ring of
// three slots per wave; a counted `s_waitcnt vmcnt` retires chunk j (the
// count covers only the younger chunks' loads, so the stores issued in
// between can only make it wait longer).  All LDS is one array (logf table
// first): a second __shared__ object makes hipcc wait vmcnt(0) before every
// LDS read (cdna_hip_programming.md, "three .s-level traps").
// CWQ_DECODE_GLDS (cwq_dispatch.h) 0: k_decode_q4 for single-step codes too.
#ifndef CWQ_GLDS_SLOTS
#define CWQ_GLDS_SLOTS 2  // ring slots per wave (chunks in flight: slots - 1)
#endif
constexpr int kGldsSlots = CWQ_GLDS_SLOTS;
static_assert(kGldsSlots == 2 || kGldsSlots == 3, "1 or 2 chunks ahead");
constexpr int kGldsSlot = 1024 + 1024 + 256;  // p_loc, p_scale (64 x 16 B), index (64 x 4 B)
#ifndef CWQ_GLDS_MIN_WAVES
#define CWQ_GLDS_MIN_WAVES 7  // 69 VGPRs, 2 x 2.3 KB ring per wave (tools/variants.sh glds*)
#endif
__global__ void __launch_bounds__(256, CWQ_GLDS_MIN_WAVES) k_decode_q4_glds(
    const int32_t* __restrict__ idx, const float4* __restrict__ p_loc,
    const float4* __restrict__ p_scale, uint32_t qpb, uint32_t bpw, int64_t nb, int64_t n_cand,
    float rho, int32_t seed, int64_t block_id_base, float4* __restrict__ out_sample) {
  __shared__ __attribute__((aligned(16))) char lds[256 + 4 * kGldsSlots * kGldsSlot];
  double* logtab = reinterpret_cast<double*>(lds);
  if (threadIdx.x < 32) logtab[threadIdx.x] = kLogTabConst[threadIdx.x];
  __syncthreads();
  const Q4Lane L = q4_lane(qpb, bpw);
  const uint32_t lane = threadIdx.x & 63u;
  char* ring = lds + 256 + wave_id() * (kGldsSlots * kGldsSlot);
  const int64_t B = (int64_t)bpw * qpb;
  const int64_t ngroups = (nb + B - 1) / B;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t grp = (int64_t)blockIdx.x * 4 + wave_id(); grp < ngroups; grp += nwaves) {
    const int64_t gb0 = grp * B;
    const PhiloxStream kl = generate_key(step_seed(block_seed(seed, block_id_base + gb0 + lane), 0), 42);
    const uint32_t J = qpb;
    // chunk j's rows: lane -> block gb0 + j bpw + lb, Philox block q (contiguous
    // float4s); lanes past nb or the group read row 0 (valid memory, unused)
    auto issue = [&](uint32_t j) {
      char* slot = ring + (j % kGldsSlots) * kGldsSlot;
      const int64_t g = gb0 + (int64_t)(j * bpw + L.lb);
      const bool ok = L.active && g < nb;
      const int64_t t = ok ? g * qpb + L.q : 0;
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(p_loc + t),
                                       (__attribute__((address_space(3))) void*)(slot),
                                       16, 0, 0);
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(p_scale + t),
                                       (__attribute__((address_space(3))) void*)(slot + 1024),
                                       16, 0, 0);
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(idx + (ok ? g : 0)),
                                       (__attribute__((address_space(3))) void*)(slot + 2048),
                                       4, 0, 0);
    };
    constexpr uint32_t kAhead = kGldsSlots - 1;
    for (uint32_t j = 0; j < kAhead && j < J; ++j) issue(j);
    for (uint32_t j = 0; j < J; ++j) {
      if (j + kAhead < J) issue(j + kAhead);
      // retire chunk j: at most the younger chunks' loads (3 each) may stay in flight
      const uint32_t younger = (J - 1 - j) < kAhead ? (J - 1 - j) : kAhead;
      if (younger >= 2)
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else if (younger == 1)
        asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // the slot's rows by inline-asm LDS reads: hipcc would put a vmcnt(0)
      // (every chunk in flight) in front of ordinary reads of DMA-written LDS
      char* slot = ring + (j % kGldsSlots) * kGldsSlot;
      const uint32_t a16 =
          (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)(slot) + lane * 16u;
      const uint32_t a4 =
          (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)(slot + 2048) + lane * 4u;
      float4 cl, cs;
      int32_t n;
      asm volatile(
          "ds_read_b128 %0, %3\n\t"
          "ds_read_b128 %1, %3 offset:1024\n\t"
          "ds_read_b32 %2, %4\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(cl), "=&v"(cs), "=&v"(n)
          : "v"(a16), "v"(a4)
          : "memory");
      const uint32_t src = j * bpw + L.lb;  // the lane holding this block's key
      const PhiloxStream ku{(uint32_t)__shfl((int)kl.k0, (int)src, 64),
                            (uint32_t)__shfl((int)kl.k1, (int)src, 64),
                            (uint32_t)__shfl((int)kl.c2, (int)src, 64),
                            (uint32_t)__shfl((int)kl.c3, (int)src, 64)};
      const int64_t g = gb0 + (int64_t)src;
      if (L.active && g < nb) {
        float v[4];
        if (n < 0 || n >= n_cand) {
          v[0] = v[1] = v[2] = v[3] = __builtin_nanf("");
        } else {
          const F4 z = normal4_dev(ku, (uint64_t)n * qpb + L.q, logtab);
          const float zz[4] = {z.a, z.b, z.c, z.d};
          const float ls[4] = {cl.x, cl.y, cl.z, cl.w};
          const float ss[4] = {rho * cs.x, rho * cs.y, rho * cs.z, rho * cs.w};
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            v[w] = 0.0f + shard_sample(ls[w], ss[w], zz[w]);  // :153, from tf.zeros (:143)
          }
        }
        typedef float nt4 __attribute__((ext_vector_type(4)));
        const nt4 vo = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(vo, reinterpret_cast<nt4*>(out_sample) + g * qpb + L.q);
      }
      // the slot is rewritten by issue(j + 3) next iteration: this wave's reads are done
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    }
  }
}

// Grouped (CSR) decode on the standard proposal with the destandardisation
// fused: k_decode with p_loc = 0, p_scale = 1 followed by k_destandardise, the
// same roundings in the same order.  The unit of work is a slot, one Philox
// block of a group's selected row: at step s the row n starts at flat element
// k0 = n d of the step's stream, and slot q evaluates block (k0 >> 2) + q once
// (one Philox + two exact Box-Muller pairs).  With r = k0 & 3 the four dims
// 4q .. 4q+3 (quad q) are words r..3 of slot q's block and words 0..r-1 of
// slot q+1's, so a group of d > 0 dims has ceil(d/4) + 1 slots (slot_off: that
// prefix over the groups, nb + 1 entries; an empty group has none): slot q <
// ceil(d/4) owns quad q and takes the next block from the next lane by lane
// shuffle, the group's last slot owns no dims.  r changes from step to step,
// so the accumulators stay with the dims.  (First mapping tried: ceil(d/4)
// lanes per group, a lane evaluating the next block itself where no next lane
// had it; nearly every wave then ran the Box-Muller twice per step -- lane 63
// of a long group, the last quad of a short one: DESIGN.md.)
// A wave covers slots [63 w, 63 w + 64): its lane 63 repeats the next wave's
// lane 0 and owns nothing here, so every owning lane has its next lane in the
// wave.  A group longer than 252 dims simply spans waves and workgroups.
// Stream keys (TF GenerateKey: a Philox-10 call each): the wave's lanes cover
// a contiguous run of L groups; L <= 64: lane i derives the key of (step s0 +
// i / L, the run's group i % L) for a window of 64 / L steps at once, and
// every lane takes its (group, step) key by shuffle: a 4095-dim group at 30
// steps pays one key call per wave, not 30 per lane.  L > 64 (a run of empty
// groups inside the wave's slots): each lane derives its own keys.
// Waves past the slot count ns (= slot_off[nb], passed by value) return at
// once; the last wave's lanes past it stay as shuffle partners and key
// producers only: they form no address from their own index (the one read
// they may make is a seed of the wave's own run of groups).
// U: steps evaluated together (2 for multi-step codes: a long group's waves are
// few -- one per SIMD at the c2cli shape -- and two independent Philox /
// Box-Muller chains hide each other's latency; the sums stay in step order).
template <int U>
__global__ void __launch_bounds__(256) k_decode_csr_q4(
    const int32_t* __restrict__ idx, const int64_t* __restrict__ block_off,
    const int64_t* __restrict__ slot_off, int64_t nb, int64_t ns, SeedSpec sd, int n_steps,
    int64_t n_cand, float nst, float sdiv, float rho, const float* __restrict__ dst_loc,
    const float* __restrict__ dst_scale, float* __restrict__ out) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t t0 = ((int64_t)blockIdx.x * 4 + wave_id()) * 63;
  if (t0 >= ns) return;
  const int64_t t = t0 + lane;
  const bool active = t < ns;
  const uint32_t last = (uint32_t)(ns - t0 < 64 ? ns - t0 : 64) - 1u;  // last active lane
  int64_t g = 0, off = 0, d = 0, q = 0;
  if (active) {
    g = block_of_dim(slot_off, nb, t);
    off = block_off[g];
    d = block_off[g + 1] - off;
    q = t - slot_off[g];
  }
  const int64_t j0 = 4 * q;
  // this lane's dims: quad q's (1..4), none for a group's last slot or lane 63
  const int cnt = active && lane < 63u && j0 < d ? (int)(d - j0 < 4 ? d - j0 : 4) : 0;
  // the wave's run of groups [g_first, g_last]
  const int64_t g_first = __shfl(g, 0, 64);
  const int64_t g_last = __shfl(g, (int)last, 64);
  const int64_t run = g_last - g_first + 1;
  const uint32_t L = __builtin_amdgcn_readfirstlane((uint32_t)(run < 65 ? run : 65));
  const bool shared_keys = L <= 64u;
  const uint32_t spw = shared_keys ? 64u / L : 1u;       // steps per key window
  const uint32_t gi = active ? (uint32_t)(g - g_first) : 0u;
  const uint32_t ds_lane = shared_keys ? lane / L : 0u;  // this lane's (step, group) of a window
  const uint32_t gj_lane = lane - ds_lane * L;
  const int32_t seed_own = active ? sd.of(g) : 0;
  const int32_t seed_win =
      shared_keys && ds_lane < spw ? sd.of(g_first + gj_lane) : 0;  // g_first + gj_lane <= g_last
  float ls, ss;  // wave-uniform: the standard proposal's shard
  shard_consts(0.0f, 1.0f, nst, sdiv, rho, ls, ss);
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sample = tf.zeros (:143)
  bool bad = false;
  PhiloxStream kw{0u, 0u, 0u, 0u};
  uint32_t ws = 0;  // first step of the key window
  for (int s0 = 0; s0 < n_steps; s0 += U) {
    const int nu = n_steps - s0 < U ? n_steps - s0 : U;  // wave-uniform
    PhiloxStream ku[U];
    uint64_t k0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // keys and rows first: the branches stay out of the arithmetic
      const int s = s0 + u < n_steps ? s0 + u : n_steps - 1;
      if (shared_keys) {
        if ((uint32_t)s == ws + spw || s == 0) {  // wave-uniform
          ws = (uint32_t)s;
          kw = generate_key(step_seed(seed_win, (int32_t)(ws + ds_lane)), 42);
        }
        const int src = (int)(((uint32_t)s - ws) * L + gi);
        ku[u] = PhiloxStream{
            (uint32_t)__shfl((int)kw.k0, src, 64), (uint32_t)__shfl((int)kw.k1, src, 64),
            (uint32_t)__shfl((int)kw.c2, src, 64), (uint32_t)__shfl((int)kw.c3, src, 64)};
      } else {
        ku[u] = generate_key(step_seed(seed_own, s), 42);
      }
      int64_t n = active ? (int64_t)idx[g * n_steps + s] : 0;
      if (n < 0 || n >= n_cand) {  // NaN for the whole group, as in k_decode
        bad = true;
        n = 0;
      }
      k0[u] = (uint64_t)n * (uint64_t)d;
    }
    float zz[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t r = (uint32_t)(k0[u] & 3u);
      const F4 z = normal4_dev(ku[u], (k0[u] >> 2) + (uint64_t)q, logtab);
      // the next slot's block (an owning lane's next lane is its group's next slot)
      const float na = __shfl_down(z.a, 1, 64), nb1 = __shfl_down(z.b, 1, 64),
                  nc = __shfl_down(z.c, 1, 64);
      zz[u][0] = r == 0 ? z.a : (r == 1 ? z.b : (r == 2 ? z.c : z.d));
      zz[u][1] = r == 0 ? z.b : (r == 1 ? z.c : (r == 2 ? z.d : na));
      zz[u][2] = r == 0 ? z.c : (r == 1 ? z.d : (r == 2 ? na : nb1));
      zz[u][3] = r == 0 ? z.d : (r == 1 ? na : (r == 2 ? nb1 : nc));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < nu) {
#pragma unroll
        for (int w = 0; w < 4; ++w)
          v[w] = v[w] + shard_sample(ls, ss, zz[u][w]);  // :153 sample + row indices[i]
      }
    }
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < cnt) {
      const int64_t i = off + j0 + w;
      const float x = bad ? __builtin_nanf("") : v[w];
      out[i] = destandardise_1(x, dst_loc[i], dst_scale[i]);  // :362
    }
  }
}

// ---------------------------------------------------------------------------
// misc.py:3-17 materialised: out[n*d+j] = loc[j] + scale[j] * (z*1 + 0).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_stateless_normal_sample(
    const float* __restrict__ loc, const float* __restrict__ scale, int64_t d, int64_t total,
    int32_t seed, float* __restrict__ out) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  const PhiloxStream st = generate_key(seed, 42);
  const int64_t ngrp = (total + 3) >> 2;
  for (int64_t G = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; G < ngrp;
       G += (int64_t)gridDim.x * blockDim.x) {
    const F4 z = normal4_dev(st, (uint64_t)G, logtab);
    const float zz[4] = {z.a, z.b, z.c, z.d};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int64_t f = 4 * G + w;
      if (f < total) {
        const int64_t j = f % d;
        const float r = zz[w] * 1.0f + 0.0f;  // rnd * stddev + mean
        const float sc = scale[j];
        out[f] = shard_sample(loc[j], sc, r);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Grouped-wrapper elementwise pieces.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_standardise(
    const float* __restrict__ q_loc, const float* __restrict__ q_scale,
    const float* __restrict__ p_loc, const float* __restrict__ p_scale, int64_t n,
    float* __restrict__ t_loc, float* __restrict__ t_scale) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    standardise_1(q_loc[i], q_scale[i], p_loc[i], p_scale[i], t_loc[i], t_scale[i]);
  }
}

__global__ void __launch_bounds__(256) k_kl_normal_normal(
    const float* __restrict__ a_loc, const float* __restrict__ a_scale,
    const float* __restrict__ b_loc, const float* __restrict__ b_scale, int64_t n,
    float* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = kl_normal_normal_1(a_loc[i], a_scale[i], b_loc[i], b_scale[i]);
}

// The grouped coder's first launch (coded_greedy_sampler.py:193-201): the
// standardised target (k_standardise's expressions), the per-dim KL
// (k_kl_normal_normal's), the standard prior's zeros and ones, and zeroed
// partition counters (nz u64 at zinfo), in one pass over the inputs.
__global__ void __launch_bounds__(256) k_grouped_prep(
    const float* __restrict__ q_loc, const float* __restrict__ q_scale,
    const float* __restrict__ p_loc, const float* __restrict__ p_scale, int64_t n,
    float* __restrict__ t_loc, float* __restrict__ t_scale, float* __restrict__ kl,
    float* __restrict__ zeros, float* __restrict__ ones, unsigned long long* __restrict__ zinfo,
    int nz) {
  if (blockIdx.x == 0 && (int)threadIdx.x < nz) zinfo[threadIdx.x] = 0ull;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float ql = q_loc[i], qs = q_scale[i], pl = p_loc[i], ps = p_scale[i];
    standardise_1(ql, qs, pl, ps, t_loc[i], t_scale[i]);
    kl[i] = kl_normal_normal_1(ql, qs, pl, ps);
    zeros[i] = 0.0f;
    ones[i] = 1.0f;
  }
}

// The grouped importance coder's first launch (coded_importance_sampler.py:
// 137-148, 150, 160-163) in one pass: the standardised target (k_standardise's
// expressions), the per-dim KL (k_kl_normal_normal's) and the outlier test
// (k_imp_outliers': bits = kl / np.float32(log 2) <= limit, NaN an outlier,
// outliers standardised to N(0, 1)), the standard prior's zeros and ones, the
// KL of the (masked) standardised target against N(0, 1), which is what the
// partition and the plan read, and, for the outlier dims only, the target draw
// q_loc + q_scale z (:150; z element j of stateless_normal([1, D], [seed - 1,
// 42]), k_stateless_normal_sample's expressions).  A batch of
// items (item_off: device [n_items + 1], seed1: device [n_items] of
// seed - 1) numbers each item's dims from 0 in its own stream; item_off ==
// nullptr: one item with seed - 1 = seed1_one.
__global__ void __launch_bounds__(256) k_imp_grouped_prep(
    const float* __restrict__ q_loc, const float* __restrict__ q_scale,
    const float* __restrict__ p_loc, const float* __restrict__ p_scale, int64_t n, float limit,
    const int64_t* __restrict__ item_off, const int32_t* __restrict__ seed1, int64_t n_items,
    int32_t seed1_one, float* __restrict__ t_loc, float* __restrict__ t_scale,
    uint8_t* __restrict__ keep, float* __restrict__ zeros, float* __restrict__ ones,
    float* __restrict__ kl2, float* __restrict__ tsamp) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float ql = q_loc[i], qs = q_scale[i], pl = p_loc[i], ps = p_scale[i];
    float tl, ts;
    standardise_1(ql, qs, pl, ps, tl, ts);
    const float kl = kl_normal_normal_1(ql, qs, pl, ps);
    const float bits = kl / 0.6931472f;
    const bool k = bits <= limit;
    if (!k) {
      tl = 0.0f;
      ts = 1.0f;
      int64_t j = i;
      int32_t sd = seed1_one;
      if (item_off) {  // item of dim i: last it with item_off[it] <= i
        int64_t lo = 0, hi = n_items;
        while (hi - lo > 1) {
          const int64_t mid = (lo + hi) >> 1;
          if (item_off[mid] <= i) lo = mid; else hi = mid;
        }
        j = i - item_off[lo];
        sd = seed1[lo];
      }
      const F4 z = normal4_dev(generate_key(sd, 42), (uint64_t)j >> 2, logtab);
      const float r = f4_word(z, (uint32_t)j & 3u) * 1.0f + 0.0f;  // rnd * stddev + mean
      tsamp[i] = shard_sample(ql, qs, r);
    }
    t_loc[i] = tl;
    t_scale[i] = ts;
    keep[i] = k ? 1 : 0;
    zeros[i] = 0.0f;
    ones[i] = 1.0f;
    kl2[i] = kl_normal_normal_1(tl, ts, 0.0f, 1.0f);
  }
}

__global__ void __launch_bounds__(256) k_destandardise(const float* sample,
                                                       const float* __restrict__ p_loc,
                                                       const float* __restrict__ p_scale,
                                                       int64_t n, float* out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    out[i] = destandardise_1(sample[i], p_loc[i], p_scale[i]);
  }
}

// ---------------------------------------------------------------------------
// Diagnostics: device transcendentals over explicit inputs.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_selftest_bm(uint32_t m0, int64_t count,
                                                     float* __restrict__ rad,
                                                     float* __restrict__ sn,
                                                     float* __restrict__ cs) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t m = m0 + (uint32_t)i;
    rad[i] = bm_radius_dev(m, logtab);
    float s, c;
    sincosf_pos(bm_angle_dev(m), s, c);
    sn[i] = s;
    cs[i] = c;
  }
}

__global__ void __launch_bounds__(256) k_selftest_screen(uint32_t m0, int64_t count,
                                                         float* __restrict__ rad,
                                                         float* __restrict__ sn,
                                                         float* __restrict__ cs) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t m = m0 + (uint32_t)i;
    rad[i] = bm_qradius_screen(m);  // r~ / sqrt(2 ln 2)
    float s, c;
    bm_sincos_screen(m, s, c);
    sn[i] = s;
    cs[i] = c;
  }
}

// out[w] = max over the 64 inputs of wave w (wave_max_f32, the DPP reduction
// the pruned kernel shares tau with)
__global__ void __launch_bounds__(256) k_selftest_wave_max(const float* __restrict__ x, int64_t nw,
                                                           float* __restrict__ out) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const float v = w < nw ? x[w * 64 + (threadIdx.x & 63)] : -__builtin_inff();
  const float m = wave_max_f32(v);
  if (w < nw && (threadIdx.x & 63) == 0) out[w] = m;
}

__global__ void __launch_bounds__(256) k_selftest_logf(const float* __restrict__ x, int64_t n,
                                                       float* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = logf_full(x[i], kLogTabConst);
}

__global__ void __launch_bounds__(256) k_selftest_div(const float* __restrict__ a,
                                                      const float* __restrict__ b, int64_t n,
                                                      float* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float y = 1.0f / b[i];
    out[i] = div_rn_markstein(a[i], b[i], y);
  }
}

// ---------------------------------------------------------------------------
// Host-side launchers.
// ---------------------------------------------------------------------------

static SeedSpec seeds_of(const EncodeArgs& a) {
  return SeedSpec{a.seed, a.block_id_base, a.seeds};
}

// float4 access needs 16-byte aligned bases (callers may pass offset views);
// with q4_shape (cwq_dispatch.h) the condition of the float4 kernels
static bool aligned16(const void* a, const void* b, const void* c) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
}

hipError_t launch_prep_dims(const float* t_scale, const float* p_loc, const float* p_scale,
                            int64_t n, int n_steps, float rho, float* loc_s, float* scale_s,
                            float* lognorm, float* out_sample, unsigned long long* keys,
                            int64_t nb, hipStream_t stream) {
  if (n <= 0 && nb <= 0) return hipSuccess;
  const float nst = (float)n_steps;
  const float sdiv = (float)__builtin_sqrt((double)n_steps);
  hipLaunchKernelGGL(k_prep_dims, dim3(grid_for(n > nb ? n : nb, 256, 65536)), dim3(256), 0,
                     stream, t_scale, p_loc, p_scale, n, nst, sdiv, rho, loc_s, scale_s, lognorm,
                     out_sample, keys, nb);
  return hipGetLastError();
}

template <int DC, bool STEP0>
static void launch_eval_t(const EncodeArgs& a, int step, hipStream_t stream) {
  const int64_t ntiles = a.nb * a.tiles_per_block;
  const unsigned grid = (unsigned)(ntiles < (1LL << 30) ? ntiles : (1LL << 30));
  hipLaunchKernelGGL((k_encode_eval<DC, STEP0>), dim3(grid), dim3(256), 0, stream, a.t_loc,
                     a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample, a.block_off, a.ud,
                     ntiles, a.tiles_per_block, a.cand_per_tile, a.n_cand, seeds_of(a),
                     step, a.keys);
}

// k_encode_prune's allow_screen: bit 0 the screening pass, bits 1-2 the tau
// guess (0 off, 1 on, 2 every screened tile retried: tests)
static int prune_screen_arg(const EncodeArgs& a) {
  const int scr = a.prune >= 2 ? 1 : 0;
  const int gm = a.tau_guess >= 0 ? (a.tau_guess & 3) : scr;
  return scr | (gm << 1);
}

template <int D, bool STEP0>
static void launch_prune_t(const EncodeArgs& a, int step, hipStream_t stream) {
  // grid of 256 CUs x 6 resident workgroups x 256; each workgroup loops over
  // its tiles (C4: 2.5 each).  Many more workgroups than resident slots keep
  // the SIMDs busy while a workgroup sets up its next tile: 1,536 (exactly
  // resident) was 15% slower on C4, 12,288 2%, 98,304 0.5%; one tile per
  // workgroup (1M) 0.5% (tools/variants.sh pg*)
#ifndef CWQ_PRUNE_GRID
#define CWQ_PRUNE_GRID (256 * 6 * 256)
#endif
  constexpr int64_t kPruneGrid = CWQ_PRUNE_GRID;
  const int64_t ntiles = a.nb * a.tiles_per_block;
#ifndef CWQ_TILE_INTERLEAVE
#define CWQ_TILE_INTERLEAVE 1
#endif
  // tau seeding: when a block spans several tiles, most of them
  // run at once and each would warm its threshold up from -inf.  A first launch
  // scores the block's first 2^CWQ_SEED_LOG2 candidates in small tiles; their
  // exact best keys land in keys[g], and every tile of the main launch starts
  // from that value (an actual row's exact value, so never above the block's
  // best).  The sample's rows are scored again by the main launch: its keys
  // are exact, so the final argmax is unchanged.
#ifndef CWQ_SEED_LOG2
#define CWQ_SEED_LOG2 0  // off: measured no gain
#endif
#ifndef CWQ_SEED_TILE
#define CWQ_SEED_TILE 4096
#endif
#ifndef CWQ_SEED_MIN_TPB
#define CWQ_SEED_MIN_TPB 2
#endif
  const int64_t seed_n = CWQ_SEED_LOG2 > 0 ? ((int64_t)1 << CWQ_SEED_LOG2) : 0;
  const bool seeded = CWQ_TILE_INTERLEAVE && seed_n > 0 && a.tiles_per_block >= CWQ_SEED_MIN_TPB &&
                      a.n_cand >= 4 * seed_n;
  if (seeded) {
    const int64_t cpt_s = seed_n < CWQ_SEED_TILE ? (seed_n > 0 ? seed_n : 1) : CWQ_SEED_TILE;
    const int64_t nt_s = a.nb * (seed_n / cpt_s);
    hipLaunchKernelGGL((k_encode_prune<D, STEP0, true, false>),
                       dim3((unsigned)(nt_s < kPruneGrid ? nt_s : kPruneGrid)), dim3(256), 0,
                       stream, a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample,
                       nt_s, seed_n / cpt_s, cpt_s, seed_n, seeds_of(a), step,
                       prune_screen_arg(a), a.keys, seed_n / cpt_s, 1, nullptr, DeferArgs<0>{});
  }
  // tile queue (k_encode_prune): a persistent grid of CWQ_QUEUE_GRID workgroups
  // draws tiles from a counter in the workspace, zeroed here before the launch;
  // for which launches: takes_tile_queue (cwq_dispatch.h)
#ifndef CWQ_TILE_QUEUE
#define CWQ_TILE_QUEUE 1
#endif
  // Deferral (k_encode_prune FORM 1 and 2, k_score_survivors): for one tile per
  // block, where the caller's workspace has the regions (defer_ws) and the
  // screening pass is on.  Three more launches cost a fixed 0.15 ms or so (the
  // launch over an empty deferred list alone is 1,536 workgroups that start and
  // leave), against 1.3% of the screening kernel's time, so only for calls of
  // at least CWQ_DEFER_MIN_WORK candidate dims (rows x d): 16,384 blocks of
  // d = 64 at 16 bits, 12 ms, were 1.2% faster, of d = 32, 4.7 ms, 2% slower
  // (DESIGN.md 4 "Deferral"); C4 has 2^41.  defer_mode >= 1 (tests) takes it
  // at any size.
#ifndef CWQ_DEFER
#define CWQ_DEFER 1
#endif
#ifndef CWQ_DEFER_MIN_WORK
#define CWQ_DEFER_MIN_WORK (1LL << 36)
#endif
  const int64_t tile_rows = a.cand_per_tile < a.n_cand ? a.cand_per_tile : a.n_cand;
  bool defer = CWQ_DEFER && a.defer_surv && a.defer_count && a.defer_list && a.defer_dcount &&
               a.defer_mode != 0 && (prune_screen_arg(a) & 1) && a.tiles_per_block == 1 &&
               !seeded && ntiles < (1LL << 31) &&
               // (the product can pass 2^63: tile_rows D <= 2^36 divides instead)
               (a.defer_mode >= 1 || ntiles >= (CWQ_DEFER_MIN_WORK + tile_rows * D - 1) / (tile_rows * D));
  // the queue's grid: every resident slot of the form that runs
  const int64_t queue_grid = defer ? 256 * (int64_t)CWQ_DEFER_MIN_WAVES : (int64_t)CWQ_QUEUE_GRID;
  uint32_t* tq = nullptr;
  if (CWQ_TILE_QUEUE && a.tq != nullptr && takes_tile_queue(ntiles, a.cand_per_tile, queue_grid))
    tq = a.tq;
  // one launch zeroes the deferred list's length and the queue's counter
  if (defer || tq)
    hipLaunchKernelGGL(k_counters_reset, dim3(1), dim3(64), 0, stream,
                       defer ? a.defer_dcount : nullptr, tq);
  auto qgrid = [&](int64_t nt) -> unsigned {
    const int64_t cap = tq ? queue_grid : kPruneGrid;
    return (unsigned)(nt < cap ? nt : cap);
  };
  // The loop variant (CWQ_PARK_COMPLETE): tiles of CWQ_PARK_MIN_ROWS rows or
  // more take the instance whose completed rows park.  A parked row idles for
  // up to CWQ_TAU_SHARE_MASK iterations, which is nothing where a handful of a
  // tile's rows complete (C4: 15 of 65,536) and a cliff where most do, as in
  // tiles of a few rows per lane, whose tau has no time to rise, and in rows of
  // two units (d = 8), which complete whenever their first unit does not drop
  // them.  Measured on one-tile blocks: d = 32 at 4,096 rows
  // +0.2%, at 8,192 -0.8%, at 16,384 -1.9%; d = 64 at 8,192 -1.5%; d = 16 at
  // 8,192 +1.5%, at 16,384 -0.3%; d = 8 at 8,192 +1.7%.  Parking pays from
  // about 2^16 Philox blocks per tile on, so the threshold is stated in rows of
  // a d = 32 tile and scaled by 32 / d.  The rows are those of a full tile; the
  // tail tiles of such a launch are a quarter of it and start from keys[g], the
  // tiles before them having finished.
  auto with_park = [&](auto launch) {
    if constexpr (CWQ_PARK_COMPLETE && D >= CWQ_PARK_MIN_D) {
      if (tile_rows * D >= (int64_t)CWQ_PARK_MIN_ROWS * 32) return launch(std::true_type{});
    }
    return launch(std::false_type{});
  };
  if (CWQ_TILE_INTERLEAVE && (a.tiles_per_block > 1 || seeded)) {
    // tail: the last tile of each block's few last tiles split in CWQ_TAIL_SPLIT,
    // about two resident rounds (1,536 workgroups) of short tiles at the end
#ifndef CWQ_TAIL_SPLIT
#define CWQ_TAIL_SPLIT 4
#endif
    const int64_t tpb = a.tiles_per_block;
    int64_t from = tpb, div = 1;
    if (CWQ_TAIL_SPLIT > 1 && tpb >= 2 && a.cand_per_tile % (256 * CWQ_TAIL_SPLIT) == 0) {
      div = CWQ_TAIL_SPLIT;
      int64_t L = (2 * 1536 + div * a.nb - 1) / (div * a.nb);
      L = L < tpb / 2 ? L : tpb / 2;
      from = tpb - L;
    }
    const int64_t tpb2 = from + (tpb - from) * div;
    const int64_t nt2 = a.nb * tpb2;
    with_park([&](auto park) {
      hipLaunchKernelGGL((k_encode_prune<D, STEP0, true, decltype(park)::value>),
                         dim3(qgrid(nt2)), dim3(256), 0,
                         stream, a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample,
                         nt2, tpb2, a.cand_per_tile, a.n_cand, seeds_of(a), step,
                         prune_screen_arg(a), a.keys, from, (int)div, tq, DeferArgs<0>{});
    });
  } else if (defer) {
    // Deferral: the screening-only form lists each block's rows
    // that reach its tau, k_score_survivors scores them, and the full kernel
    // runs over the blocks the first launch put on the deferred list, whose
    // length it reads on the device: a fixed grid, which finds the list empty
    // as a rule, and no wait on the host.
    const int q = a.defer_mode == 2 ? -1 : (a.defer_mode == 3 ? 0 : (int)kDeferQ);
    static_assert(kDeferQ >= 0 && kDeferQ <= kDeferSlots, "Q slots per block");
    with_park([&](auto park) {
      hipLaunchKernelGGL((k_encode_prune<D, STEP0, false, decltype(park)::value, 1>),
                         dim3(qgrid(ntiles)), dim3(256), 0,
                         stream, a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample,
                         ntiles, a.tiles_per_block, a.cand_per_tile, a.n_cand, seeds_of(a), step,
                         prune_screen_arg(a), a.keys, a.tiles_per_block, 1, tq,
                         DeferArgs<1>{a.defer_surv, a.defer_count, a.defer_list, a.defer_dcount, q});
    });
    constexpr int64_t kRowsPerWg = 4 * ((64 / (D / 4)) < 8 ? (64 / (D / 4)) : 8);
    hipLaunchKernelGGL((k_score_survivors<D, STEP0>),
                       dim3((unsigned)((a.nb + kRowsPerWg - 1) / kRowsPerWg)), dim3(256), 0, stream,
                       a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample, a.nb,
                       seeds_of(a), step, (const uint32_t*)a.defer_surv,
                       (const uint32_t*)a.defer_count, a.keys);
    with_park([&](auto park) {
      hipLaunchKernelGGL((k_encode_prune<D, STEP0, false, decltype(park)::value, 2>),
                         dim3((unsigned)(ntiles < 1536 ? ntiles : 1536)), dim3(256), 0,
                         stream, a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample,
                         ntiles, a.tiles_per_block, a.cand_per_tile, a.n_cand, seeds_of(a), step,
                         prune_screen_arg(a), a.keys, a.tiles_per_block, 1, nullptr,
                         DeferArgs<2>{a.defer_surv, a.defer_count, a.defer_list, a.defer_dcount, q});
    });
  } else {
    with_park([&](auto park) {
      hipLaunchKernelGGL((k_encode_prune<D, STEP0, false, decltype(park)::value>),
                         dim3(qgrid(ntiles)), dim3(256), 0,
                         stream, a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample,
                         ntiles, a.tiles_per_block, a.cand_per_tile, a.n_cand, seeds_of(a), step,
                         prune_screen_arg(a), a.keys, a.tiles_per_block, 1, tq, DeferArgs<0>{});
    });
  }
}

template <bool STEP0>
static void launch_prune_csr(const EncodeArgs& a, bool coop, int step, hipStream_t stream) {
  // own tiling: ~8192 tiles of >= 1024 candidates; tiles of a block share tau
  // through gtau, and later tiles start from it.  With few rows per lane
  // (EncodePlan::coop: a few large groups) long rows are walked cooperatively
  // by 16 lanes instead, in tiles of >= 128 candidates.
  int64_t tpb, max_tpb;
  if (coop) {
    tpb = (CWQ_CSR_COOP_TILES + a.nb - 1) / a.nb;
    max_tpb = a.n_cand / CWQ_CSR_COOP_TILE > 1 ? a.n_cand / CWQ_CSR_COOP_TILE : 1;
  } else {
    tpb = (CWQ_CSR_TILES + a.nb - 1) / a.nb;
    max_tpb = a.n_cand / CWQ_CSR_TILE > 1 ? a.n_cand / CWQ_CSR_TILE : 1;
  }
  tpb = tpb < max_tpb ? tpb : max_tpb;
  const int64_t cpt = (a.n_cand + tpb - 1) / tpb;
  tpb = (a.n_cand + cpt - 1) / cpt;  // no tile may start at or past n_cand
#if CWQ_COOP_CLASS_TILES
  // one-class tiles come in fours (the kernel skips a residue tile that gets
  // no row of a short last chunk)
  if (coop && tpb >= 4) tpb = (tpb + 3) & ~(int64_t)3;
#endif
  const int64_t ntiles = a.nb * tpb;
  const int64_t coop_min_d = coop ? (int64_t)CWQ_CSR_COOP_MIN_D : INT64_MAX;
#ifndef CWQ_PREP_SPLIT_MAX_NB
#define CWQ_PREP_SPLIT_MAX_NB 256
#endif
  // few blocks: one workgroup per class
  const unsigned cls_wgs = a.nb <= CWQ_PREP_SPLIT_MAX_NB ? 4 : 1;
  hipLaunchKernelGGL((k_csr_prep<STEP0>), dim3(grid_for(a.nb, 1, 65536), cls_wgs), dim3(256), 0,
                     stream, a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample,
                     a.block_off, a.ud, a.nb, a.sab, a.cdim, a.bpre, a.ordu, a.grp, a.gtau,
                     a.abp, (int64_t)CWQ_CSR_LDS_DIMS, coop_min_d);
  constexpr int64_t kGrid = 1 << 20;
  const unsigned grid = (unsigned)(ntiles < kGrid ? ntiles : kGrid);
  if (coop)
    hipLaunchKernelGGL((k_encode_prune_csr<STEP0, true>), dim3(grid), dim3(256), 0, stream,
                       a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample,
                       a.block_off, a.ud, ntiles, tpb, cpt, a.n_cand, seeds_of(a),
                       step, (const float2*)a.sab, (const float*)a.bpre,
                       (const uint32_t*)a.ordu, (const float4*)a.grp, a.gtau, a.keys,
                       coop_min_d, (const float4*)a.abp);
  else
    hipLaunchKernelGGL((k_encode_prune_csr<STEP0, false>), dim3(grid), dim3(256), 0, stream,
                       a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample,
                       a.block_off, a.ud, ntiles, tpb, cpt, a.n_cand, seeds_of(a),
                       step, (const float2*)a.sab, (const float*)a.bpre,
                       (const uint32_t*)a.ordu, (const float4*)a.grp, a.gtau, a.keys,
                       coop_min_d, (const float4*)a.abp);
}

// The small pipeline (k_small_*): constants, persistent screen, finalize.  The
// launches also write the step's indices and sample (EncodePlan::self_finalizing).
template <bool STEP0>
static void launch_small_pipe(const EncodeArgs& a, int step, hipStream_t stream) {
  SmallRec* rec = (SmallRec*)a.slist;
  float2* pab = const_cast<float2*>(a.pre_ab);  // by absolute dim (launch_encode)
  const float nst = (float)a.n_steps;
  const float sdiv = (float)__builtin_sqrt((double)a.n_steps);
  const unsigned pgrid = grid_for(a.nb, kSmallPrepBlocks, 1u << 31);
  if (STEP0)
    hipLaunchKernelGGL(k_small_prep1<true>, dim3(pgrid), dim3(CWQ_PREP1_THREADS), 0, stream, a.t_loc,
                       a.t_scale, a.p_loc, a.p_scale, nst, sdiv, a.rho, a.loc_s, a.scale_s,
                       a.lognorm, a.out_sample, a.block_off, a.ud, a.nb, seeds_of(a), step,
                       pab, rec, a.sdmap);
  else
    hipLaunchKernelGGL(k_small_prep1<false>, dim3(pgrid), dim3(CWQ_PREP1_THREADS), 0, stream, a.t_loc,
                       a.t_scale, a.p_loc, a.p_scale, nst, sdiv, a.rho, a.loc_s, a.scale_s,
                       a.lognorm, a.out_sample, a.block_off, a.ud, a.nb, seeds_of(a), step,
                       pab, rec, a.sdmap);
  const int64_t nu = a.nb;
  for (int64_t u0 = 0; u0 < nu; u0 += (int64_t)1 << 30)
    hipLaunchKernelGGL((k_small_one<STEP0>),
                       dim3((unsigned)(nu - u0 < (1LL << 30) ? nu - u0 : (1LL << 30))),
                       dim3(64), 0, stream, a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm,
                       a.out_sample, rec, a.pre_ab, a.nb, u0, a.n_cand, step, a.n_steps,
                       a.out_idx);
  const unsigned dgrid = grid_for(a.total_dims > a.nb ? a.total_dims : a.nb, 256, 16384);
  hipLaunchKernelGGL((k_small_finalize<STEP0>), dim3(dgrid), dim3(256), 0, stream, a.loc_s,
                     a.scale_s, rec, a.sdmap, a.out_idx, step, a.n_steps, a.block_off, a.ud,
                     a.nb, a.out_sample, step == a.n_steps - 1 ? a.ds_out : nullptr, a.ds_loc,
                     a.ds_scale);
}

// The three-kernel small-candidate path (k_small_prep/screen/survivors).
template <bool STEP0>
static void launch_small_three(const EncodeArgs& a, int step, hipStream_t stream) {
  const int64_t ntiles = a.nb * a.tiles_per_block;
  hipLaunchKernelGGL((k_small_prep<STEP0>), dim3(grid_for(a.nb, 4 * 64, 16384)), dim3(256), 0,
                     stream, a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm, a.out_sample,
                     a.block_off, a.ud, a.nb, seeds_of(a), step, a.sab, a.bpre, a.grp, a.gtau,
                     a.ordu);
  hipLaunchKernelGGL((k_small_screen<STEP0>), dim3(grid_for(ntiles, 4, 1u << 20)),
                     dim3(256), 0, stream, a.block_off, a.ud, ntiles, a.tiles_per_block,
                     a.cand_per_tile, a.n_cand, seeds_of(a), step, (const float2*)a.sab,
                     (const float*)a.bpre, a.grp, a.gtau, a.ordu, a.slist);
  hipLaunchKernelGGL((k_small_survivors<STEP0>), dim3(grid_for(a.nb, 4 * 64, 4096)),
                     dim3(256), 0, stream, a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm,
                     a.out_sample, a.block_off, a.ud, a.nb, a.n_cand, seeds_of(a), step,
                     (const float4*)a.grp, (const uint32_t*)a.gtau, (const uint32_t*)a.ordu,
                     (const uint2*)a.slist, (const float*)a.bpre, a.keys);
}

// A wave per candidate row (k_encode_rows_wave): four rows per workgroup
// iteration, at most CWQ_ROWS_WAVE_WGS workgroups (8 per CU: DESIGN.md 4e).
#ifndef CWQ_ROWS_WAVE_WGS
#define CWQ_ROWS_WAVE_WGS (8 * 256)
#endif
template <bool STEP0>
static void launch_rows_wave(const EncodeArgs& a, int step, hipStream_t stream) {
  int n_bits = 0;
  while (((int64_t)1 << n_bits) < a.n_cand) ++n_bits;
  const int64_t rows = a.nb << n_bits;  // nb <= 2^31 and n_bits <= 30 (the C ABI's checks)
  hipLaunchKernelGGL((k_encode_rows_wave<STEP0>), dim3(grid_for(rows, 4, CWQ_ROWS_WAVE_WGS)),
                     dim3(256), 0, stream, a.t_loc, a.t_scale, a.loc_s, a.scale_s, a.lognorm,
                     a.out_sample, a.block_off, a.ud, a.nb, n_bits, seeds_of(a), step, a.keys);
}

static EncodeShape shape_of(const EncodeArgs& a) {
  return {a.block_off != nullptr, a.ud, a.max_d, a.nb, a.n_cand, a.prune, a.rows_wave};
}

// Scoring launches of one step on the plan's path (encode_plan, cwq_dispatch.h).
template <bool STEP0>
static void launch_eval_dc(const EncodeArgs& a, const EncodePlan& plan, int step,
                           hipStream_t stream) {
  switch (plan.path) {
    case EncodePath::RowsWave: return launch_rows_wave<STEP0>(a, step, stream);
    case EncodePath::UniformPruned:
      switch (a.ud) {
        case 8: return launch_prune_t<8, STEP0>(a, step, stream);
        case 16: return launch_prune_t<16, STEP0>(a, step, stream);
        case 24: return launch_prune_t<24, STEP0>(a, step, stream);
        case 32: return launch_prune_t<32, STEP0>(a, step, stream);
        case 40: return launch_prune_t<40, STEP0>(a, step, stream);
        case 48: return launch_prune_t<48, STEP0>(a, step, stream);
        case 56: return launch_prune_t<56, STEP0>(a, step, stream);
        default: return launch_prune_t<64, STEP0>(a, step, stream);  // the plan admits no other
      }
    case EncodePath::CsrPruned: return launch_prune_csr<STEP0>(a, plan.coop, step, stream);
    case EncodePath::SmallPipe: return launch_small_pipe<STEP0>(a, step, stream);
    case EncodePath::SmallThree: return launch_small_three<STEP0>(a, step, stream);
    case EncodePath::Eval:
      if (a.block_off == nullptr) {
        switch (a.ud) {
          case 8: return launch_eval_t<8, STEP0>(a, step, stream);
          case 16: return launch_eval_t<16, STEP0>(a, step, stream);
          case 32: return launch_eval_t<32, STEP0>(a, step, stream);
          default: break;
        }
      }
      return launch_eval_t<0, STEP0>(a, step, stream);
  }
}

// One step's scoring launches on their own (backfitting, cwq_backfit.hip).
// Nothing in the launchers above is tied to the step's number: the tile queue
// word is zeroed before every launch that uses it, INTER follows the tiling,
// and the kernels take the step only for the stream's seed.  k_small_prep1<FIRST>
// is tied to step 0, but the small pipeline is excluded here (keys_only).
hipError_t launch_score_step(const EncodeArgs& a_in, int step, hipStream_t stream) {
  if (a_in.nb <= 0) return hipSuccess;
  EncodeArgs a = a_in;
  a.pre_ab = a.sab;
  EncodeShape shape = shape_of(a);
  shape.keys_only = true;
  const EncodePlan plan = encode_plan(shape);
  const bool screened = plan.path == EncodePath::CsrPruned || plan.path == EncodePath::SmallThree;
  if (plan.self_finalizing ||
      (screened && !(a.sab && a.cdim && a.bpre && a.ordu && a.grp && a.gtau && a.slist && a.sdmap)))
    return hipErrorInvalidValue;
  launch_eval_dc<false>(a, plan, step, stream);
  return hipGetLastError();
}

// The step loop of one block range on one stream: reset the argmax keys, score
// the candidates, finalize (index + best) -- steps are sequential per block.
static hipError_t encode_steps(const EncodeArgs& a, hipStream_t stream, bool events) {
  hipError_t e;
  const EncodePlan plan = encode_plan(shape_of(a));
  // the general finalize covers max(nb, dims of this block range) threads
#ifndef CWQ_FIN_MAX_WGS
#define CWQ_FIN_MAX_WGS 16384
#endif
  const unsigned fgrid_dims =
      grid_for(a.total_dims > a.nb ? a.total_dims : a.nb, 256, CWQ_FIN_MAX_WGS);
  for (int s = 0; s < a.n_steps; ++s) {
    // step 0's keys were zeroed by k_prep_dims (launch_encode); the small
    // pipeline keeps its argmax in registers and LDS and never reads keys
    if (s > 0 && !plan.self_finalizing) {
      hipLaunchKernelGGL(k_keys_reset, dim3(grid_for(a.nb, 256, 4096)), dim3(256), 0, stream,
                         a.keys, a.nb);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (events && s == 0 && a.ev_start) {
      e = hipEventRecord((hipEvent_t)a.ev_start, stream);
      if (e != hipSuccess) return e;
    }
    if (s == 0)
      launch_eval_dc<true>(a, plan, s, stream);
    else
      launch_eval_dc<false>(a, plan, s, stream);
    if (events && s == a.n_steps - 1 && a.ev_stop) {
      e = hipEventRecord((hipEvent_t)a.ev_stop, stream);
      if (e != hipSuccess) return e;
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (plan.self_finalizing) continue;
    if (q4_shape(a.block_off != nullptr, a.ud) &&
        aligned16(a.loc_s, a.scale_s, a.out_sample)) {
      const uint32_t qpb = (uint32_t)(a.ud / 4), bpw = 64u / qpb;
      hipLaunchKernelGGL(k_encode_finalize_q4, dim3(grid_for(a.nb, 4 * (int64_t)bpw, 1u << 20)),
                         dim3(256), 0, stream, (const float4*)a.loc_s, (const float4*)a.scale_s,
                         qpb, bpw, a.nb, seeds_of(a), s, a.n_steps, a.keys,
                         a.out_idx, (float4*)a.out_sample);
    } else {
      hipLaunchKernelGGL(k_encode_finalize, dim3(fgrid_dims), dim3(256), 0, stream, a.loc_s,
                         a.scale_s, a.block_off, a.ud, a.nb, seeds_of(a), s,
                         a.n_steps, a.keys, a.out_idx, a.out_sample);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Two library streams per device (created once per host thread) onto which a
// multi-step CSR encode forks: the two halves of the block range run their
// step loops concurrently, so one half's end-of-step tail (the last tiles of
// a step, and the finalize/prep launches between steps) overlaps the other
// half's work.  Fork and join are events on the caller's stream, so the call
// stays stream-ordered (and capturable) for the caller.
namespace {
constexpr int kMaxSplit = CWQ_ENCODE_SPLIT > 3 ? CWQ_ENCODE_SPLIT : 3;
constexpr int kMaxDevices = 16;
struct ForkStreams {
  bool ok = false;
  hipStream_t s[kMaxSplit] = {};
  hipStream_t cp[2] = {};  // copy streams of the pipelined batch coder (D2H, H2D)
  hipEvent_t fork = nullptr, join[kMaxSplit] = {};
  ~ForkStreams() {  // thread exit (the process's main thread: exit(), before HIP's teardown)
    if (!ok) return;
    for (int i = 0; i < kMaxSplit; ++i) {
      (void)hipStreamDestroy(s[i]);
      (void)hipEventDestroy(join[i]);
    }
    for (int i = 0; i < 2; ++i) (void)hipStreamDestroy(cp[i]);
    (void)hipEventDestroy(fork);
  }
};
thread_local ForkStreams tl_fork[kMaxDevices];
// The helper streams of the device the caller's stream belongs to (not the
// thread's current device: a caller may enqueue onto another GPU's stream).
ForkStreams* fork_streams(hipStream_t stream) {
  int dev = 0;
  if (hipStreamGetDevice(stream, &dev) != hipSuccess || dev < 0 || dev >= kMaxDevices)
    return nullptr;
  ForkStreams& f = tl_fork[dev];
  if (!f.ok) {
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    if (cur != dev && hipSetDevice(dev) != hipSuccess) return nullptr;
    bool good = true;
    int made_s = 0, made_e = 0, made_c = 0;
    for (int i = 0; i < kMaxSplit && good; ++i) {
      good = hipStreamCreateWithFlags(&f.s[i], hipStreamNonBlocking) == hipSuccess;
      made_s += good;
      good = good && hipEventCreateWithFlags(&f.join[i], hipEventDisableTiming) == hipSuccess;
      made_e += good;
    }
    for (int i = 0; i < 2 && good; ++i) {
      good = hipStreamCreateWithFlags(&f.cp[i], hipStreamNonBlocking) == hipSuccess;
      made_c += good;
    }
    good = good && hipEventCreateWithFlags(&f.fork, hipEventDisableTiming) == hipSuccess;
    if (!good) {  // nothing half-made stays behind; the caller runs unsplit
      for (int i = 0; i < made_s; ++i) (void)hipStreamDestroy(f.s[i]);
      for (int i = 0; i < made_e; ++i) (void)hipEventDestroy(f.join[i]);
      for (int i = 0; i < made_c; ++i) (void)hipStreamDestroy(f.cp[i]);
    }
    if (cur != dev) (void)hipSetDevice(cur);
    if (!good) return nullptr;
    f.ok = true;
  }
  return &f;
}
}  // namespace

hipStream_t copy_stream(hipStream_t stream, int which) {
  ForkStreams* f = fork_streams(stream);
  return f && which >= 0 && which < 2 ? f->cp[which] : nullptr;
}

hipError_t launch_encode(const EncodeArgs& a_in, hipStream_t stream) {
  hipError_t e;
  EncodeArgs a = a_in;
  // the small pipeline's per-dim screening constants, by absolute dim offset: a
  // view of sab (the other paths' scratch) taken before a fork shifts it per part
  a.pre_ab = a.sab;
  const EncodeShape shape = shape_of(a);
  const EncodePlan plan = encode_plan(shape);  // of the whole call; encode_steps: of each part
  // a guard, not a dispatch input: the screened paths' arrays were given
  const bool screened = plan.path == EncodePath::CsrPruned ||
                        plan.path == EncodePath::SmallPipe || plan.path == EncodePath::SmallThree;
  if (screened && !(a.sab && a.cdim && a.bpre && a.ordu && a.grp && a.gtau && a.slist && a.sdmap))
    return hipErrorInvalidValue;
  if (plan.self_finalizing)
    e = hipSuccess;  // its step 0 does k_prep_dims' work in k_small_prep1
  else
    e = launch_prep_dims(a.t_scale, a.p_loc, a.p_scale, a.total_dims, a.n_steps, a.rho, a.loc_s,
                         a.scale_s, a.lognorm, a.out_sample, a.keys, a.nb, stream);
  if (e != hipSuccess) return e;
  if (a.nb == 0) return hipSuccess;
  // :292 destandardise after the last step: the small pipeline's finalize
  // does it, anything else one k_destandardise on the caller's stream
  const bool ds_after = a.ds_out != nullptr && !plan.self_finalizing;
  auto ds = [&]() -> hipError_t {
    if (!ds_after) return hipSuccess;
    return launch_destandardise(a.out_sample, a.ds_loc, a.ds_scale, a.total_dims, a.ds_out,
                                stream);
  };
  const int k = encode_fork_parts(shape, a.n_steps);
  ForkStreams* f = k > 1 ? fork_streams(stream) : nullptr;
  if (f == nullptr) {
    if ((e = encode_steps(a, stream, true)) != hipSuccess) return e;
    return ds();
  }
  // k parts of the block range: block-indexed arrays move by g0, the padded
  // per-block regions of the general kernel by 8 g0 / 12 g0 (their layout is
  // off + 8 g / off + 12 g with absolute dim offsets off).
  if (a.ev_start && (e = hipEventRecord((hipEvent_t)a.ev_start, stream)) != hipSuccess) return e;
  if ((e = hipEventRecord(f->fork, stream)) != hipSuccess) return e;
  int forked = 0;
  for (int i = 0; i < k && e == hipSuccess; ++i) {
    const int64_t g0 = a.nb * i / k, g1 = a.nb * (i + 1) / k;
    EncodeArgs p = a;
    p.block_off = a.block_off + g0;
    p.nb = g1 - g0;
    p.block_id_base = a.block_id_base + g0;
    if (a.seeds) p.seeds = a.seeds + g0;
    p.keys = a.keys + g0;
    if (a.tq) p.tq = a.tq + i;  // its own tile queue counter
    p.defer_surv = nullptr;  // (parts are CSR calls: no deferral, and one list counter)
    p.out_idx = a.out_idx + g0 * a.n_steps;
    if (a.sab) p.sab = a.sab + 8 * g0;
    if (a.bpre) p.bpre = a.bpre + 12 * g0;
    if (a.ordu) p.ordu = a.ordu + 12 * g0;
    if (a.grp) p.grp = a.grp + g0;
    if (a.gtau) p.gtau = a.gtau + g0 * CWQ_CSR_GTAU_STRIDE;
    // abp is indexed by absolute dim offset alone (csr_rec_base): unshifted
    if (a.slist) p.slist = a.slist + CWQ_SLIST_PER_BLOCK * g0;
    // sdmap is indexed by absolute dim offset (its values: the part's block numbers)
    if ((e = hipStreamWaitEvent(f->s[i], f->fork, 0)) != hipSuccess) break;
    forked = i + 1;
    e = encode_steps(p, f->s[i], false);
  }
  // join every stream that was forked, also after an error: the caller's
  // stream must not run ahead of (or free buffers under) work already queued
  for (int i = 0; i < forked; ++i) {
    hipError_t ej = hipEventRecord(f->join[i], f->s[i]);
    if (ej == hipSuccess) ej = hipStreamWaitEvent(stream, f->join[i], 0);
    if (ej != hipSuccess) {
      (void)hipStreamSynchronize(f->s[i]);  // last resort: drain it on the host
      if (e == hipSuccess) e = ej;
    }
  }
  if (e != hipSuccess) return e;
  if (a.ev_stop && (e = hipEventRecord((hipEvent_t)a.ev_stop, stream)) != hipSuccess) return e;
  return ds();
}

hipError_t launch_decode(const int32_t* idx, const float* p_loc, const float* p_scale,
                         const int64_t* block_off, int64_t ud, int64_t nb, int64_t total_dims,
                         int n_bits,
                         int n_steps, int32_t seed, float rho, int64_t block_id_base,
                         float* out_sample, hipStream_t stream) {
  // the kernel and its launch size: decode_plan alone (cwq_dispatch.h)
  const DecodePlan p = decode_plan(DecodeShape{block_off != nullptr, ud, nb, total_dims, n_steps,
                                               aligned16(p_loc, p_scale, out_sample)});
  if (p.workgroups == 0) return hipSuccess;
  const float nst = (float)n_steps;
  const float sdiv = (float)__builtin_sqrt((double)n_steps);
  switch (p.kernel) {
    case DecodeKernel::Q4Glds:
      hipLaunchKernelGGL(k_decode_q4_glds, dim3(p.workgroups), dim3(256), 0, stream, idx,
                         (const float4*)p_loc, (const float4*)p_scale, p.qpb, p.bpw, nb,
                         (int64_t)1 << n_bits, rho, seed, block_id_base, (float4*)out_sample);
      break;
    case DecodeKernel::Q4:
      hipLaunchKernelGGL(k_decode_q4, dim3(p.workgroups), dim3(256), 0, stream, idx,
                         (const float4*)p_loc, (const float4*)p_scale, p.qpb, p.bpw, nb, n_steps,
                         (int64_t)1 << n_bits, nst, sdiv, rho, seed, block_id_base,
                         (float4*)out_sample);
      break;
    case DecodeKernel::General:
      hipLaunchKernelGGL(k_decode, dim3(p.workgroups), dim3(256), 0, stream, idx, p_loc, p_scale,
                         block_off, ud, nb, n_steps, (int64_t)1 << n_bits, nst, sdiv, rho, seed,
                         block_id_base, out_sample);
      break;
  }
  return hipGetLastError();
}

hipError_t launch_decode_csr_q4(const int32_t* idx, const int64_t* block_off,
                                const int64_t* slot_off, int64_t nb, int64_t n_slots,
                                const int32_t* block_seeds, int n_bits, int n_steps, float rho,
                                const float* dst_loc, const float* dst_scale, float* out,
                                hipStream_t stream) {
  if (nb <= 0 || n_slots <= 0) return hipSuccess;
  const int64_t grid = ((n_slots + 62) / 63 + 3) / 4;  // a wave per 63 slots (k_decode_csr_q4)
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  const float nst = (float)n_steps;
  const float sdiv = (float)__builtin_sqrt((double)n_steps);
  hipLaunchKernelGGL(n_steps > 1 ? k_decode_csr_q4<2> : k_decode_csr_q4<1>, dim3((unsigned)grid),
                     dim3(256), 0, stream, idx, block_off,
                     slot_off, nb, n_slots, SeedSpec{0, 0, block_seeds}, n_steps,
                     (int64_t)1 << n_bits, nst, sdiv, rho, dst_loc, dst_scale, out);
  return hipGetLastError();
}

hipError_t launch_stateless_normal_sample(const float* loc, const float* scale, int64_t d,
                                          int64_t num_samples, int32_t seed, float* out,
                                          hipStream_t stream) {
  const int64_t total = d * num_samples;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_stateless_normal_sample, dim3(grid_for((total + 3) / 4, 256, 65536)),
                     dim3(256), 0, stream, loc, scale, d, total, seed, out);
  return hipGetLastError();
}

hipError_t launch_standardise(const float* q_loc, const float* q_scale, const float* p_loc,
                              const float* p_scale, int64_t n, float* t_loc, float* t_scale,
                              hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_standardise, dim3(grid_for(n, 256, 65536)), dim3(256), 0, stream, q_loc,
                     q_scale, p_loc, p_scale, n, t_loc, t_scale);
  return hipGetLastError();
}

hipError_t launch_kl(const float* q_loc, const float* q_scale, const float* p_loc,
                     const float* p_scale, int64_t n, float* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_kl_normal_normal, dim3(grid_for(n, 256, 65536)), dim3(256), 0, stream,
                     q_loc, q_scale, p_loc, p_scale, n, out);
  return hipGetLastError();
}

hipError_t launch_grouped_prep(const float* q_loc, const float* q_scale, const float* p_loc,
                               const float* p_scale, int64_t n, float* t_loc, float* t_scale,
                               float* kl, float* zeros, float* ones, unsigned long long* zinfo,
                               int nz, hipStream_t stream) {
  if (n <= 0 && nz <= 0) return hipSuccess;
  if (nz < 0 || nz > 256 || (nz > 0 && !zinfo)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_grouped_prep, dim3(n > 0 ? grid_for(n, 256, 65536) : 1u), dim3(256), 0,
                     stream, q_loc, q_scale, p_loc, p_scale, n, t_loc, t_scale, kl, zeros, ones,
                     zinfo, nz);
  return hipGetLastError();
}

hipError_t launch_imp_grouped_prep(const float* q_loc, const float* q_scale, const float* p_loc,
                                   const float* p_scale, int64_t n, float limit,
                                   const int64_t* item_off, const int32_t* seed1, int64_t n_items,
                                   int32_t seed1_one, float* t_loc, float* t_scale, uint8_t* keep,
                                   float* zeros, float* ones, float* kl2, float* tsamp,
                                   hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_imp_grouped_prep, dim3(grid_for(n, 256, 65536)), dim3(256), 0, stream,
                     q_loc, q_scale, p_loc, p_scale, n, limit, item_off, seed1, n_items, seed1_one,
                     t_loc, t_scale, keep, zeros, ones, kl2, tsamp);
  return hipGetLastError();
}

hipError_t launch_destandardise(const float* sample, const float* p_loc, const float* p_scale,
                                int64_t n, float* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_destandardise, dim3(grid_for(n, 256, 65536)), dim3(256), 0, stream,
                     sample, p_loc, p_scale, n, out);
  return hipGetLastError();
}

hipError_t launch_selftest_bm(uint32_t m0, int64_t count, float* rad, float* sn, float* cs,
                              hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_selftest_bm, dim3(grid_for(count, 256, 65536)), dim3(256), 0, stream, m0,
                     count, rad, sn, cs);
  return hipGetLastError();
}

hipError_t launch_selftest_screen(uint32_t m0, int64_t count, float* rad, float* sn, float* cs,
                                  hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_selftest_screen, dim3(grid_for(count, 256, 65536)), dim3(256), 0, stream,
                     m0, count, rad, sn, cs);
  return hipGetLastError();
}

int tile_times(unsigned long long* t0, unsigned long long* t1, unsigned int* wg, int n) {
#ifdef CWQ_TILE_TIMES
  if (n > kTileTimes) n = kTileTimes;
  if (hipMemcpyFromSymbol(t0, HIP_SYMBOL(g_tile_t0), (size_t)n * 8) != hipSuccess ||
      hipMemcpyFromSymbol(t1, HIP_SYMBOL(g_tile_t1), (size_t)n * 8) != hipSuccess ||
      hipMemcpyFromSymbol(wg, HIP_SYMBOL(g_tile_wg), (size_t)n * 4) != hipSuccess)
    return -1;
  return n;
#else
  (void)t0; (void)t1; (void)wg; (void)n;
  return 0;
#endif
}

int quad_times(unsigned long long* t, unsigned int* info, int n) {
#ifdef CWQ_QUAD_TIMES
  if (n > kQuadTimes) n = kQuadTimes;
  if (hipMemcpyFromSymbol(t, HIP_SYMBOL(g_quad_t), (size_t)n * 6 * 8) != hipSuccess ||
      hipMemcpyFromSymbol(info, HIP_SYMBOL(g_quad_info), (size_t)n * 4 * 4) != hipSuccess)
    return -1;
  return n;
#else
  (void)t; (void)info; (void)n;
  return 0;
#endif
}

int prune_stats(unsigned long long* out72, int reset) {
#ifdef CWQ_PRUNE_STATS
  if (hipMemcpyFromSymbol(out72, HIP_SYMBOL(g_prune_stats), sizeof(unsigned long long) * 72) !=
      hipSuccess)
    return -1;
  if (reset & 6) {
    const int v = (reset & 2) ? 1 : 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_seed_tau), &v, sizeof(int)) != hipSuccess) return -1;
  }
  if (reset & 1) {
    static const unsigned long long zero[72] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_prune_stats), zero, sizeof(zero)) != hipSuccess) return -1;
  }
  return 1;
#else
  for (int i = 0; i < 72; ++i) out72[i] = 0;
  (void)reset;
  return 0;
#endif
}

hipError_t launch_selftest_wave_max(const float* x, int64_t nw, float* out, hipStream_t stream) {
  if (nw <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_selftest_wave_max, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, stream, x,
                     nw, out);
  return hipGetLastError();
}

hipError_t launch_selftest_div(const float* a, const float* b, int64_t n, float* out,
                               hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_selftest_div, dim3(grid_for(n, 256, 65536)), dim3(256), 0, stream, a, b, n,
                     out);
  return hipGetLastError();
}

hipError_t launch_selftest_logf(const float* x, int64_t n, float* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_selftest_logf, dim3(grid_for(n, 256, 65536)), dim3(256), 0, stream, x, n,
                     out);
  return hipGetLastError();
}

}  // namespace cwq
