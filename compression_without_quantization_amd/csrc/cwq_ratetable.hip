// cwq_ratetable.hip -- rate tables for the single-step greedy coder (DESIGN.md
// 4j): for every block and every budget b = 0 .. B the index cwq_greedy_encode
// chooses at b bits and the log-density it wins, and budgets chosen from such a
// table.
//
// Candidate row n of a block is drawn from the flat indices n d + j of one
// stream, whatever the budget: the 2^b rows of a b-bit code are
// the first 2^b rows of a B-bit code.  The winner at b bits is the argmax over
// rows [0, 2^b) of one list, and the argmax key holds its value.
//
//   k_rate_levels   scores rows [0, 2^L), L = min(B, 11), of every block once
//                   and keeps the best key of every level of rows in
//                   lkeys[g][r]: level 0 is row 0, level r >= 1 rows
//                   [2^(r-1), 2^r).  A lane per row (eval_row_f), or a wave per
//                   row for blocks of at least CWQ_CSR_COOP_MIN_D dims.
//   k_rate_fold     the running maximum of lkeys[g][0 .. L] over r is budget
//                   r's key: lower levels hold lower indices and the key
//                   prefers the lower index on equal values, so a plain u64
//                   maximum is the encoder's argmax.
//   k_rate_columns  budgets 12 .. B come from one launch_encode each (the host
//                   loop in cwq_capi.hip); this reads their key columns.
//   k_choose_bits   per block the lowest b that maximises value[g][b] - lam b.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "cwq_device.h"
#include "cwq_kernels.h"

namespace cwq {

namespace {

constexpr int kRowChunk = 248;  // exact_row_wave's chunk: a multiple of 8, at most 63 Philox blocks

// Row `kbase / d` of a step-0 stream scored by a whole wave, k_encode_rows_wave's
// values bit for bit: the terms of up to 63 Philox blocks per chunk go through
// `buf`, lanes 0-7 fold them into the eight Eigen accumulators and lane 8 into
// the tail, in eval_row_f's order.  Full exec mask; every lane returns the value.
__device__ __forceinline__ float rate_row_wave(const PhiloxStream& st, uint64_t kbase, int64_t d,
                                               const float* __restrict__ loc_s,
                                               const float* __restrict__ scale_s,
                                               const float* __restrict__ mu,
                                               const float* __restrict__ sg,
                                               const float* __restrict__ lognorm,
                                               const double* logtab, float* buf, uint32_t lane) {
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
          const float sc = scale_s[j];
          buf[e] = log_prob(shard_sample(loc_s[j], sc, f4_word(z, (uint32_t)t)), mu[j], sg[j],
                            lognorm[j]);
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

// A running (level, best key) pair: rows arrive in increasing order, so the
// level only rises; the best key of a finished level goes to the workgroup's
// LDS maxima.
struct LevelFold {
  int cur = -1;
  uint64_t best = 0;
  __device__ __forceinline__ void flush(unsigned long long* lvl) {
    if (best) atomicMax(&lvl[cur], (unsigned long long)best);
  }
  __device__ __forceinline__ void add(float v, uint32_t n, unsigned long long* lvl) {
    const int r = rate_level(n);
    if (r != cur) {
      flush(lvl);
      cur = r;
      best = 0;
    }
    const uint64_t k = argmax_key(v, n);
    best = k > best ? k : best;
  }
};

// One tile = (block g, rows [n0, n1)), n0 a multiple of 256.  Wave v owns the
// rows n == n0 + v (mod 4), as in k_encode_eval: the Philox word alignment of a
// lane's rows is uniform within the wave.  LONG: blocks of at least
// CWQ_CSR_COOP_MIN_D dims give every row to a whole wave instead.  DC > 0:
// uniform blocks of that many dims (k_encode_eval's compile-time lengths).
template <bool LONG, int DC>
__global__ void __launch_bounds__(256) k_rate_levels(
    const float* __restrict__ t_loc, const float* __restrict__ t_scale,
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const float* __restrict__ lognorm, const int64_t* __restrict__ block_off, int64_t ud,
    int64_t ntiles, int64_t tiles_per_block, int64_t rows_per_tile, int64_t n_rows, SeedSpec sd,
    unsigned long long* __restrict__ lkeys) {
  __shared__ double logtab[32];
  __shared__ unsigned long long lvl[kRateLevels];
  __shared__ float rowbuf[LONG ? 4 : 1][kRowChunk];
  fill_logtab(logtab);
  const uint32_t wv = wave_id();
  const uint32_t lane = threadIdx.x & 63u;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (threadIdx.x < kRateLevels) lvl[threadIdx.x] = 0ull;
    __syncthreads();
    const int64_t g = tile / tiles_per_block;
    const int64_t tt = tile - g * tiles_per_block;
    const BlockSpan sp = block_span(block_off, ud, g);
    const int64_t n0 = tt * rows_per_tile;
    const int64_t n1 = (n0 + rows_per_tile < n_rows) ? n0 + rows_per_tile : n_rows;
    const PhiloxStream st = generate_key(step_seed(sd.of(g), 0), 42);
    const float* ls = loc_s + sp.off;
    const float* ss = scale_s + sp.off;
    const float* mu = t_loc + sp.off;
    const float* sg = t_scale + sp.off;
    const float* ln = lognorm + sp.off;
    LevelFold f;
    if (LONG && sp.d >= CWQ_CSR_COOP_MIN_D) {
      // uniform over the wave: rate_row_wave runs with all 64 lanes
      for (int64_t n = n0 + wv; n < n1; n += 4) {
        const float v = rate_row_wave(st, (uint64_t)n * (uint64_t)sp.d, sp.d, ls, ss, mu, sg, ln,
                                      logtab, rowbuf[LONG ? wv : 0], lane);
        if (lane == 0) f.add(v, (uint32_t)n, lvl);
      }
      if (lane == 0) f.flush(lvl);
    } else {
      const int align = (int)(((uint64_t)(n0 + wv) * (uint64_t)sp.d) & 3u);
      for (int64_t n = n0 + 4 * (int64_t)lane + wv; n < n1; n += 256) {
        const float v = eval_row_f<DC>(
            st, (uint64_t)n * (uint64_t)sp.d, sp.d, align, logtab, [&](int64_t e, float zz) {
              const float sc = ss[e];
              return log_prob(shard_sample(ls[e], sc, zz), mu[e], sg[e], ln[e]);
            });
        f.add(v, (uint32_t)n, lvl);
      }
      // past a block's first 256 rows a wave's rows share one level: one LDS
      // atomic per wave then, else one per lane
      const int c = __builtin_amdgcn_readfirstlane(f.cur);
      if (__all(f.best == 0 || f.cur == c)) {
        const uint64_t m = wave_max_u64(f.best);
        if (lane == 0 && m) atomicMax(&lvl[c], (unsigned long long)m);
      } else {
        f.flush(lvl);
      }
    }
    __syncthreads();
    if (threadIdx.x < kRateLevels && lvl[threadIdx.x])
      atomicMax(&lkeys[g * kRateLevels + threadIdx.x], lvl[threadIdx.x]);
    __syncthreads();
  }
}

// What a reduced key says: the index by key_index, the value by the inverse of
// the key's ord.  A key at or below the clamp level (0: no row beat the
// reducer's initial accumulator) is index 0 at -FLT_MAX; an empty block's rows
// all score +0, which is what it gets whether or not a kernel scored them.
__device__ __forceinline__ void write_entry(uint64_t key, bool empty, int32_t* idx, float* value) {
  const uint32_t o = (uint32_t)(key >> 32);
  *idx = (int32_t)key_index(key);
  *value = empty ? 0.0f : (o > kArgmaxClampOrd ? unord_f32(o) : -0x1.fffffep+127f);
}

__global__ void __launch_bounds__(256) k_rate_fold(
    const unsigned long long* __restrict__ lkeys, const int64_t* __restrict__ block_off,
    int64_t ud, int64_t nb, int levels, int n_cols, int32_t* __restrict__ out_idx,
    float* __restrict__ out_value) {
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < nb;
       g += (int64_t)gridDim.x * blockDim.x) {
    const bool empty = block_span(block_off, ud, g).d <= 0;
    uint64_t m = 0;
    for (int r = 0; r <= levels; ++r) {
      const uint64_t k = lkeys[g * kRateLevels + r];
      m = k > m ? k : m;
      write_entry(m, empty, out_idx + g * n_cols + r, out_value + g * n_cols + r);
    }
  }
}

// hkeys [n_high][nb]: column c is budget first + c's argmax keys
__global__ void __launch_bounds__(256) k_rate_columns(
    const unsigned long long* __restrict__ hkeys, const int64_t* __restrict__ block_off,
    int64_t ud, int64_t nb, int first, int n_high, int n_cols, int32_t* __restrict__ out_idx,
    float* __restrict__ out_value) {
  const int64_t total = nb * n_high;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = t / nb, g = t - c * nb;
    const bool empty = block_span(block_off, ud, g).d <= 0;
    write_entry(hkeys[t], empty, out_idx + g * n_cols + first + c,
                out_value + g * n_cols + first + c);
  }
}

__global__ void k_total_reset(long long* __restrict__ total) { *total = 0; }

// A lane per block.  float64 with a separate multiply and subtract (the build
// has -ffp-contract=off), so numpy reproduces every comparison.
__global__ void __launch_bounds__(256) k_choose_bits(const float* __restrict__ value, int64_t nb,
                                                     int n_cols, double lam, int lo, int hi,
                                                     int32_t* __restrict__ out_bits,
                                                     long long* __restrict__ total) {
  long long sum = 0;
  for (int64_t g0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) & ~(int64_t)63; g0 < nb;
       g0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = g0 + (threadIdx.x & 63);
    if (g < nb) {
      int best_b = lo;
      double best = (double)value[g * n_cols + lo] - lam * (double)lo;
      for (int b = lo + 1; b <= hi; ++b) {
        const double s = (double)value[g * n_cols + b] - lam * (double)b;
        if (s > best) best = s, best_b = b;
      }
      out_bits[g] = best_b;
      sum += best_b;
    }
  }
  if (total == nullptr) return;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd((unsigned long long*)total, (unsigned long long)sum);
}

// ---- budgets under a total (cwq_rate_solve.h) ---------------------
// The sweeps read the table a tile of 64 rows per wave at a time: the tile is
// 64 n_cols contiguous floats, loaded coalesced into LDS at a row stride of
// n_cols | 1 words, from which lane l reads row l.  ds_read_b32 banks are the
// word address mod 32 within each half of the wave, and an odd stride sends 32
// consecutive rows to 32 different banks.  Per-lane totals are 32-bit: a
// workgroup's share of the rows of a table that fits the device's memory sums
// far below 2^32 (4 (B + 1) nb bytes of table bound nb B).
constexpr int kSolveWaves = 4;               // per workgroup
// The grid: 256 CUs x the workgroups of k_solve_sweep a CU holds at once, so
// that no workgroup waits for another to end; the tiles beyond are strided
// over.  A CU holds what its registers and its LDS both allow: by registers a
// wave of each workgroup per SIMD (r = 3, 4, 5, 6: 67, 77, 109, 167 VGPRs as
// hipcc of ROCm 7 allots them, i.e. 7, 6, 4, 3 waves of the 512 a SIMD lane
// has), by LDS 160 KiB over the workgroup's tiles (solve_grid below).
constexpr unsigned kSolveWgPerCuRegs = kSolveLevels == 6 ? 3 : kSolveLevels == 5 ? 4
                                       : kSolveLevels == 4 ? 6 : 7;
constexpr size_t kSolveLdsPerCu = 160 * 1024;
constexpr size_t kSolveStaticLds = 8 * kSolveSlots;  // k_solve_sweep's wg_tot

__global__ void k_solve_reset(SolveState* __restrict__ st) {
  st->span_key = 0;
  st->total0 = 0;
  st->done = 0;
}

// This wave's next tile into `mine`; returns the row of this lane, or nullptr
// past the table's end.  Full exec mask.
__device__ __forceinline__ const float* solve_stage(const float* __restrict__ value, int64_t tile,
                                                    int64_t nb, int n_cols, int stride, float* mine,
                                                    uint32_t lane) {
  const int64_t row0 = tile * 64;
  const int rows = nb - row0 < 64 ? (int)(nb - row0) : 64;
  const int cnt = rows * n_cols;
  const float* src = value + row0 * n_cols;
  // the reads of the tile before are done before this one's stores
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int i = (int)lane; i < cnt; i += 64) {
    const int r = i / n_cols;
    mine[r * stride + (i - r * n_cols)] = src[i];
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return (int)lane < rows ? mine + lane * stride : nullptr;
}

// One price.  FIRST: lam = 0; total(0) and the span's key go to the state, no
// bits are written.  Else lam = *lam_p (the last step's), and the bits and
// their sum are the call's results.  k_choose_bits' arithmetic, term for term.
template <bool FIRST>
__global__ void __launch_bounds__(64 * kSolveWaves) k_solve_single(
    const float* __restrict__ value, int64_t nb, int n_cols, int lo, int hi, int stride,
    int64_t tiles, const double* __restrict__ lam_p, SolveState* __restrict__ st,
    int32_t* __restrict__ out_bits, long long* __restrict__ out_total) {
  extern __shared__ float solve_rows[];
  const uint32_t lane = threadIdx.x & 63u, wv = wave_id();
  float* mine = solve_rows + (size_t)wv * 64 * stride;
  const double lam = FIRST ? 0.0 : *lam_p;
  long long sum = 0;
  uint64_t span = 0;
  for (int64_t t = (int64_t)blockIdx.x * kSolveWaves + wv; t < tiles;
       t += (int64_t)gridDim.x * kSolveWaves) {
    const float* row = solve_stage(value, t, nb, n_cols, stride, mine, lane);
    if (row) {
      const double v_lo = (double)row[lo];
      int best_b = lo;
      double best = v_lo - solve_product(lam, lo);
      for (int b = lo + 1; b <= hi; ++b) {
        const double v = (double)row[b];
        const double s = v - solve_product(lam, b);
        if (s > best) best = s, best_b = b;
        if (FIRST) {
          const uint64_t k = solve_span_key(v - v_lo);
          span = k > span ? k : span;
        }
      }
      if (!FIRST) out_bits[t * 64 + lane] = best_b;
      sum += best_b;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
  long long* total = FIRST ? (long long*)&st->total0 : out_total;
  if (lane == 0 && sum) atomicAdd((unsigned long long*)total, (unsigned long long)sum);
  if (FIRST) {
    span = wave_max_u64(span);
    if (lane == 0 && span) atomicMax((unsigned long long*)&st->span_key, (unsigned long long)span);
  }
}

// One wave between two sweeps.  Round 0 starts the interval from the first
// sweep's facts; round i > 0 walks the tree of round i - 1 by its totals.  Before
// the last round's end it lays out the next tree (lane k: node k's products)
// and zeroes its totals; at the end it writes lam_hi and zeroes the sum the
// last pass adds to.
__global__ void __launch_bounds__(64) k_solve_step(SolveState* __restrict__ st,
                                                   double* __restrict__ prod,
                                                   long long* __restrict__ totals, int64_t target,
                                                   int n_budgets, int round,
                                                   double* __restrict__ out_lam,
                                                   long long* __restrict__ out_total) {
  const int k = (int)threadIdx.x;
  SolveInterval iv;
  int done;
  if (round == 0) {
    iv = solve_start(st->total0, target, solve_span_of(st->span_key));
    done = st->total0 <= target;
  } else {
    iv = SolveInterval{st->lo, st->hi};
    done = st->done;
    if (!done) iv = solve_walk(iv, (const int64_t*)totals, target);
  }
  // Every lane has read the state and walked the totals before any lane zeroes
  // them: this barrier is the only thing that orders the two, so the kernel
  // must stay at one workgroup (it is launched as one wave).  All lanes walk,
  // redundantly: each needs the interval for its node.
  __syncthreads();
  if (round < kSolveRounds) {
    if (k < kSolveSlots) {
      solve_fill_node(iv, k, n_budgets, prod);
      totals[k] = 0;
    }
    if (k == 0) st->lo = iv.lo, st->hi = iv.hi, st->done = done;
  } else if (k == 0) {
    *out_lam = iv.hi;
    *out_total = 0;
  }
}

// total(mid_k) of every node of the tree in `prod`, eight nodes at a time: a
// lane holds its row's value at b once per eight nodes, subtracts the nodes'
// products (wave-uniform) and keeps eight running maxima, k_choose_bits' rule
// with the multiply taken out.  Slot 0 is no node; it is evaluated (at lam 0)
// for the loop's regularity and nobody reads its total.
__global__ void __launch_bounds__(64 * kSolveWaves) k_solve_sweep(
    const float* __restrict__ value, int64_t nb, int n_cols, int lo, int hi, int stride,
    int64_t tiles, const SolveState* __restrict__ st, const double* __restrict__ prod,
    long long* __restrict__ totals) {
  extern __shared__ float solve_rows[];
  __shared__ unsigned long long wg_tot[kSolveSlots];
  if (st->done) return;  // uniform over the grid
  const uint32_t lane = threadIdx.x & 63u, wv = wave_id();
  float* mine = solve_rows + (size_t)wv * 64 * stride;
  if (threadIdx.x < kSolveSlots) wg_tot[threadIdx.x] = 0ull;
  uint32_t tot[kSolveSlots];
#pragma unroll
  for (int k = 0; k < kSolveSlots; ++k) tot[k] = 0;
  for (int64_t t = (int64_t)blockIdx.x * kSolveWaves + wv; t < tiles;
       t += (int64_t)gridDim.x * kSolveWaves) {
    const float* row = solve_stage(value, t, nb, n_cols, stride, mine, lane);
    const double v_lo = row ? (double)row[lo] : 0.0;
#pragma unroll
    for (int c = 0; row && c < kSolveSlots; c += 8) {
      double best[8];
      int best_b[8];
      const double* p = prod + solve_prod_at(lo, c);
#pragma unroll
      for (int j = 0; j < 8; ++j) best[j] = v_lo - p[j], best_b[j] = lo;
      for (int b = lo + 1; b <= hi; ++b) {
        const double v = (double)row[b];
        p = prod + solve_prod_at(b, c);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const double s = v - p[j];
          if (s > best[j]) best[j] = s, best_b[j] = b;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) tot[c + j] += (uint32_t)best_b[j];
    }
  }
  __syncthreads();  // wg_tot is zero
#pragma unroll
  for (int k = 0; k < kSolveSlots; ++k) {
    uint32_t s = tot[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0 && s) atomicAdd(&wg_tot[k], (unsigned long long)s);
  }
  __syncthreads();
  if (threadIdx.x < kSolveSlots && wg_tot[threadIdx.x])
    atomicAdd((unsigned long long*)&totals[threadIdx.x], wg_tot[threadIdx.x]);
}

// out_idx[g] = the table's index at the budget chosen for block g
__global__ void __launch_bounds__(256) k_rate_gather(const int32_t* __restrict__ tidx,
                                                     const int32_t* __restrict__ bits, int64_t nb,
                                                     int n_cols, int32_t* __restrict__ out_idx) {
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < nb;
       g += (int64_t)gridDim.x * blockDim.x)
    out_idx[g] = tidx[g * n_cols + bits[g]];
}

}  // namespace

hipError_t launch_choose_bits_total(const float* value, int64_t nb, int n_cols, int64_t target,
                                    int lo, int hi, int32_t* out_bits, double* out_lam,
                                    int64_t* out_total, SolveState* state, double* prod,
                                    int64_t* totals, hipStream_t stream) {
  const int stride = n_cols | 1;
  const size_t lds = (size_t)kSolveWaves * 64 * stride * sizeof(float);
  const int64_t tiles = (nb + 63) / 64;
  const unsigned by_lds = (unsigned)(kSolveLdsPerCu / (lds + kSolveStaticLds));  // >= 5: lds <= 31 KiB
  const unsigned per_cu = by_lds < kSolveWgPerCuRegs ? by_lds : kSolveWgPerCuRegs;
  const dim3 grid(grid_for(tiles, kSolveWaves, 256 * per_cu)), wg(64 * kSolveWaves);
  long long* tot = (long long*)totals;
  hipLaunchKernelGGL(k_solve_reset, dim3(1), dim3(1), 0, stream, state);
  hipLaunchKernelGGL(k_solve_single<true>, grid, wg, lds, stream, value, nb, n_cols, lo, hi, stride,
                     tiles, (const double*)nullptr, state, (int32_t*)nullptr, (long long*)nullptr);
  for (int round = 0; round <= kSolveRounds; ++round) {
    hipLaunchKernelGGL(k_solve_step, dim3(1), dim3(64), 0, stream, state, prod, tot, target, n_cols,
                       round, out_lam, (long long*)out_total);
    if (round < kSolveRounds)
      hipLaunchKernelGGL(k_solve_sweep, grid, wg, lds, stream, value, nb, n_cols, lo, hi, stride,
                         tiles, (const SolveState*)state, (const double*)prod, tot);
  }
  hipLaunchKernelGGL(k_solve_single<false>, grid, wg, lds, stream, value, nb, n_cols, lo, hi, stride,
                     tiles, (const double*)out_lam, state, out_bits, (long long*)out_total);
  return hipGetLastError();
}

hipError_t launch_rate_gather(const int32_t* tidx, const int32_t* bits, int64_t nb, int n_cols,
                              int32_t* out_idx, hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rate_gather, dim3(grid_for(nb, 256, 4096)), dim3(256), 0, stream, tidx, bits,
                     nb, n_cols, out_idx);
  return hipGetLastError();
}

hipError_t launch_rate_levels(const RatePlan& p, const float* t_loc, const float* t_scale,
                              const float* loc_s, const float* scale_s, const float* lognorm,
                              const int64_t* block_off, int64_t ud, int32_t seed,
                              int64_t block_id_base, unsigned long long* lkeys,
                              hipStream_t stream) {
  if (p.workgroups == 0) return hipSuccess;
  const SeedSpec sd{seed, block_id_base, nullptr};
  const int64_t n_rows = (int64_t)1 << p.levels;
#define CWQ_RATE_LEVELS(LONG, DC)                                                               \
  hipLaunchKernelGGL((k_rate_levels<LONG, DC>), dim3(p.workgroups), dim3(256), 0, stream, t_loc, \
                     t_scale, loc_s, scale_s, lognorm, block_off, ud, p.tiles,                   \
                     p.tiles_per_block, p.rows_per_tile, n_rows, sd, lkeys)
  if (p.long_rows)
    CWQ_RATE_LEVELS(true, 0);
  else if (block_off == nullptr && ud == 8)
    CWQ_RATE_LEVELS(false, 8);
  else if (block_off == nullptr && ud == 16)
    CWQ_RATE_LEVELS(false, 16);
  else if (block_off == nullptr && ud == 32)
    CWQ_RATE_LEVELS(false, 32);
  else
    CWQ_RATE_LEVELS(false, 0);
#undef CWQ_RATE_LEVELS
  return hipGetLastError();
}

hipError_t launch_rate_fold(const RatePlan& p, const unsigned long long* lkeys,
                            const unsigned long long* hkeys, const int64_t* block_off, int64_t ud,
                            int64_t nb, int max_bits, int32_t* out_idx, float* out_value,
                            hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rate_fold, dim3(grid_for(nb, 256, 4096)), dim3(256), 0, stream, lkeys,
                     block_off, ud, nb, p.levels, max_bits + 1, out_idx, out_value);
  if (p.high_count > 0)
    hipLaunchKernelGGL(k_rate_columns, dim3(grid_for(nb * p.high_count, 256, 4096)), dim3(256), 0,
                       stream, hkeys, block_off, ud, nb, p.high_first, p.high_count, max_bits + 1,
                       out_idx, out_value);
  return hipGetLastError();
}

hipError_t launch_choose_bits(const float* value, int64_t nb, int n_cols, double lam, int lo,
                              int hi, int32_t* out_bits, int64_t* out_total, hipStream_t stream) {
  if (out_total) hipLaunchKernelGGL(k_total_reset, dim3(1), dim3(1), 0, stream, (long long*)out_total);
  if (nb > 0)
    hipLaunchKernelGGL(k_choose_bits, dim3(grid_for(nb, 256, 4096)), dim3(256), 0, stream, value,
                       nb, n_cols, lam, lo, hi, out_bits, (long long*)out_total);
  return hipGetLastError();
}

}  // namespace cwq
