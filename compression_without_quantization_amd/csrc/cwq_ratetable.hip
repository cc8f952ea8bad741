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

}  // namespace

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
