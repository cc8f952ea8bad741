// cwq_varbits.hip -- uniform blocks with a bit budget of their own.
//
// The tuned encoders take one n_bits_per_step per launch.  This file adds the
// layer around them: the budget of each block
// from its KL (k_block_bits), a stable counting sort of the blocks by budget
// (k_vb_hist / k_vb_scan / k_vb_rank), the gather into sorted order and the
// scatter back, and the packed bitstream of the indices (k_vb_off_* for the
// bit offsets, k_vb_pack, k_vb_unpack).  Nothing here scores a candidate: the
// blocks of one budget are coded by the existing launch_encode.
//
// Ragged (CSR) blocks reuse the sort and the stream and add
// their own budgets (k_block_bits_csr), the sorted ragged layout with the facts
// the host needs to launch each bucket (k_vbc_tile / k_vbc_reduce /
// k_vbc_soff_final) and a segmented gather and scatter (k_vbc_gather,
// k_vbc_scatter).
//
// Backfitting under budgets adds the gather of an index table
// into sorted order with its range check (k_vb_gather_table) and the scatter
// of the per-block results (k_vb_scatter_blocks).
//
// Every result is reproducible: the only atomics are integer adds (a histogram
// in LDS, the range check's count of failures), all other global writes are
// plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cwq_device.h"
#include "cwq_kernels.h"

namespace cwq {
namespace {

// kVbThreads, kVbPerThread, kVbTile, kVbBins: cwq_workspace.h (they size the scratch)
constexpr int kVbMaxBits = 30;                      // CWQ_MAX_BITS_PER_STEP

__device__ __forceinline__ int vb_bin(int32_t b) {
  return (b < 0 || b > kVbMaxBits) ? kVbBins - 1 : b;
}
// field width in the stream; an out-of-range count takes no room (and raises
// the offsets pass's flag)
__device__ __forceinline__ int vb_width(int32_t b) { return (b < 0 || b > kVbMaxBits) ? 0 : b; }

// ---------------------------------------------------------------------------
// The bit budget of each block: ceil(KL_g / ln 2 + extra_bits), clamped.  One
// lane per block; the block's per-dim float32 KLs (kl_normal_normal_1) are
// summed in float64 in dim order.
// ---------------------------------------------------------------------------
template <bool VEC4>
__global__ void __launch_bounds__(kVbThreads) k_block_bits(
    const float* __restrict__ q_loc, const float* __restrict__ q_scale,
    const float* __restrict__ p_loc, const float* __restrict__ p_scale, int64_t nb, int64_t d,
    double extra_bits, int32_t min_bits, int32_t max_bits, int32_t* __restrict__ bits_out,
    float* __restrict__ kl_bits_out) {
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < nb;
       g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = g * d;
    double S = 0.0;
    if (VEC4) {
      const float4* ql = (const float4*)(q_loc + o);
      const float4* qs = (const float4*)(q_scale + o);
      const float4* pl = (const float4*)(p_loc + o);
      const float4* ps = (const float4*)(p_scale + o);
      for (int64_t j = 0; j < d / 4; ++j) {
        const float4 a = ql[j], b = qs[j], c = pl[j], e = ps[j];
        S = S + (double)kl_normal_normal_1(a.x, b.x, c.x, e.x);
        S = S + (double)kl_normal_normal_1(a.y, b.y, c.y, e.y);
        S = S + (double)kl_normal_normal_1(a.z, b.z, c.z, e.z);
        S = S + (double)kl_normal_normal_1(a.w, b.w, c.w, e.w);
      }
    } else {
      for (int64_t j = 0; j < d; ++j)
        S = S + (double)kl_normal_normal_1(q_loc[o + j], q_scale[o + j], p_loc[o + j],
                                           p_scale[o + j]);
    }
    const double kl_bits = S / 0.6931471805599453;  // log(2.0)
    int32_t b = max_bits;                           // a non-finite sum: the most we may spend
    if (S - S == 0.0) {
      const double v = ceil(kl_bits + extra_bits);
      b = v < (double)min_bits ? min_bits : (v > (double)max_bits ? max_bits : (int32_t)v);
    }
    bits_out[g] = b;
    if (kl_bits_out) kl_bits_out[g] = (float)kl_bits;
  }
}

// ---------------------------------------------------------------------------
// Stable counting sort of the blocks by bit count: perm[rank] = g.
// Workgroup w owns blocks [w kVbTile, (w + 1) kVbTile) in all three stages.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kVbThreads) k_vb_hist(const int32_t* __restrict__ bits,
                                                        int64_t nb,
                                                        uint32_t* __restrict__ wg_hist) {
  __shared__ uint32_t h[kVbBins];
  if (threadIdx.x < kVbBins) h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t g0 = (int64_t)blockIdx.x * kVbTile;
  for (int i = threadIdx.x; i < kVbTile; i += kVbThreads) {
    const int64_t g = g0 + i;
    if (g < nb) atomicAdd(&h[vb_bin(bits[g])], 1u);
  }
  __syncthreads();
  if (threadIdx.x < kVbBins) wg_hist[(int64_t)blockIdx.x * kVbBins + threadIdx.x] = h[threadIdx.x];
}

// One workgroup: wg_hist[w][b] becomes the rank of workgroup w's first block
// of bin b (bins in ascending order, workgroups in order inside a bin), and
// counts[b] the bin's size.  Lane b of segment s walks an eighth of the rows.
__global__ void __launch_bounds__(kVbThreads) k_vb_scan(uint32_t* __restrict__ wg_hist,
                                                        int64_t nwg,
                                                        uint32_t* __restrict__ counts) {
  constexpr int kSeg = kVbThreads / kVbBins;
  __shared__ uint32_t seg[kSeg][kVbBins];
  __shared__ uint32_t start[kVbBins];
  const int b = threadIdx.x & (kVbBins - 1), s = threadIdx.x / kVbBins;
  const int64_t per = (nwg + kSeg - 1) / kSeg;
  const int64_t w0 = s * per < nwg ? s * per : nwg;
  const int64_t w1 = w0 + per < nwg ? w0 + per : nwg;
  uint32_t sum = 0;
  for (int64_t w = w0; w < w1; ++w) sum += wg_hist[w * kVbBins + b];
  seg[s][b] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int bb = 0; bb < kVbBins; ++bb) {
      uint32_t t = 0;
      for (int ss = 0; ss < kSeg; ++ss) t += seg[ss][bb];
      counts[bb] = t;
      start[bb] = run;
      run += t;
    }
  }
  __syncthreads();
  uint32_t run = start[b];
  for (int ss = 0; ss < s; ++ss) run += seg[ss][b];
  for (int64_t w = w0; w < w1; ++w) {
    const uint32_t t = wg_hist[w * kVbBins + b];
    wg_hist[w * kVbBins + b] = run;
    run += t;
  }
}

// Ranks inside a workgroup, 256 blocks at a time in block order: a lane's rank
// among its wave's lanes of the same bin comes from five ballots, the waves'
// counts per bin go through LDS.
__global__ void __launch_bounds__(kVbThreads) k_vb_rank(const int32_t* __restrict__ bits,
                                                        int64_t nb,
                                                        const uint32_t* __restrict__ wg_base,
                                                        int32_t* __restrict__ perm) {
  constexpr int kWaves = kVbThreads / 64;
  __shared__ uint32_t base[kVbBins];
  __shared__ uint32_t wcnt[kWaves][kVbBins];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < kVbBins) {
    base[tid] = wg_base[(int64_t)blockIdx.x * kVbBins + tid];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) wcnt[w][tid] = 0;
  }
  __syncthreads();
  const int64_t g0 = (int64_t)blockIdx.x * kVbTile;
  for (int c = 0; c < kVbTile; c += kVbThreads) {
    if (g0 + c >= nb) break;  // uniform
    const int64_t g = g0 + c + tid;
    const bool valid = g < nb;
    const int bin = valid ? vb_bin(bits[g]) : 0;
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 5; ++bit) {
      const bool set = (bin >> bit) & 1;
      const uint64_t bal = __ballot(set);
      m &= set ? bal : ~bal;
    }
    const uint32_t r = (uint32_t)__popcll(m & (((uint64_t)1 << lane) - 1));
    if (valid && r == 0) wcnt[wave][bin] = (uint32_t)__popcll(m);
    __syncthreads();
    if (valid) {
      uint32_t o = base[bin] + r;
      for (int w = 0; w < wave; ++w) o += wcnt[w][bin];
      perm[o] = (int32_t)g;
    }
    __syncthreads();
    if (tid < kVbBins) {
      uint32_t t = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        t += wcnt[w][tid];
        wcnt[w][tid] = 0;
      }
      base[tid] += t;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Gather into sorted order (row r of the outputs = row perm[r] of the inputs)
// with each row's seed, and the scatter of the results back.  V: float4 rows
// (d % 4 == 0, 16-byte aligned bases) or float.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void vb_row_of(int64_t i, int64_t dv, int64_t& r, int64_t& q) {
  if ((uint64_t)(i | dv) >> 32) {
    r = i / dv;
  } else {
    r = (int64_t)((uint32_t)i / (uint32_t)dv);
  }
  q = i - r * dv;
}

template <typename V>
__global__ void __launch_bounds__(kVbThreads) k_vb_gather(
    const V* __restrict__ a0, const V* __restrict__ a1, const V* __restrict__ a2,
    const V* __restrict__ a3, const int32_t* __restrict__ perm, int64_t nb, int64_t dv,
    int32_t seed, int64_t block_id_base, V* __restrict__ o0, V* __restrict__ o1,
    V* __restrict__ o2, V* __restrict__ o3, int32_t* __restrict__ seeds) {
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t total = nb * dv;
  for (int64_t i = t0; i < total; i += stride) {
    int64_t r, q;
    vb_row_of(i, dv, r, q);
    const int64_t src = (int64_t)perm[r] * dv + q;
    o0[i] = a0[src];
    o1[i] = a1[src];
    o2[i] = a2[src];
    o3[i] = a3[src];
  }
  for (int64_t r = t0; r < nb; r += stride) seeds[r] = block_seed(seed, block_id_base + perm[r]);
}

template <typename V>
__global__ void __launch_bounds__(kVbThreads) k_vb_scatter(
    const V* __restrict__ sample_s, const int32_t* __restrict__ idx_s,
    const int32_t* __restrict__ perm, int64_t nb, int64_t dv, int64_t n_steps,
    V* __restrict__ out_sample, int32_t* __restrict__ out_idx) {
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t total = nb * dv;
  for (int64_t i = t0; i < total; i += stride) {
    int64_t r, q;
    vb_row_of(i, dv, r, q);
    out_sample[(int64_t)perm[r] * dv + q] = sample_s[i];
  }
  const int64_t ni = nb * n_steps;
  for (int64_t i = t0; i < ni; i += stride) {
    int64_t r, s;
    vb_row_of(i, n_steps, r, s);
    out_idx[(int64_t)perm[r] * n_steps + s] = idx_s[i];
  }
}

// ---------------------------------------------------------------------------
// Bit offsets: off[g] = sum over g' < g of n_steps * width(g'), off[nb] the
// total.  Two levels: a sum per workgroup tile, one workgroup scanning those,
// then each tile's own scan on top of its base.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int64_t wg_incl_scan(int64_t v, int64_t* lds) {  // lds [kVbThreads]
  const int tid = threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  for (int o = 1; o < kVbThreads; o <<= 1) {
    const int64_t t = tid >= o ? lds[tid - o] : 0;
    __syncthreads();
    lds[tid] += t;
    __syncthreads();
  }
  const int64_t r = lds[tid];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(kVbThreads) k_vb_off_partial(const int32_t* __restrict__ bits,
                                                               int64_t nb, int64_t n_steps,
                                                               int64_t* __restrict__ partial,
                                                               uint32_t* __restrict__ flag) {
  __shared__ int64_t lds[kVbThreads];
  __shared__ uint32_t bad_any;
  if (threadIdx.x == 0) bad_any = 0;
  __syncthreads();
  const int64_t g0 = (int64_t)blockIdx.x * kVbTile;
  int64_t sum = 0;
  bool bad = false;
  for (int i = threadIdx.x; i < kVbTile; i += kVbThreads) {
    const int64_t g = g0 + i;
    if (g < nb) {
      const int32_t b = bits[g];
      bad |= b < 0 || b > kVbMaxBits;
      sum += n_steps * vb_width(b);
    }
  }
  if (bad) bad_any = 1;  // every writer stores the same value
  const int64_t incl = wg_incl_scan(sum, lds);
  if (threadIdx.x == kVbThreads - 1) {
    partial[blockIdx.x] = incl;
    if (bad_any) *flag = 1;
  }
}

// One workgroup: partial[] to its exclusive scan; the total to off_end
// (off[nb]) and, where asked for, to total_out (-1 when the flag is raised).
__global__ void __launch_bounds__(kVbThreads) k_vb_off_scan(int64_t* __restrict__ partial,
                                                            int64_t nwg,
                                                            const uint32_t* __restrict__ flag,
                                                            int64_t* __restrict__ off_end,
                                                            int64_t* __restrict__ total_out) {
  __shared__ int64_t lds[kVbThreads];
  int64_t carry = 0;
  for (int64_t c = 0; c < nwg; c += kVbThreads) {
    const int64_t w = c + threadIdx.x;
    const int64_t v = w < nwg ? partial[w] : 0;
    const int64_t incl = wg_incl_scan(v, lds);
    if (w < nwg) partial[w] = carry + incl - v;
    lds[threadIdx.x] = incl;
    __syncthreads();
    carry += lds[kVbThreads - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *off_end = carry;
    if (total_out) *total_out = *flag ? -1 : carry;
  }
}

__global__ void __launch_bounds__(kVbThreads) k_vb_off_final(const int32_t* __restrict__ bits,
                                                             int64_t nb, int64_t n_steps,
                                                             const int64_t* __restrict__ partial,
                                                             int64_t* __restrict__ off) {
  __shared__ int64_t lds[kVbThreads];
  const int64_t g0 = (int64_t)blockIdx.x * kVbTile + (int64_t)threadIdx.x * kVbPerThread;
  int64_t w[kVbPerThread];
  int64_t sum = 0;
#pragma unroll
  for (int k = 0; k < kVbPerThread; ++k) {
    w[k] = g0 + k < nb ? n_steps * vb_width(bits[g0 + k]) : 0;
    sum += w[k];
  }
  int64_t run = partial[blockIdx.x] + wg_incl_scan(sum, lds) - sum;
#pragma unroll
  for (int k = 0; k < kVbPerThread; ++k) {
    if (g0 + k < nb) off[g0 + k] = run;
    run += w[k];
  }
}

// The last k in [0, n) with off[k] <= x (off non-decreasing, off[0] <= x).
__device__ __forceinline__ int64_t vb_last_le(const int64_t* __restrict__ off, int64_t n,
                                              int64_t x) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= x) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// ---------------------------------------------------------------------------
// Pack: one thread per 32-bit word of the output.  Stream bit i lies in byte
// i / 8 at bit 7 - i % 8 (binary_io._pack_bits), field (g, s) covers stream
// bits [off[g] + s w, off[g] + (s + 1) w) with its value's bit 0 first
// (to_bit_string).  The thread finds the first block reaching into its word by
// binary search, ORs every overlapping field into a big-endian word V (stream
// bit 32 j + t at bit 31 - t: the bit-reversed value shifted into place) and
// stores it once, byte-swapped.  Runs of zero-width blocks are skipped by
// another search, so a word costs at most 32 fields and their searches.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kVbThreads) k_vb_pack(
    const int32_t* __restrict__ idx, const int32_t* __restrict__ bits,
    const int64_t* __restrict__ off, int64_t nb, int64_t n_steps, uint8_t* __restrict__ out,
    int64_t out_cap, int64_t n_words, int word_stores) {
  const int64_t total = off[nb];
  const int64_t need = (total + 7) >> 3;
  const int64_t limit = need < out_cap ? need : out_cap;  // bytes this call may write
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n_words;
       j += (int64_t)gridDim.x * blockDim.x) {
    if (4 * j >= limit) return;
    const int64_t W0 = 32 * j, W1 = W0 + 32;  // W0 < total
    uint32_t V = 0;
    int64_t g = vb_last_le(off, nb + 1, W0);  // < nb, and off[g + 1] > W0
    while (g < nb) {
      const int64_t o = off[g];
      if (o >= W1) break;
      int w = vb_width(bits[g]);
      if (w == 0) {  // to the last block starting here: the one that has a width
        g = vb_last_le(off, nb + 1, o);
        if (g >= nb) break;
        w = vb_width(bits[g]);
      }
      int64_t s = o < W0 ? (W0 - o) / w : 0;
      for (; s < n_steps; ++s) {
        const int64_t fo = o + s * w;
        if (fo >= W1) break;
        const uint32_t v = (uint32_t)idx[g * n_steps + s] & (((uint32_t)1 << w) - 1u);
        const uint32_t r = __brev(v);
        const int sh = (int)(fo - W0);  // in (-30, 32)
        V |= sh >= 0 ? (r >> sh) : (r << -sh);
      }
      ++g;
    }
    if (word_stores && 4 * j + 4 <= limit) {
      ((uint32_t*)out)[j] = __builtin_bswap32(V);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * j + k < limit) out[4 * j + k] = (uint8_t)(V >> (24 - 8 * k));
    }
  }
}

// Unpack: one thread per field; the (at most five) bytes it spans are read one
// by one, those past n_bytes as 0.
__global__ void __launch_bounds__(kVbThreads) k_vb_unpack(
    const uint8_t* __restrict__ bytes, int64_t n_bytes, const int32_t* __restrict__ bits,
    const int64_t* __restrict__ off, int64_t nb, int64_t n_steps, int32_t* __restrict__ idx) {
  const int64_t nf = nb * n_steps;
  for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nf;
       f += (int64_t)gridDim.x * blockDim.x) {
    int64_t g, s;
    vb_row_of(f, n_steps, g, s);
    const int w = vb_width(bits[g]);
    uint32_t v = 0;
    if (w > 0) {
      const int64_t fo = off[g] + s * w;
      const int64_t by0 = fo >> 3;
      uint64_t B = 0;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const uint64_t byte = by0 + k < n_bytes ? bytes[by0 + k] : 0;
        B |= byte << (56 - 8 * k);
      }
      const uint32_t x = (uint32_t)((B << (fo & 7)) >> 32);  // first stream bit at bit 31
      v = __brev(x) & (((uint32_t)1 << w) - 1u);
    }
    idx[f] = (int32_t)v;
  }
}

// ---------------------------------------------------------------------------
// Ragged (CSR) blocks, DESIGN.md 4d.  Block g is dims [block_off[g],
// block_off[g + 1]); a negative length counts as 0 everywhere (and is reported
// through VbcFacts::bad_len).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int64_t vbc_len(const int64_t* __restrict__ off, int64_t g) {
  const int64_t d = off[g + 1] - off[g];
  return d > 0 ? d : 0;
}

// The budget of each ragged block.  A wave per block: the lanes compute 64
// dims' float32 KLs at once, the float64 sum then takes them in dim order
// (every lane keeps the same sum), which is k_block_bits's arithmetic without
// one lane walking a 4,095-dim group alone.
__global__ void __launch_bounds__(kVbThreads) k_block_bits_csr(
    const float* __restrict__ q_loc, const float* __restrict__ q_scale,
    const float* __restrict__ p_loc, const float* __restrict__ p_scale,
    const int64_t* __restrict__ block_off, int64_t nb, double extra_bits, double n_steps,
    int32_t min_bits, int32_t max_bits, int32_t* __restrict__ bits_out,
    float* __restrict__ kl_bits_out) {
  constexpr int kWaves = kVbThreads / 64;
  const int lane = threadIdx.x & 63;
  for (int64_t g = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); g < nb;
       g += (int64_t)gridDim.x * kWaves) {  // wave-uniform
    const int64_t o = block_off[g];
    const int64_t d = vbc_len(block_off, g);
    double S = 0.0;
    for (int64_t j0 = 0; j0 < d; j0 += 64) {
      const int64_t j = j0 + lane;
      float v = 0.0f;
      if (j < d) v = kl_normal_normal_1(q_loc[o + j], q_scale[o + j], p_loc[o + j], p_scale[o + j]);
      const int n = d - j0 < 64 ? (int)(d - j0) : 64;
#pragma unroll
      for (int k = 0; k < 64; ++k)
        if (k < n) S = S + (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
    }
    const double kl_bits = S / 0.6931471805599453;  // log(2.0)
    int32_t b = max_bits;                           // a non-finite sum: the most we may spend
    if (S - S == 0.0) {
      const double v = ceil((kl_bits + extra_bits) / n_steps);
      b = v < (double)min_bits ? min_bits : (v > (double)max_bits ? max_bits : (int32_t)v);
    }
    if (lane == 0) {
      bits_out[g] = b;
      if (kl_bits_out) kl_bits_out[g] = (float)kl_bits;
    }
  }
}

// Per bucket: the dims it holds and its longest block; per tile of the sorted
// order: its dims.  Workgroup w covers the sorted rows [w kVbTile, (w + 1)
// kVbTile) and writes wg[w][0..31] (dims by bucket), wg[w][32..63] (longest),
// wg[w][64] (blocks of negative length) and wg[w][65] (the tile's dims):
// integer LDS atomics only.

__global__ void __launch_bounds__(kVbThreads) k_vbc_tile(const int32_t* __restrict__ bits,
                                                         const int64_t* __restrict__ block_off,
                                                         const int32_t* __restrict__ perm,
                                                         int64_t nb,
                                                         unsigned long long* __restrict__ wg) {
  __shared__ unsigned long long h[kVbcFactsRow];
  if (threadIdx.x < kVbcFactsRow) h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kVbTile;
  for (int i = threadIdx.x; i < kVbTile; i += kVbThreads) {
    const int64_t r = r0 + i;
    if (r < nb) {
      const int64_t g = perm[r];
      const int bin = vb_bin(bits[g]);
      if (block_off[g + 1] < block_off[g]) atomicAdd(&h[2 * kVbBins], 1ull);
      const unsigned long long d = (unsigned long long)vbc_len(block_off, g);
      atomicAdd(&h[bin], d);
      atomicMax(&h[kVbBins + bin], d);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int b = 0; b < kVbBins; ++b) t += h[b];
    h[2 * kVbBins + 1] = t;
  }
  __syncthreads();
  if (threadIdx.x < kVbcFactsRow)
    wg[(int64_t)blockIdx.x * kVbcFactsRow + threadIdx.x] = h[threadIdx.x];
}

// One workgroup: the tiles' rows to the call's facts, with the buckets' first
// rows and first dims (exclusive scans over the 32 buckets), and the tiles'
// dims to their exclusive scan partial[] (k_vb_off_scan's loop), the total to
// off_end (soff[nb]).
__global__ void __launch_bounds__(kVbThreads) k_vbc_reduce(
    const unsigned long long* __restrict__ wg, int64_t nwg, const uint32_t* __restrict__ counts,
    VbcFacts* __restrict__ facts, int64_t* __restrict__ partial, int64_t* __restrict__ off_end) {
  __shared__ unsigned long long acc[kVbcFactsRow];
  __shared__ int64_t lds[kVbThreads];
  const int c = threadIdx.x;
  if (c <= 2 * kVbBins) {
    const bool is_max = c >= kVbBins && c < 2 * kVbBins;
    unsigned long long a = 0;
    for (int64_t w = 0; w < nwg; ++w) {
      const unsigned long long v = wg[w * kVbcFactsRow + c];
      a = is_max ? (v > a ? v : a) : a + v;
    }
    acc[c] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t pre = 0;
    uint32_t start = 0;
    for (int b = 0; b < kVbBins; ++b) {
      facts->dims[b] = (int64_t)acc[b];
      facts->maxd[b] = (int64_t)acc[kVbBins + b];
      facts->pre[b] = pre;
      facts->counts[b] = counts[b];
      facts->start[b] = start;
      pre += (int64_t)acc[b];
      start += counts[b];
    }
    facts->bad_len = (int64_t)acc[2 * kVbBins];
  }
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < nwg; c0 += kVbThreads) {
    const int64_t w = c0 + threadIdx.x;
    const int64_t v = w < nwg ? (int64_t)wg[w * kVbcFactsRow + 2 * kVbBins + 1] : 0;
    const int64_t incl = wg_incl_scan(v, lds);
    if (w < nwg) partial[w] = carry + incl - v;
    lds[threadIdx.x] = incl;
    __syncthreads();
    carry += lds[kVbThreads - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) *off_end = carry;
}

// Sorted offsets: each tile's own scan of the lengths in sorted order on top
// of its base (k_vb_off_final's pattern), and everything else a row needs.
__global__ void __launch_bounds__(kVbThreads) k_vbc_soff_final(
    const int32_t* __restrict__ bits, const int64_t* __restrict__ block_off,
    const int32_t* __restrict__ perm, int64_t nb, const int64_t* __restrict__ partial,
    const VbcFacts* __restrict__ facts, int32_t seed, int64_t block_id_base,
    int64_t* __restrict__ soff, int64_t* __restrict__ roff, int64_t* __restrict__ src,
    int32_t* __restrict__ seeds) {
  __shared__ int64_t lds[kVbThreads];
  const int64_t r0 = (int64_t)blockIdx.x * kVbTile + (int64_t)threadIdx.x * kVbPerThread;
  int64_t len[kVbPerThread];
  int64_t sum = 0;
#pragma unroll
  for (int k = 0; k < kVbPerThread; ++k) {
    len[k] = r0 + k < nb ? vbc_len(block_off, perm[r0 + k]) : 0;
    sum += len[k];
  }
  int64_t run = partial[blockIdx.x] + wg_incl_scan(sum, lds) - sum;
#pragma unroll
  for (int k = 0; k < kVbPerThread; ++k) {
    const int64_t r = r0 + k;
    if (r < nb) {
      const int64_t g = perm[r];
      const int bin = vb_bin(bits[g]);
      const int64_t pre = facts->pre[bin];
      soff[r] = run;
      roff[r + bin] = run - pre;
      if (r + 1 == (int64_t)facts->start[bin] + facts->counts[bin])  // the bucket's last row
        roff[r + bin + 1] = run + len[k] - pre;
      src[r] = block_off[g];
      seeds[r] = block_seed(seed, block_id_base + g);
    }
    run += len[k];
  }
}

// Segmented gather and scatter: a thread per sorted dim finds its row by binary
// search in soff (rows of 0 dims share their successor's offset and are never
// found).
__global__ void __launch_bounds__(kVbThreads) k_vbc_gather(
    const float* __restrict__ a0, const float* __restrict__ a1, const float* __restrict__ a2,
    const float* __restrict__ a3, const int64_t* __restrict__ soff,
    const int64_t* __restrict__ src, int64_t nb, int64_t cap, float* __restrict__ o0,
    float* __restrict__ o1, float* __restrict__ o2, float* __restrict__ o3) {
  const int64_t total = soff[nb] < cap ? soff[nb] : cap;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = vb_last_le(soff, nb + 1, i);  // < nb: soff[nb] > i
    const int64_t s = src[r] + (i - soff[r]);
    o0[i] = a0[s];
    o1[i] = a1[s];
    o2[i] = a2[s];
    o3[i] = a3[s];
  }
}

__global__ void __launch_bounds__(kVbThreads) k_vbc_scatter(
    const float* __restrict__ sample_s, const int32_t* __restrict__ idx_s,
    const int64_t* __restrict__ soff, const int64_t* __restrict__ src,
    const int32_t* __restrict__ perm, int64_t nb, int64_t cap, int64_t n_steps,
    float* __restrict__ out_sample, int32_t* __restrict__ out_idx) {
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t total = soff[nb] < cap ? soff[nb] : cap;
  for (int64_t i = t0; i < total; i += stride) {
    const int64_t r = vb_last_le(soff, nb + 1, i);
    out_sample[src[r] + (i - soff[r])] = sample_s[i];
  }
  const int64_t ni = nb * n_steps;
  for (int64_t i = t0; i < ni; i += stride) {
    int64_t r, s;
    vb_row_of(i, n_steps, r, s);
    out_idx[(int64_t)perm[r] * n_steps + s] = idx_s[i];
  }
}

// ---------------------------------------------------------------------------
// Backfitting under budgets: an index table's rows into sorted
// order with the range check folded in, and a block's value and accept count
// back to caller order.  An entry of block g fails when it lies outside
// [0, 2^bits[g]); a block whose count is itself out of range is not tested (the
// sort reports it).  The failures are summed in LDS and reach *bad, which the
// launcher zeroed, by one integer add per workgroup that saw any.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kVbThreads) k_vb_gather_table(
    const int32_t* __restrict__ idx, const int32_t* __restrict__ bits,
    const int32_t* __restrict__ perm, int64_t nb, int64_t n_steps, int32_t* __restrict__ idx_s,
    uint32_t* __restrict__ bad) {
  __shared__ uint32_t fails;
  if (threadIdx.x == 0) fails = 0;
  __syncthreads();
  const int64_t ni = nb * n_steps;
  uint32_t mine = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ni;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r, s;
    vb_row_of(i, n_steps, r, s);
    const int64_t g = perm[r];
    const int32_t v = idx[g * n_steps + s];
    const int32_t b = bits[g];
    if (b >= 0 && b <= kVbMaxBits && (v < 0 || v >= ((int32_t)1 << b))) ++mine;
    idx_s[i] = v;
  }
  if (mine) atomicAdd(&fails, mine);
  __syncthreads();
  if (threadIdx.x == 0 && fails) atomicAdd(bad, fails);
}

__global__ void __launch_bounds__(kVbThreads) k_vb_scatter_blocks(
    const float* __restrict__ value_s, const int32_t* __restrict__ count_s,
    const int32_t* __restrict__ perm, int64_t nb, float* __restrict__ out_value,
    int32_t* __restrict__ out_count) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nb;
       r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = perm[r];
    if (out_value) out_value[g] = value_s[r];
    if (out_count) out_count[g] = count_s[r];
  }
}

bool aligned16_all(const void* a, const void* b, const void* c, const void* d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15u) == 0;
}


}  // namespace

hipError_t launch_block_bits(const float* q_loc, const float* q_scale, const float* p_loc,
                             const float* p_scale, int64_t nb, int64_t d, double extra_bits,
                             int32_t min_bits, int32_t max_bits, int32_t* bits_out,
                             float* kl_bits_out, hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  const bool vec = d % 4 == 0 && aligned16_all(q_loc, q_scale, p_loc, p_scale);
  hipLaunchKernelGGL(vec ? k_block_bits<true> : k_block_bits<false>,
                     dim3(grid_for(nb, kVbThreads, 65536)), dim3(kVbThreads), 0, stream, q_loc,
                     q_scale, p_loc, p_scale, nb, d, extra_bits, min_bits, max_bits, bits_out,
                     kl_bits_out);
  return hipGetLastError();
}


hipError_t launch_vb_sort(const int32_t* bits, int64_t nb, int32_t* perm, uint32_t* wg_hist,
                          uint32_t* counts, hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  const int64_t nwg = vb_tiles(nb);
  if (nb > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vb_hist, dim3((unsigned)nwg), dim3(kVbThreads), 0, stream, bits, nb,
                     wg_hist);
  hipLaunchKernelGGL(k_vb_scan, dim3(1), dim3(kVbThreads), 0, stream, wg_hist, nwg, counts);
  hipLaunchKernelGGL(k_vb_rank, dim3((unsigned)nwg), dim3(kVbThreads), 0, stream, bits, nb,
                     (const uint32_t*)wg_hist, perm);
  return hipGetLastError();
}

hipError_t launch_vb_gather(const float* t_loc, const float* t_scale, const float* p_loc,
                            const float* p_scale, const int32_t* perm, int64_t nb, int64_t d,
                            int32_t seed, int64_t block_id_base, float* t_loc_s, float* t_scale_s,
                            float* p_loc_s, float* p_scale_s, int32_t* seeds_s,
                            hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  const bool vec = d % 4 == 0 && aligned16_all(t_loc, t_scale, p_loc, p_scale) &&
                   aligned16_all(t_loc_s, t_scale_s, p_loc_s, p_scale_s);
  if (vec) {
    const int64_t dv = d / 4;
    hipLaunchKernelGGL(k_vb_gather<float4>, dim3(grid_for(nb * (dv > 0 ? dv : 1), kVbThreads, 1u << 20)),
                       dim3(kVbThreads), 0, stream, (const float4*)t_loc, (const float4*)t_scale,
                       (const float4*)p_loc, (const float4*)p_scale, perm, nb, dv, seed,
                       block_id_base, (float4*)t_loc_s, (float4*)t_scale_s, (float4*)p_loc_s,
                       (float4*)p_scale_s, seeds_s);
  } else {
    hipLaunchKernelGGL(k_vb_gather<float>, dim3(grid_for(nb * d, kVbThreads, 1u << 20)),
                       dim3(kVbThreads), 0, stream, t_loc, t_scale, p_loc, p_scale, perm, nb, d,
                       seed, block_id_base, t_loc_s, t_scale_s, p_loc_s, p_scale_s, seeds_s);
  }
  return hipGetLastError();
}

hipError_t launch_vb_scatter(const float* sample_s, const int32_t* idx_s, const int32_t* perm,
                             int64_t nb, int64_t d, int n_steps, float* out_sample,
                             int32_t* out_idx, hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  const bool vec = d % 4 == 0 && aligned16_all(sample_s, out_sample, nullptr, nullptr);
  const int64_t dv = vec ? d / 4 : d;
  const int64_t work = nb * dv > nb * n_steps ? nb * dv : nb * n_steps;
  const unsigned grid = grid_for(work, kVbThreads, 1u << 20);
  if (vec) {
    hipLaunchKernelGGL(k_vb_scatter<float4>, dim3(grid), dim3(kVbThreads), 0, stream,
                       (const float4*)sample_s, idx_s, perm, nb, dv, (int64_t)n_steps,
                       (float4*)out_sample, out_idx);
  } else {
    hipLaunchKernelGGL(k_vb_scatter<float>, dim3(grid), dim3(kVbThreads), 0, stream, sample_s,
                       idx_s, perm, nb, dv, (int64_t)n_steps, out_sample, out_idx);
  }
  return hipGetLastError();
}


// The out-of-range flag of launch_vb_offsets, zeroed by a launch: pack and
// unpack can be captured, and a captured sequence holds no memset node
// (DESIGN.md 4 "Graph replay").
static __global__ void k_vb_flag_reset(uint32_t* __restrict__ flag) {
  if (threadIdx.x == 0) *flag = 0u;
}

hipError_t launch_vb_offsets(const int32_t* bits, int64_t nb, int n_steps, int64_t* off,
                             int64_t* partial, uint32_t* flag, int64_t* total_out,
                             hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  if (nb > 0x7fffffff) return hipErrorInvalidValue;
  const int64_t nwg = vb_tiles(nb);
  hipLaunchKernelGGL(k_vb_flag_reset, dim3(1), dim3(64), 0, stream, flag);
  hipLaunchKernelGGL(k_vb_off_partial, dim3((unsigned)nwg), dim3(kVbThreads), 0, stream, bits, nb,
                     (int64_t)n_steps, partial, flag);
  hipLaunchKernelGGL(k_vb_off_scan, dim3(1), dim3(kVbThreads), 0, stream, partial, nwg,
                     (const uint32_t*)flag, off + nb, total_out);
  hipLaunchKernelGGL(k_vb_off_final, dim3((unsigned)nwg), dim3(kVbThreads), 0, stream, bits, nb,
                     (int64_t)n_steps, (const int64_t*)partial, off);
  return hipGetLastError();
}

hipError_t launch_vb_pack(const int32_t* idx, const int32_t* bits, const int64_t* off, int64_t nb,
                          int n_steps, uint8_t* out, int64_t out_cap, hipStream_t stream) {
  if (nb <= 0 || out_cap <= 0) return hipSuccess;
  const int64_t n_words = (out_cap + 3) / 4;
  hipLaunchKernelGGL(k_vb_pack, dim3(grid_for(n_words, kVbThreads, 1u << 20)), dim3(kVbThreads),
                     0, stream, idx, bits, off, nb, (int64_t)n_steps, out, out_cap, n_words,
                     ((uintptr_t)out & 3u) == 0 ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_vb_unpack(const uint8_t* bytes, int64_t n_bytes, const int32_t* bits,
                            const int64_t* off, int64_t nb, int n_steps, int32_t* idx,
                            hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_vb_unpack, dim3(grid_for(nb * n_steps, kVbThreads, 1u << 20)),
                     dim3(kVbThreads), 0, stream, bytes, n_bytes, bits, off, nb, (int64_t)n_steps,
                     idx);
  return hipGetLastError();
}

hipError_t launch_block_bits_csr(const float* q_loc, const float* q_scale, const float* p_loc,
                                 const float* p_scale, const int64_t* block_off, int64_t nb,
                                 double extra_bits, int n_steps, int32_t min_bits,
                                 int32_t max_bits, int32_t* bits_out, float* kl_bits_out,
                                 hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_block_bits_csr, dim3(grid_for(nb, kVbThreads / 64, 65536)),
                     dim3(kVbThreads), 0, stream, q_loc, q_scale, p_loc, p_scale, block_off, nb,
                     extra_bits, (double)n_steps, min_bits, max_bits, bits_out, kl_bits_out);
  return hipGetLastError();
}


hipError_t launch_vbc_layout(const int32_t* bits, const int64_t* block_off, const int32_t* perm,
                             int64_t nb, const uint32_t* counts, unsigned long long* wg,
                             VbcFacts* facts, int32_t seed, int64_t block_id_base, int64_t* soff,
                             int64_t* roff, int64_t* src, int32_t* seeds, int64_t* partial,
                             hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  if (nb > 0x7fffffff) return hipErrorInvalidValue;
  const int64_t nwg = vb_tiles(nb);
  hipLaunchKernelGGL(k_vbc_tile, dim3((unsigned)nwg), dim3(kVbThreads), 0, stream, bits,
                     block_off, perm, nb, wg);
  hipLaunchKernelGGL(k_vbc_reduce, dim3(1), dim3(kVbThreads), 0, stream,
                     (const unsigned long long*)wg, nwg, counts, facts, partial, soff + nb);
  hipLaunchKernelGGL(k_vbc_soff_final, dim3((unsigned)nwg), dim3(kVbThreads), 0, stream, bits,
                     block_off, perm, nb, (const int64_t*)partial, (const VbcFacts*)facts, seed,
                     block_id_base, soff, roff, src, seeds);
  return hipGetLastError();
}

hipError_t launch_vbc_gather(const float* t_loc, const float* t_scale, const float* p_loc,
                             const float* p_scale, const int64_t* soff, const int64_t* src,
                             int64_t nb, int64_t cap, float* t_loc_s, float* t_scale_s,
                             float* p_loc_s, float* p_scale_s, hipStream_t stream) {
  if (nb <= 0 || cap <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_vbc_gather, dim3(grid_for(cap, kVbThreads, 1u << 20)), dim3(kVbThreads), 0,
                     stream, t_loc, t_scale, p_loc, p_scale, soff, src, nb, cap, t_loc_s,
                     t_scale_s, p_loc_s, p_scale_s);
  return hipGetLastError();
}

hipError_t launch_vbc_scatter(const float* sample_s, const int32_t* idx_s, const int64_t* soff,
                              const int64_t* src, const int32_t* perm, int64_t nb, int64_t cap,
                              int n_steps, float* out_sample, int32_t* out_idx,
                              hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  const int64_t work = cap > nb * n_steps ? cap : nb * n_steps;
  hipLaunchKernelGGL(k_vbc_scatter, dim3(grid_for(work, kVbThreads, 1u << 20)), dim3(kVbThreads),
                     0, stream, sample_s, idx_s, soff, src, perm, nb, cap, (int64_t)n_steps,
                     out_sample, out_idx);
  return hipGetLastError();
}

hipError_t launch_vb_gather_table(const int32_t* idx, const int32_t* bits, const int32_t* perm,
                                  int64_t nb, int n_steps, int32_t* idx_s, uint32_t* bad,
                                  hipStream_t stream) {
  if (nb <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(bad, 0, 4, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_vb_gather_table, dim3(grid_for(nb * n_steps, kVbThreads, 1u << 16)),
                     dim3(kVbThreads), 0, stream, idx, bits, perm, nb, (int64_t)n_steps, idx_s,
                     bad);
  return hipGetLastError();
}

hipError_t launch_vb_scatter_blocks(const float* value_s, const int32_t* count_s,
                                    const int32_t* perm, int64_t nb, float* out_value,
                                    int32_t* out_count, hipStream_t stream) {
  if (nb <= 0 || (!out_value && !out_count)) return hipSuccess;
  hipLaunchKernelGGL(k_vb_scatter_blocks, dim3(grid_for(nb, kVbThreads, 1u << 16)),
                     dim3(kVbThreads), 0, stream, value_s, count_s, perm, nb, out_value,
                     out_count);
  return hipGetLastError();
}

}  // namespace cwq
