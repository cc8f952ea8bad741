// cwq_kernels.h -- launchers shared between the kernels and the C ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cwq_dispatch.h"
#include "cwq_workspace.h"
#include "cwq_budget_plan.h"

namespace cwq {

// Records `msg` for cwq_last_error() (thread-local) and returns `code`.
int set_error(int code, const char* msg);

// First entry of a long block's visit-order records (abp, 32 B per entry) for a
// block at absolute dim offset off (csr_rec_entries, cwq_workspace.h, sizes the
// array: each long block gets a disjoint region of d + 12 entries).
__host__ __device__ inline int64_t csr_rec_base(int64_t off) {
  return off + 12 * (off / (CWQ_CSR_LDS_DIMS + 1));
}

struct EncodeArgs {
  const float* t_loc;
  const float* t_scale;
  const float* p_loc;
  const float* p_scale;
  const int64_t* block_off;  // nullptr -> uniform blocks of dimension ud
  int64_t ud;
  int64_t nb;
  int64_t total_dims;
  int64_t max_d;             // longest block (uniform: ud); -1: unknown
  int64_t n_cand;            // 2^n_bits_per_step
  int64_t tiles_per_block;
  int64_t cand_per_tile;     // multiple of 256
  int n_steps;
  int prune;                 // 1: use the pruned kernel where it applies
  int tau_guess = -1;        // k_encode_prune's tau guess: -1 = on where prune >= 2; 0, 1, 2
  int32_t seed;
  float rho;
  int64_t block_id_base;
  const int32_t* seeds;      // device [nb] per-block seeds, or nullptr: seed + block_id_base + g
  int32_t* out_idx;
  float* out_sample;
  // workspace
  unsigned long long* keys;  // [nb]
  // tile queue counters of k_encode_prune (kTileQueueSlots u32, one per fork
  // part; nullptr: static tile loop); zeroed by the launcher before each launch
  uint32_t* tq = nullptr;
  // deferred exact work of k_encode_prune's one-tile-per-block launches
  // (defer_ws, cwq_workspace.h); nullptr: the single launch.  defer_mode: -1 the
  // launcher's rule, 0 off, 1 on, 2 every tile deferred, 3 Q = 0 (tests)
  uint32_t* defer_surv = nullptr;
  uint32_t* defer_count = nullptr;
  uint32_t* defer_list = nullptr;
  uint32_t* defer_dcount = nullptr;
  int defer_mode = -1;
  float* loc_s;              // [total_dims]
  float* scale_s;            // [total_dims]
  float* lognorm;            // [total_dims]
  // screening constants of the general pruned kernel (k_encode_prune_csr):
  // there iff has_screen_arrays (cwq_dispatch.h), which sizes the workspace
  // and picks the path; the launchers only check that they were given
  float2* sab;               // [total_dims + 8 nb] (sA, sB), 4 zero pads either side per block
  float* cdim;               // [total_dims] C_j of the screening bound (k_csr_prep scratch)
  float* bpre;               // [total_dims + 12 nb] drop bounds per visit position (k_csr_prep)
  uint32_t* ordu;            // [total_dims + 12 nb] unit visited at each position
  float4* grp;               // [nb] (c1, c2, As, Pq); c1 == 0: block not screened
  uint32_t* gtau;            // [nb] per-block shared threshold (ord)
  float4* abp;               // [2 (total_dims + 12 nb)] visit-order (sa, sb) records of the
                             // blocks longer than CWQ_CSR_LDS_DIMS; there iff
                             // has_long_block_records, else nullptr
  uint2* slist;              // screened small-candidate path: CWQ_SLIST_PER_BLOCK
                             // (row, upper bits) survivor slots per block; the
                             // per-block counts live in ordu[off + 12 g]
  // optional profiling events around the eval launches (hipEvent_t)
  void* ev_start;
  void* ev_stop;
  // the small-candidate pipeline (k_small_*; there iff has_screen_arrays):
  // per-dim screening constants (sA, sB) by absolute dim offset (a view of
  // sab, set by launch_encode) and the dim -> block map [total_dims]
  const float2* pre_ab = nullptr;
  uint32_t* sdmap = nullptr;
  // grouped pipelines (coded_greedy_sampler.py:292): also ds_out[i] =
  // ds_scale[i] * sample[i] + ds_loc[i] after the last step, folded into the
  // small pipeline's finalize where it runs, else one k_destandardise
  float* ds_out = nullptr;
  const float* ds_loc = nullptr;
  const float* ds_scale = nullptr;
  // score every candidate row exactly with a whole wave (k_encode_rows_wave)
  // instead of any other scoring path; results are those of prune == 0
  bool rows_wave = false;
};

// Library copy streams (which = 0: device to host, 1: host to device) on the
// device of the caller's stream, created once per host thread; nullptr if they
// cannot be made.  Used by the pipelined batch coder to overlap its copies with
// the coding on the caller's stream.
hipStream_t copy_stream(hipStream_t stream, int which);
hipError_t launch_encode(const EncodeArgs& a, hipStream_t stream);
hipError_t launch_decode(const int32_t* idx, const float* p_loc, const float* p_scale,
                         const int64_t* block_off, int64_t ud, int64_t nb, int64_t total_dims,
                         int n_bits,
                         int n_steps, int32_t seed, float rho, int64_t block_id_base,
                         float* out_sample, hipStream_t stream);
// Grouped decode on the standard proposal, destandardisation fused
// (k_decode_csr_q4): slot_off is the prefix of decode_csr_slots(d_g) over the nb
// groups (nb + 1 entries, n_slots its last), block_seeds the per-group seeds [nb].
__host__ __device__ inline int64_t decode_csr_slots(int64_t d) {
  return d > 0 ? ((d + 3) >> 2) + 1 : 0;  // the row's Philox blocks at any alignment
}
hipError_t launch_decode_csr_q4(const int32_t* idx, const int64_t* block_off,
                                const int64_t* slot_off, int64_t nb, int64_t n_slots,
                                const int32_t* block_seeds, int n_bits, int n_steps, float rho,
                                const float* dst_loc, const float* dst_scale, float* out,
                                hipStream_t stream);
hipError_t launch_stateless_normal_sample(const float* loc, const float* scale, int64_t d,
                                          int64_t num_samples, int32_t seed, float* out,
                                          hipStream_t stream);
hipError_t launch_standardise(const float* q_loc, const float* q_scale, const float* p_loc,
                              const float* p_scale, int64_t n, float* t_loc, float* t_scale,
                              hipStream_t stream);
hipError_t launch_kl(const float* q_loc, const float* q_scale, const float* p_loc,
                     const float* p_scale, int64_t n, float* out, hipStream_t stream);
hipError_t launch_destandardise(const float* sample, const float* p_loc, const float* p_scale,
                                int64_t n, float* out, hipStream_t stream);
// the grouped importance coder's standardise + KL + outliers + standard prior
// + KL against N(0, 1) + the outlier dims' target draw (seed - 1 per item:
// item_off / seed1 device arrays of a batch, or item_off == nullptr and
// seed1_one for one item), one launch (cwq_code_grouped_importance[_batch])
hipError_t launch_imp_grouped_prep(const float* q_loc, const float* q_scale, const float* p_loc,
                                   const float* p_scale, int64_t n, float limit,
                                   const int64_t* item_off, const int32_t* seed1, int64_t n_items,
                                   int32_t seed1_one, float* t_loc, float* t_scale, uint8_t* keep,
                                   float* zeros, float* ones, float* kl2, float* tsamp,
                                   hipStream_t stream);
// standardise + KL + the standard prior's zeros/ones + nz zeroed u64 at zinfo
// (nz <= 256), one launch (the grouped coder's first step)
hipError_t launch_grouped_prep(const float* q_loc, const float* q_scale, const float* p_loc,
                               const float* p_scale, int64_t n, float* t_loc, float* t_scale,
                               float* kl, float* zeros, float* ones, unsigned long long* zinfo,
                               int nz, hipStream_t stream);

// The grouped coder's greedy partition on the device (cwq_partition.hip), of
// one item (item_off == nullptr, n_items == 1) or of each item [item_off[k],
// item_off[k+1]) of a batch (device offsets): item k's starts at starts +
// item_off[k] + 2 k, iinfo[2k] their count (G + 1), iinfo[2k + 1] its largest
// group (iinfo holds 4 n_items entries: the rest is scratch).  partition_fell_back(info copied to the host): not covered, the caller
// runs the host loop (the results never depend on which path ran).
bool partition_applies(int64_t D, int64_t size_threshold);
// One item of a batch in the device layout of its chunk's encode: its G groups
// go to offs[go ...] (block offsets relative to the chunk's first dim: rel +
// its starts at dstarts[src ...]) and seeds[gs ...] (seed + g, :282); term >= 0:
// offs[term] = dc, the chunk's closing offset (written with the chunk's last item).
struct BatchItem {
  int64_t src, rel, go, gs, G, term, dc;
  int64_t pk, ns;  // the item's start list: packed offset and length (pstarts)
  int32_t seed, pad;
};
static_assert(sizeof(BatchItem) == kBatchItemBytes, "batch_ws sizes the layout table by it");
// pstarts (may be nullptr): every item's start list packed back to back, for
// one device-to-host copy
hipError_t launch_batch_layout(const BatchItem* items, int64_t n_items, const int64_t* dstarts,
                               int64_t* offs, int32_t* seeds, int64_t* pstarts,
                               hipStream_t stream);
// ws: part_ws(D).total bytes.  info_zeroed: info[0..7] (and, single item, iinfo[0..1]) were zeroed on the
// stream by the caller (launch_grouped_prep); otherwise a memset does it
hipError_t launch_partition(const float* kl, int64_t D, const int64_t* item_off, int64_t n_items,
                            int64_t size_threshold, float thr, int64_t* starts, int64_t* iinfo,
                            void* ws, unsigned long long* info, hipStream_t stream,
                            bool info_zeroed = false);
bool partition_fell_back(const unsigned long long* info_host);

hipError_t launch_imp_outliers(const float* kl, int64_t n, float limit, float* t_loc,
                               float* t_scale, uint8_t* keep, hipStream_t stream);
hipError_t launch_importance_encode(const float* t_loc, const float* t_scale, const float* p_loc,
                                    const float* p_scale, const int64_t* block_off,
                                    const int64_t* n_samples, int64_t nb, int64_t total_dims,
                                    int32_t seed, int64_t block_id_base,
                                    const int32_t* block_seeds, int allow_screen,
                                    int64_t* out_index, float* out_sample,
                                    void* workspace,  // imp_ws(nb, total_dims).total bytes
                                    hipStream_t stream, int64_t total_cands = -1,
                                    int64_t total_tiles = -1, const float* dst_loc = nullptr,
                                    const float* dst_scale = nullptr, float* dst_out = nullptr);
// The encode launch's k_imp_eval tile count from host copies of the plan
// (total_cands: sum of max(N_g, 1)); it only selects the tile hand-out.
int64_t importance_tile_count(const int64_t* n_samples_host, int64_t nb, int64_t total_cands);
hipError_t launch_importance_decode(const int64_t* index, const float* p_loc,
                                    const float* p_scale, const int64_t* block_off, int64_t nb,
                                    int32_t seed, int64_t block_id_base, float* out_sample,
                                    hipStream_t stream);
// Grouped decode of a batch: rows of the standard proposal N(0, 1) with
// per-group seeds, destandardised by dst_loc / dst_scale into dst_out.
hipError_t launch_importance_decode_grouped(const int64_t* index, const int64_t* block_off,
                                            int64_t nb, const int32_t* block_seeds,
                                            const float* dst_loc, const float* dst_scale,
                                            float* dst_out, hipStream_t stream);

// ---- uniform blocks with per-block bit budgets (cwq_varbits.hip) ----------
// bits_out[g] = clamp(ceil(KL_g / ln 2 + extra_bits), min_bits, max_bits), KL_g
// the float64 sum of block g's float32 per-dim KLs; kl_bits_out (or nullptr):
// KL_g / ln 2 as float32.
hipError_t launch_block_bits(const float* q_loc, const float* q_scale, const float* p_loc,
                             const float* p_scale, int64_t nb, int64_t d, double extra_bits,
                             int32_t min_bits, int32_t max_bits, int32_t* bits_out,
                             float* kl_bits_out, hipStream_t stream);
// Stable counting sort of nb <= 2^31 - 1 blocks by bit count: perm[rank] = g,
// counts[0..30] the blocks of each count, counts[31] those outside [0, 30]
// (ranked last).  wg_hist: vb_tiles(nb) * kVbBins u32 of scratch.
hipError_t launch_vb_sort(const int32_t* bits, int64_t nb, int32_t* perm, uint32_t* wg_hist,
                          uint32_t* counts, hipStream_t stream);
// Rows perm[r] of the four inputs to rows r of the sorted copies, and
// seeds_s[r] = block_seed(seed, block_id_base + perm[r]).
hipError_t launch_vb_gather(const float* t_loc, const float* t_scale, const float* p_loc,
                            const float* p_scale, const int32_t* perm, int64_t nb, int64_t d,
                            int32_t seed, int64_t block_id_base, float* t_loc_s, float* t_scale_s,
                            float* p_loc_s, float* p_scale_s, int32_t* seeds_s,
                            hipStream_t stream);
// Rows r of sample_s (d floats) and idx_s (n_steps int32) to rows perm[r].
hipError_t launch_vb_scatter(const float* sample_s, const int32_t* idx_s, const int32_t* perm,
                             int64_t nb, int64_t d, int n_steps, float* out_sample,
                             int32_t* out_idx, hipStream_t stream);
// off[0..nb]: exclusive scan of n_steps * bits[g] in block order (a count
// outside [0, 30] counts as 0 and sets *flag); total_out (or nullptr) receives
// off[nb], or -1 when the flag is set.  partial: vb_tiles(nb) i64 of scratch.
hipError_t launch_vb_offsets(const int32_t* bits, int64_t nb, int n_steps, int64_t* off,
                             int64_t* partial, uint32_t* flag, int64_t* total_out,
                             hipStream_t stream);
// The packed stream of idx [nb, n_steps] (binary_io._pack_bits of the joined
// to_bit_string fields), at most out_cap bytes of it, and its inverse (bytes
// past n_bytes read as 0).
hipError_t launch_vb_pack(const int32_t* idx, const int32_t* bits, const int64_t* off, int64_t nb,
                          int n_steps, uint8_t* out, int64_t out_cap, hipStream_t stream);
hipError_t launch_vb_unpack(const uint8_t* bytes, int64_t n_bytes, const int32_t* bits,
                            const int64_t* off, int64_t nb, int n_steps, int32_t* idx,
                            hipStream_t stream);

// ---- ragged (CSR) blocks with per-block bit budgets (cwq_varbits.hip) -----
// bits_out[g] = clamp(ceil((KL_g / ln 2 + extra_bits) / n_steps), min_bits,
// max_bits) of block g = dims [block_off[g], block_off[g + 1]).
hipError_t launch_block_bits_csr(const float* q_loc, const float* q_scale, const float* p_loc,
                                 const float* p_scale, const int64_t* block_off, int64_t nb,
                                 double extra_bits, int n_steps, int32_t min_bits,
                                 int32_t max_bits, int32_t* bits_out, float* kl_bits_out,
                                 hipStream_t stream);
// The sorted layout, from the sort's perm and counts: the facts (VbcFacts,
// cwq_budget_plan.h: what the host reads back, in one copy); soff[0..nb]
// the exclusive scan of the block lengths in sorted order; roff [nb + 33]:
// bucket b's own offsets, relative to its first dim, with a terminator of its
// own, at roff + start[b] + b (counts[b] + 1 entries); src[r] =
// block_off[perm[r]]; seeds[r] = block_seed(seed, block_id_base + perm[r]).
// wg: vb_tiles(nb) * kVbcFactsRow u64; partial: vb_tiles(nb) i64.
hipError_t launch_vbc_layout(const int32_t* bits, const int64_t* block_off, const int32_t* perm,
                             int64_t nb, const uint32_t* counts, unsigned long long* wg,
                             VbcFacts* facts, int32_t seed, int64_t block_id_base, int64_t* soff,
                             int64_t* roff, int64_t* src, int32_t* seeds, int64_t* partial,
                             hipStream_t stream);
// Sorted dim i of row r (soff[r] <= i < soff[r + 1]) is dim src[r] + i - soff[r]
// of the caller's arrays.  Nothing at or past sorted dim cap is touched.
hipError_t launch_vbc_gather(const float* t_loc, const float* t_scale, const float* p_loc,
                             const float* p_scale, const int64_t* soff, const int64_t* src,
                             int64_t nb, int64_t cap, float* t_loc_s, float* t_scale_s,
                             float* p_loc_s, float* p_scale_s, hipStream_t stream);
hipError_t launch_vbc_scatter(const float* sample_s, const int32_t* idx_s, const int64_t* soff,
                              const int64_t* src, const int32_t* perm, int64_t nb, int64_t cap,
                              int n_steps, float* out_sample, int32_t* out_idx,
                              hipStream_t stream);

// Backfitting under budgets.  Row r of idx_s = row perm[r] of
// the table idx [nb, n_steps]; *bad = the entries outside [0, 2^bits[g]) of
// their block g (blocks whose count is itself outside [0, 30] are not tested).
hipError_t launch_vb_gather_table(const int32_t* idx, const int32_t* bits, const int32_t* perm,
                                  int64_t nb, int n_steps, int32_t* idx_s, uint32_t* bad,
                                  hipStream_t stream);
// out_value[perm[r]] = value_s[r], out_count[perm[r]] = count_s[r] (either
// output may be nullptr).
hipError_t launch_vb_scatter_blocks(const float* value_s, const int32_t* count_s,
                                    const int32_t* perm, int64_t nb, float* out_value,
                                    int32_t* out_count, hipStream_t stream);

// ---- beam search over steps (cwq_beam.hip) -------------------
constexpr int kMaxBeam = 16;  // CWQ_MAX_BEAM
struct BeamArgs {
  const float* t_loc;
  const float* t_scale;
  const float* p_loc;
  const float* p_scale;
  const int64_t* block_off;  // nullptr -> uniform blocks of dimension ud
  int64_t ud, nb, total_dims, max_d;
  int n_bits, n_steps, beam;
  int32_t seed;
  float rho;
  int64_t block_id_base;
  int32_t* out_idx;
  float* out_sample;
  float* out_value;  // or nullptr
  void* workspace;   // beam_ws(nb, total_dims, n_steps, beam).total bytes
  void* ev_start;    // hipEvent_t around the scoring launches, or nullptr
  void* ev_stop;
  BeamPath path;
  bool quarter_tiles;  // tests: tiles a quarter of the size (same results)
  // cwq_beam_encode_var: the blocks' bit counts, device [nb];
  // n_bits is then max_bits, the bound the counts are read as clamped to.
  // nullptr: every block at n_bits.
  const int32_t* n_bits_dev = nullptr;
};
hipError_t launch_beam_encode(const BeamArgs& a, hipStream_t stream);

// ---- backfitting (cwq_backfit.hip) ---------------------------
// k_prep_dims: the shard constants and normalisers of every dim, out_sample = 0
// and keys = 0 (launch_encode's first launch).
hipError_t launch_prep_dims(const float* t_scale, const float* p_loc, const float* p_scale,
                            int64_t n, int n_steps, float rho, float* loc_s, float* scale_s,
                            float* lognorm, float* out_sample, unsigned long long* keys,
                            int64_t nb, hipStream_t stream);
// The scoring launches of step `step` alone, in the form of a step > 0 (every
// row is scored against a.out_sample, the carried vector) whatever the step's
// number: the block's best key lands in a.keys, which the caller zeroed; no
// index or sample is written.  The path is encode_plan's with keys_only set.
hipError_t launch_score_step(const EncodeArgs& a, int step, hipStream_t stream);
// rows, value, count: what a backfit call has beyond the encoder's arrays
// (backfit_ws, cwq_workspace.h)
struct BackfitArgs {
  EncodeArgs enc;      // the encoder's arguments; out_idx is the table (in and out),
                       // out_sample the carried vector between the launches and the result
  int sweeps;
  float* rows;
  float* value;
  int32_t* count;
  float* out_value;       // or nullptr
  int32_t* out_accepted;  // or nullptr
  BackfitPath path;
  // nullptr: one budget (enc.n_cand) for every block, one scoring launch
  // sequence per step.  Otherwise the call's buckets (each of at least one bit
  // and one block): a scoring launch sequence per step and bucket; blocks in no
  // bucket keep key 0, i.e. row 0.  Everything else covers all blocks at once.
  const BudgetBucket* buckets = nullptr;
  int n_buckets = 0;
};
hipError_t launch_backfit(const BackfitArgs& a, hipStream_t stream);

// ---- rate tables (cwq_ratetable.hip) ---------------------------
// The levels launch of plan p (rate_plan, cwq_rate_plan.h): the best key of
// every level of rows [0, 2^p.levels) of every block into lkeys [nb][kRateLevels],
// which the caller zeroed on the stream.  loc_s, scale_s, lognorm: k_prep_dims'
// arrays for n_steps = 1.
hipError_t launch_rate_levels(const RatePlan& p, const float* t_loc, const float* t_scale,
                              const float* loc_s, const float* scale_s, const float* lognorm,
                              const int64_t* block_off, int64_t ud, int32_t seed,
                              int64_t block_id_base, unsigned long long* lkeys,
                              hipStream_t stream);
// Columns 0 .. p.levels of out_idx / out_value [nb][max_bits + 1] from lkeys and
// columns p.high_first .. max_bits from hkeys [p.high_count][nb], the key
// columns the budgets' launch_encode calls left.
hipError_t launch_rate_fold(const RatePlan& p, const unsigned long long* lkeys,
                            const unsigned long long* hkeys, const int64_t* block_off, int64_t ud,
                            int64_t nb, int max_bits, int32_t* out_idx, float* out_value,
                            hipStream_t stream);
// out_bits[g] = the lowest b in [lo, hi] that maximises (double)value[g][b] -
// lam * (double)b over the table value [nb][n_cols]; *out_total (device, or
// nullptr) = their sum.
hipError_t launch_choose_bits(const float* value, int64_t nb, int n_cols, double lam, int lo,
                              int hi, int32_t* out_bits, int64_t* out_total, hipStream_t stream);
// launch_choose_bits at the price 60 halvings of [0, span] find for a total of at
// most `target` (ratetable.choose_bits_total's result; nb > 0):
// kSolveLaunches launches, *out_lam and *out_total are device words; state,
// prod and totals are solve_ws' regions, whatever they hold.
hipError_t launch_choose_bits_total(const float* value, int64_t nb, int n_cols, int64_t target,
                                    int lo, int hi, int32_t* out_bits, double* out_lam,
                                    int64_t* out_total, SolveState* state, double* prod,
                                    int64_t* totals, hipStream_t stream);
// out_idx[g] = tidx[g][bits[g]] over the table tidx [nb][n_cols]
hipError_t launch_rate_gather(const int32_t* tidx, const int32_t* bits, int64_t nb, int n_cols,
                              int32_t* out_idx, hipStream_t stream);

hipError_t launch_selftest_bm(uint32_t m0, int64_t count, float* rad, float* sn, float* cs,
                              hipStream_t stream);
hipError_t launch_selftest_screen(uint32_t m0, int64_t count, float* rad, float* sn, float* cs,
                                  hipStream_t stream);
int prune_stats(unsigned long long* out72, int reset);
int tile_times(unsigned long long* t0, unsigned long long* t1, unsigned int* wg, int n);
int quad_times(unsigned long long* t, unsigned int* info, int n);
hipError_t launch_selftest_wave_max(const float* x, int64_t nw, float* out, hipStream_t stream);
hipError_t launch_selftest_div(const float* a, const float* b, int64_t n, float* out,
                               hipStream_t stream);
hipError_t launch_selftest_logf(const float* x, int64_t n, float* out, hipStream_t stream);

}  // namespace cwq
