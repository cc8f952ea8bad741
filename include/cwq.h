/*
 * cwq.h -- C ABI of the MI355X (gfx950) greedy coded sampler (libcwq.so).
 *
 * Drop-in boundary for the reference's relative-entropy coding hot path.  The
 * reference has no native ABI (its sampler is a TF1 graph); each entry point
 * below replaces the graph op named next to it:
 *
 *   cwq_stateless_normal_sample  <- code/misc.py:3-17 stateless_normal_sample
 *                                   (tf.random.stateless_normal, seed=[seed,42],
 *                                   then scale*z and loc+ at misc.py:14-15)
 *   cwq_greedy_encode[_uniform]  <- code/coded_greedy_sampler.py:29-89
 *                                   code_greedy_sample, batched over the groups
 *                                   that code_grouped_greedy_sample (:170-296)
 *                                   feeds one sess.run at a time (:273-284);
 *                                   group g uses seed + block_id_base + g (:282)
 *   cwq_greedy_decode[_uniform]  <- code/coded_greedy_sampler.py:93-167
 *                                   decode_greedy_sample, batched the same way
 *                                   as decode_grouped_greedy_sample (:345-356)
 *   cwq_standardise              <- code/coded_greedy_sampler.py:193-199
 *   cwq_kl_normal_normal         <- code/coded_greedy_sampler.py:201
 *                                   (tfd.kl_divergence(target, proposal))
 *   cwq_destandardise            <- code/coded_greedy_sampler.py:292 / :362
 *   cwq_group_starts             <- code/coded_greedy_sampler.py:207-252
 *                                   (host-side sequential partition)
 *   cwq_code_grouped_greedy      <- code/coded_greedy_sampler.py:170-296
 *                                   (the whole grouped coder in one call)
 *   cwq_code_grouped_greedy_batch <- the same, once per item of a batch
 *   cwq_beam_encode              <- code/coded_greedy_sampler.py:29-89 with the B
 *                                   best partial sums kept after each step
 *                                   instead of one (not in the reference; its
 *                                   decoders read the result unchanged)
 *   cwq_decode_grouped_greedy_batch <- code/coded_greedy_sampler.py:299-364
 *                                   decode_grouped_greedy_sample, once per item
 *   cwq_decode_grouped_importance_batch <- code/coded_importance_sampler.py:
 *                                   277-363 decode_grouped_importance_sample
 *                                   (without the outlier overwrite), per item
 *
 * Conventions
 *   - All float/index pointers are DEVICE pointers (hipMalloc / torch cuda
 *     tensors) unless documented as host.  `stream` is a hipStream_t (NULL =
 *     default stream).  Calls are stream-ordered and asynchronous; no device
 *     memory is allocated and nothing synchronises (graph-capturable), except
 *     the host functions and the fused grouped pipelines documented as such.
 *     A multi-step CSR encode forks its two block halves onto two library
 *     streams (created once per host thread and device) and joins them back
 *     with events on the caller's stream.
 *   - `workspace` (device) and `host_workspace` (host) are scratch of at least
 *     the entry point's *_workspace_size bytes: their contents on entry are
 *     ignored (they may be uninitialised, or another call's leftovers) and are
 *     unspecified on return.  Output buffers are written in full, whatever they
 *     held: every element a call defines is stored (an empty block's index is
 *     0; out_sample is a sum over steps that starts from 0, not from the
 *     buffer); only capacity past the returned counts (bits_cap, starts_cap,
 *     out_cap) is left untouched.  tests/test_workspace_state_gpu.py holds
 *     every entry point to this, and tests/test_graph_replay_gpu.py holds the
 *     capturable ones to it under graph replay: each is captured once and
 *     replayed on outputs and workspaces overwritten between replays.
 *   - Blocks ("groups" in the reference) are described in CSR form:
 *     block g covers dims [block_off[g], block_off[g+1]) of the flat arrays;
 *     block_off is a device int64 array of nb+1 entries.  The *_uniform
 *     variants take a fixed block dimension instead.
 *   - target = posterior q (t_loc, t_scale); proposal = prior p (p_loc,
 *     p_scale), as in the reference's argument order.
 *   - Return value: 0 on success, a negative CWQ_ERR_* code otherwise; the
 *     message is available from cwq_last_error() (thread-local).  Nothing
 *     throws across this ABI.
 */
#ifndef CWQ_H_
#define CWQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CWQ_OK 0
#define CWQ_ERR_INVALID (-1)   /* bad argument (sizes, bits, null pointer) */
#define CWQ_ERR_HIP (-2)       /* HIP runtime error (launch, memset) */
#define CWQ_ERR_WORKSPACE (-3) /* workspace too small */
#define CWQ_ERR_CAPACITY (-4)  /* output buffer too small (retry with a larger one) */
#define CWQ_ERR_ALLOC (-5)     /* host allocation failed */

#define CWQ_MAX_BITS_PER_STEP 30

/* ABI version, (major << 16) | minor.  Bindings must refuse a library whose
 * cwq_version() differs from the header they were written against.
 *   0.2  per-call cwq_options before the stream in the encoders, a
 *        max_block_dim argument to cwq_greedy_encode_workspace_size, no
 *        process-wide tuning setters;
 *   0.3  cwq_code_grouped_greedy_begin / _end;
 *   0.4  per-item ready flags of the batched grouped coder
 *        (cwq_options.item_ready);
 *   0.5  CWQ_ERR_ALLOC (host allocation failures are returned, never thrown);
 *        starts_host of the grouped _begin calls is read asynchronously;
 *   0.6  cwq_code_grouped_importance_batch;
 *   0.7  cwq_decode_grouped_greedy_batch, cwq_decode_grouped_importance_batch;
 *   0.8  per-block bit budgets for uniform blocks: cwq_block_bits,
 *        cwq_greedy_encode_uniform_var, cwq_pack_indices_var,
 *        cwq_unpack_indices_var and their workspace sizes;
 *   0.9  per-block bit budgets for CSR blocks: cwq_block_bits_csr,
 *        cwq_greedy_encode_var and its workspace size;
 *   0.10 cwq_selftest_encode_rows_wave; cwq_greedy_encode_var codes buckets of
 *        long blocks below 4,096 candidates with a wave per candidate row
 *        (same results as before);
 *   0.11 beam search over the greedy coder's steps: cwq_beam_encode, its
 *        workspace size and cwq_selftest_beam_encode (no decoder change);
 *   0.12 backfitting: cwq_greedy_backfit and its workspace size (no decoder
 *        change);
 *   0.13 backfitting under per-block bit budgets: cwq_greedy_backfit_var (no
 *        new size function, no decoder change);
 *   0.14 cwq_selftest_encode_uniform_tau_guess (the pruned uniform encoder
 *        starts its threshold from a predicted level; same results);
 *   0.15 beam search under per-block bit budgets: cwq_beam_encode_var and
 *        cwq_selftest_beam_encode_var (no new size function, no decoder
 *        change; cwq_beam_encode's results are unchanged);
 *   0.16 cwq_greedy_encode_uniform_defer_bytes and
 *        cwq_selftest_encode_uniform_defer: cwq_greedy_encode_uniform takes a
 *        larger workspace and, given one, defers the pruned kernel's exact
 *        work to launches of its own (same results; every existing size
 *        function answers what it did);
 *   0.17 rate tables for single-step codes: cwq_rate_table,
 *        cwq_rate_table_workspace_bytes and cwq_choose_bits (no decoder
 *        change; every existing call's results and size functions are
 *        unchanged);
 *   0.18 budgets under a bit total, solved on the device: cwq_choose_bits_total,
 *        cwq_greedy_encode_rate and their workspace sizes (no decoder change;
 *        every existing call's results and size functions are unchanged). */
#define CWQ_ABI_VERSION ((0 << 16) | 18)
int cwq_version(void);

/* Thread-local description of the last error ("" if none). */
const char* cwq_last_error(void);

/* misc.py:3-17.  out[n*d + j] = loc[j] + scale[j] * Z[n*d + j] for
 * n < num_samples, j < d, where Z = tf.random.stateless_normal(
 * [num_samples, d], seed=[seed, 42]) (flat Philox4x32-10 + Box-Muller). */
int cwq_stateless_normal_sample(const float* loc, const float* scale, int64_t d,
                                int64_t num_samples, int32_t seed, float* out, void* stream);

/* Per-call options of the encoders (no process or thread state: every call
 * says what it wants; opts == NULL means the defaults below).
 *   prune_mode: 2 (default) = candidate pruning with the screening pass
 *               (DESIGN.md "screening bound") where a tile's constants allow
 *               it, exact pruning elsewhere; 1 = pruning on exact values only;
 *               0 = every candidate scored exactly.  Results never depend on
 *               it.  For the importance encoders, 2 turns on their screening
 *               pass, 0 and 1 score every candidate exactly.
 *   eval_start_event / eval_stop_event: hipEvent_t handles (both or neither)
 *               recorded on the call's stream right before the first
 *               candidate-scoring launch and right after the last one, so a
 *               caller can time the dominant kernel alone (bench.py).
 *   eval_ms_out: HOST float, or NULL.  The fused grouped calls
 *               (cwq_code_grouped_greedy[_batch], cwq_code_grouped_importance),
 *               which synchronise, write the summed milliseconds of their
 *               candidate-scoring launches (a pipelined batch codes in chunks:
 *               device gaps between them are excluded, unlike the event
 *               span).  Asynchronous entry points ignore it.
 *   item_ready: HOST int32 array of n_items flags, zeroed by the caller, or
 *               NULL.  cwq_code_grouped_greedy_batch sets flag i to 1 (a
 *               release store) as soon as item i's sample, bitcode, bits_off
 *               and starts are final in the host arrays, while later chunks
 *               still code; a caller running the call on another thread can
 *               consume the items as they complete (coded_greedy_sampler.py
 *               builds the bitcode strings this way).  The call itself still
 *               returns only when everything is done; on an error some flags
 *               stay 0.  Other entry points ignore it. */
typedef struct cwq_options {
  int32_t prune_mode;
  int32_t reserved; /* must be 0 */
  void* eval_start_event;
  void* eval_stop_event;
  float* eval_ms_out;
  int32_t* item_ready;
} cwq_options;
#define CWQ_OPTIONS_INIT {2, 0, NULL, NULL, NULL, NULL}

/* Workspace bytes needed by cwq_greedy_encode (CSR blocks) for nb blocks
 * holding total_dims dims in all, none longer than max_block_dim: the argmax
 * keys and per-dim shard constants plus the general pruned kernel's per-step
 * screening constants (24 B/dim + 244 B/block) and, when max_block_dim > 1024,
 * their visit-order copies for the long blocks (32 B/dim + 384 B per 1025
 * dims).  A
 * CSR call given less returns CWQ_ERR_WORKSPACE (it never silently falls back
 * to a slower kernel). */
size_t cwq_greedy_encode_workspace_size(int64_t nb, int64_t total_dims, int64_t max_block_dim);

/* Workspace bytes needed by cwq_greedy_encode_uniform for nb blocks of
 * dimension d: keys + shard constants only when d % 8 == 0, 8 <= d <= 64 (the
 * fast pruned kernel), the cwq_greedy_encode_workspace_size layout otherwise. */
size_t cwq_greedy_encode_uniform_workspace_size(int64_t nb, int64_t d);

/* Greedy coded sampling, encoder (coded_greedy_sampler.py:29-89) for nb
 * independent blocks.
 *   out_idx    [nb * n_steps] int32: the argmax index of every step (the
 *              reference emits these as LSB-first bit strings, :81-87)
 *   out_sample [total_dims] f32: best_sample of every block (:89)
 *   max_block_dim: an upper bound on the largest block's dimension (the same
 *              value the workspace was sized with).
 * Block g is coded with seed (seed + block_id_base + g) (int32 wrap), step i of
 * it with the stateless seed [1000*(that) + i, 42] (:55). */
int cwq_greedy_encode(const float* t_loc, const float* t_scale, const float* p_loc,
                      const float* p_scale, const int64_t* block_off, int64_t nb,
                      int64_t total_dims, int64_t max_block_dim, int n_bits_per_step,
                      int n_steps, int32_t seed, float rho, int64_t block_id_base,
                      int32_t* out_idx, float* out_sample, void* workspace,
                      size_t workspace_bytes, const cwq_options* opts, void* stream);

/* Same with every block of dimension d (block g = dims [g*d, (g+1)*d)). */
int cwq_greedy_encode_uniform(const float* t_loc, const float* t_scale, const float* p_loc,
                              const float* p_scale, int64_t nb, int64_t d,
                              int n_bits_per_step, int n_steps, int32_t seed, float rho,
                              int64_t block_id_base, int32_t* out_idx, float* out_sample,
                              void* workspace, size_t workspace_bytes, const cwq_options* opts,
                              void* stream);

/* Decoder (coded_greedy_sampler.py:93-167): sample = sum over steps of the
 * proposal-shard candidate idx[g*n_steps + i] of step i.  O(n_steps * d) per
 * block (only the selected row of the candidate stream is regenerated).
 * An index outside [0, 2^n_bits_per_step) -- a corrupt code -- is no error:
 * every dim of its block decodes to NaN, whichever of the block's steps holds
 * it, no other block is affected, and the call returns CWQ_OK. */
int cwq_greedy_decode(const int32_t* idx, const float* p_loc, const float* p_scale,
                      const int64_t* block_off, int64_t nb, int64_t total_dims,
                      int64_t max_block_dim, int n_bits_per_step, int n_steps, int32_t seed,
                      float rho, int64_t block_id_base, float* out_sample, void* stream);

/* Same with every block of dimension d; out-of-range indices as above.  The
 * arrays need no alignment beyond float's (d % 4 == 0, d <= 256 with all three
 * on 16-byte boundaries takes faster kernels; the results are the same bits). */
int cwq_greedy_decode_uniform(const int32_t* idx, const float* p_loc, const float* p_scale,
                              int64_t nb, int64_t d, int n_bits_per_step, int n_steps,
                              int32_t seed, float rho, int64_t block_id_base, float* out_sample,
                              void* stream);

/* ---- Uniform blocks with a bit budget each ------------------------------- */
/* The budget of each of nb uniform blocks of dimension d from its KL:
 *   S_g     = the float64 sum over the block's dims of the float32 per-dim KL
 *             (the arithmetic of cwq_kl_normal_normal), in dim order;
 *   bits[g] = clamp(ceil(S_g / log(2.0) + extra_bits), min_bits, max_bits) in
 *             float64; a non-finite S_g gives max_bits.
 * 0 <= min_bits <= max_bits <= CWQ_MAX_BITS_PER_STEP.  bits_out: DEVICE int32
 * [nb]; kl_bits_out: DEVICE float32 [nb] receiving S_g / ln 2, or NULL.  The
 * reference closes a group at n_bits ln 2 - 1 nats (coded_greedy_sampler.py:
 * 226), which is extra_bits = 1 / ln 2.  Asynchronous. */
int cwq_block_bits(const float* q_loc, const float* q_scale, const float* p_loc,
                   const float* p_scale, int64_t nb, int64_t d, double extra_bits, int min_bits,
                   int max_bits, int32_t* bits_out, float* kl_bits_out, void* stream);

/* cwq_greedy_encode_uniform with a bit count per block: n_bits is a DEVICE
 * int32 [nb], and block g is coded exactly as cwq_greedy_encode_uniform codes
 * it with n_bits_per_step = n_bits[g] (same seed + block_id_base + g, same
 * opts; the eval events are recorded around all the scoring launches of the
 * call).  The blocks are sorted by bit count on the device (a stable counting
 * sort, so launches repeat from run to run), the 32 bucket sizes are copied
 * to the host, the rows are gathered into sorted order, every non-empty bucket
 * is coded by one launch sequence of the uniform encoder, highest bit count
 * first, all on the caller's stream, and the results are scattered back to
 * block order.  Like the fused grouped calls this one SYNCHRONISES the stream,
 * once (for the bucket sizes), and is NOT graph-capturable; everything after
 * that is only enqueued.  A bit count outside [0, CWQ_MAX_BITS_PER_STEP]
 * returns CWQ_ERR_INVALID, naming how many there are, before anything is
 * coded or written to the outputs.  nb <= 2^31 - 1; nb == 0 returns CWQ_OK
 * without touching the device.
 * Workspace: the sorted copies of the four inputs (16 nb d bytes) and of the
 * sample, the permutation, the seeds and one uniform encoder workspace, which
 * the buckets use one after another.  The size function covers n_steps <= 4 d;
 * a call with more steps needs 4 nb n_steps bytes (rounded up to 256) on top.
 * There is no decoder of its own: the indices, unpacked where they travel as a
 * stream, go to cwq_greedy_decode_uniform with n_bits_per_step =
 * CWQ_MAX_BITS_PER_STEP, which the decoders use only as the indices' range. */
size_t cwq_greedy_encode_uniform_var_workspace_size(int64_t nb, int64_t d);
int cwq_greedy_encode_uniform_var(const float* t_loc, const float* t_scale, const float* p_loc,
                                  const float* p_scale, int64_t nb, int64_t d,
                                  const int32_t* n_bits, int n_steps, int32_t seed, float rho,
                                  int64_t block_id_base, int32_t* out_idx, float* out_sample,
                                  void* workspace, size_t workspace_bytes,
                                  const cwq_options* opts, void* stream);

/* ---- Ragged (CSR) blocks with a bit budget each --------------------------- */
/* cwq_block_bits for nb CSR blocks (block g = dims [block_off[g],
 * block_off[g + 1]), block_off a DEVICE int64 [nb + 1]) of a code of n_steps
 * steps:
 *   bits[g] = clamp(ceil((S_g / log(2.0) + extra_bits) / n_steps), min_bits,
 *             max_bits) in float64,
 * S_g as above (0 for an empty block; a non-finite S_g gives max_bits), and
 * kl_bits_out[g] = (float)(S_g / ln 2).  With n_steps = 1 and equal block
 * lengths this is cwq_block_bits, bit for bit.  total_dims: the length of the
 * four arrays.  Asynchronous. */
int cwq_block_bits_csr(const float* q_loc, const float* q_scale, const float* p_loc,
                       const float* p_scale, const int64_t* block_off, int64_t nb,
                       int64_t total_dims, double extra_bits, int n_steps, int min_bits,
                       int max_bits, int32_t* bits_out, float* kl_bits_out, void* stream);

/* cwq_greedy_encode with a bit count per block: n_bits is a DEVICE int32 [nb],
 * and block g is coded exactly as cwq_greedy_encode codes it with
 * n_bits_per_step = n_bits[g] (same seed + block_id_base + g, same opts; the
 * eval events are recorded once, around all the scoring launches of the call).
 * The blocks are sorted by bit count on the device and gathered, bucket after
 * bucket, into a ragged sorted layout; the 32 bucket sizes travel to the host
 * together with each bucket's dims and its longest block, and every non-empty
 * bucket is coded by one launch sequence of the CSR encoder, highest bit count
 * first, on the caller's stream, sized by the bucket's own longest block (a
 * bucket of short blocks takes the short-block kernels whatever max_block_dim
 * says).  A bucket below 4,096 candidates (bit count < 12) whose blocks
 * average at least 256 dims is scored by the wave-per-row kernel unless
 * opts->prune_mode is 0: every candidate exactly, one wave per row, the same
 * results (the other paths there walk a row with one lane).  A
 * bucket of many short blocks and a few long ones does not meet the rule and
 * runs as before.  The results are scattered back to block order.  Like
 * cwq_greedy_encode_uniform_var this call SYNCHRONISES the stream, once, and
 * is NOT graph-capturable; everything after that is only enqueued.
 * CWQ_ERR_INVALID, before anything is coded or written to the outputs: a bit
 * count outside [0, CWQ_MAX_BITS_PER_STEP] (the message names how many), a
 * decreasing block_off, blocks holding more than total_dims dims or one longer
 * than max_block_dim.  CWQ_ERR_WORKSPACE: fewer bytes than
 * cwq_greedy_encode_var_workspace_size(nb, total_dims, max_block_dim, n_steps)
 * (0 for negative or overflowing arguments): five sorted arrays of total_dims
 * floats, 40 B per block of layout, the staged indices and one
 * cwq_greedy_encode workspace for the whole call, which the buckets use one
 * after another.  nb <= 2^31 - 1; nb == 0 returns CWQ_OK without touching the
 * device.  There is no decoder of its own: the indices, unpacked where they
 * travel as a stream, go to cwq_greedy_decode with n_bits_per_step =
 * CWQ_MAX_BITS_PER_STEP; the CSR decoder reads the count only as the bound
 * 2^n_bits an index must stay below. */
size_t cwq_greedy_encode_var_workspace_size(int64_t nb, int64_t total_dims, int64_t max_block_dim,
                                            int n_steps);
int cwq_greedy_encode_var(const float* t_loc, const float* t_scale, const float* p_loc,
                          const float* p_scale, const int64_t* block_off, int64_t nb,
                          int64_t total_dims, int64_t max_block_dim, const int32_t* n_bits,
                          int n_steps, int32_t seed, float rho, int64_t block_id_base,
                          int32_t* out_idx, float* out_sample, void* workspace,
                          size_t workspace_bytes, const cwq_options* opts, void* stream);

/* The indices of such a call as a packed stream, on the device.  Field (g, s),
 * g < nb, s < n_steps, is idx[g n_steps + s] in n_bits[g] bits, its bit 0
 * first; the fields follow each other in block order, then step order, and the
 * stream's bit i lies in byte i / 8 at bit 7 - i % 8, the last byte padded
 * with zeros: the bytes binary_io.py:76-78 writes for the joined to_bit_string
 * (:41-53) fields.  Blocks of 0 bits take no room.  idx, n_bits: DEVICE int32.
 * pack writes the first min(out_cap, ceil(total / 8)) bytes of the stream to
 * DEVICE out_bytes, never more, and the total bit count to DEVICE
 * total_bits_dev (-1 when some n_bits[g] lies outside [0, 30]; such a block
 * takes no room): a caller compares 8 out_cap with it.  unpack reads field
 * (g, s) back into idx_out[g n_steps + s]; bits past n_bytes read as 0
 * (cwq_bitcode_to_indices' rule for short codes).  Both are asynchronous and
 * stream-ordered and allocate nothing; workspace: the blocks' bit offsets.
 * nb == 0 returns CWQ_OK and writes nothing, total_bits_dev included. */
size_t cwq_pack_indices_var_workspace_size(int64_t nb);
int cwq_pack_indices_var(const int32_t* idx, const int32_t* n_bits, int64_t nb, int n_steps,
                         uint8_t* out_bytes, int64_t out_cap, int64_t* total_bits_dev,
                         void* workspace, size_t workspace_bytes, void* stream);
int cwq_unpack_indices_var(const uint8_t* bytes, int64_t n_bytes, const int32_t* n_bits,
                           int64_t nb, int n_steps, int32_t* idx_out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* coded_greedy_sampler.py:198-199: t_loc = (q_loc - p_loc) / p_scale,
 * t_scale = q_scale / p_scale (float32). */
int cwq_standardise(const float* q_loc, const float* q_scale, const float* p_loc,
                    const float* p_scale, int64_t n, float* t_loc, float* t_scale, void* stream);

/* coded_greedy_sampler.py:201: per-dim KL(q || p) of two diagonal Gaussians
 * (TFP <= 0.7 formula, float32). */
int cwq_kl_normal_normal(const float* q_loc, const float* q_scale, const float* p_loc,
                         const float* p_scale, int64_t n, float* out, void* stream);

/* coded_greedy_sampler.py:292: out = p_scale * sample + p_loc (float32, two
 * roundings).  out may alias sample. */
int cwq_destandardise(const float* sample, const float* p_loc, const float* p_scale, int64_t n,
                      float* out, void* stream);

/* HOST function (coded_greedy_sampler.py:207-252).  kl: HOST float32 [D].
 * size_threshold: the smallest group size s for which the reference's
 * `np.log(s + 1) / np.log(2) >= max_group_size_bits` holds.  n_nats:
 * n_bits_per_group * np.log(2) - 1 (float64).  Writes the reference's
 * group_start_indices (including the leading 0, the forced boundary at D-1 and
 * the trailing D) to starts[0..n) and returns n, or a negative error code if
 * cap is too small. */
int64_t cwq_group_starts(const float* kl, int64_t D, int64_t size_threshold, double n_nats,
                         int64_t* starts, int64_t cap);

/* code_grouped_greedy_sample (coded_greedy_sampler.py:170-296) in one call:
 * device standardisation and KL (:193-210), the host partition (:207-252, as
 * cwq_group_starts with size_threshold / n_nats), one greedy coder per group
 * with seed + g (:273-284), destandardisation (:292) and the LSB-first
 * bitcode (:81-87, :288).  q_* / p_*: DEVICE float32 [D] (target, proposal).
 * Outputs are HOST memory: sample_host [D] float32, bits_host ('0'/'1' chars,
 * groups x n_steps x n_bits_per_step of them), starts_host (the reference's
 * group_start_indices incl. the trailing D; starts_cap >= D + 2) and, if
 * non-NULL, kl_sum_out (sum of the per-dim KL in nats, for the reference's
 * log line).  Returns the number of groups, or a negative error code.
 * Synchronises the stream twice (after the KL, at the end). */
size_t cwq_code_grouped_greedy_workspace_size(int64_t D, int n_steps);
int64_t cwq_code_grouped_greedy(const float* q_loc, const float* q_scale, const float* p_loc,
                                const float* p_scale, int64_t D, int n_steps,
                                int n_bits_per_step, int32_t seed, float rho,
                                int64_t size_threshold, double n_nats, float* sample_host,
                                char* bits_host, int64_t bits_cap, int64_t* starts_host,
                                int64_t starts_cap, double* kl_sum_out, void* workspace,
                                size_t workspace_bytes, const cwq_options* opts, void* stream);

/* cwq_code_grouped_greedy in two halves, so the caller can work while the
 * device codes (the Python wrapper builds the reference's group_start_indices
 * list meanwhile).  _begin: the same inputs; waits for the partition (on the
 * device where it applies: its 128-byte result; else the KL copy and the host
 * loop), writes starts_host[0..G] and returns G (or a negative error code), with the
 * encode, the destandardisation and the copies of the G * n_steps indices to
 * idx_host (idx_cap >= G * n_steps; D + 1 groups at most) and of the sample to
 * sample_host still in flight on the stream: both must stay valid until _end,
 * and page-locked host memory keeps the copies asynchronous.  starts_host is
 * also the source of an asynchronous copy of the group offsets to the device:
 * it must stay valid and unchanged until _end too.
 * opts->eval_ms_out must be NULL (the caller's eval events work).  _end:
 * synchronises the stream and writes the bitcode of those indices; returns
 * the number of chars (G * n_steps * n_bits_per_step) or a negative code. */
int64_t cwq_code_grouped_greedy_begin(const float* q_loc, const float* q_scale,
                                      const float* p_loc, const float* p_scale, int64_t D,
                                      int n_steps, int n_bits_per_step, int32_t seed, float rho,
                                      int64_t size_threshold, double n_nats, float* sample_host,
                                      int32_t* idx_host, int64_t idx_cap, int64_t* starts_host,
                                      int64_t starts_cap, double* kl_sum_out, void* workspace,
                                      size_t workspace_bytes, const cwq_options* opts,
                                      void* stream);
int64_t cwq_code_grouped_greedy_end(const int32_t* idx_host, int64_t G, int n_steps,
                                    int n_bits_per_step, char* bits_host, int64_t bits_cap,
                                    void* stream);

/* A batch of independent code_grouped_greedy_sample calls (coded_greedy_sampler.py:170-296
 * once per item: the images of a dataset, or the ladder levels of several
 * images) in one call.  Item i is dims [item_off[i], item_off[i+1]) of the
 * concatenated DEVICE q_* / p_* (item_off: HOST int64 [n_items + 1], item_off[0]
 * == 0) and is coded exactly as cwq_code_grouped_greedy on that slice with seed
 * seeds[i] (HOST int32 [n_items]): its own partition (:207-252), its groups
 * numbered from 0 and coded with seeds[i] + g (:273-284).  One standardisation
 * and KL launch serve all items, and one device partition (cwq_partition.hip)
 * finds every item's groups (when the device scheme does not cover an input,
 * the host loop partitions chunk by chunk instead, with identical results).
 * The items are then pipelined in chunks of consecutive items
 * (CWQ_BATCH_CHUNKS, default 6; the first a quarter share, the last a half): one
 * encode launch sequence per chunk with per-block seeds, chunk c's results
 * copied to the host while chunk c + 1 codes, and each item's bitcode written
 * as soon as its chunk's indices arrive, on a pool of host threads (up to
 * CWQ_HOST_THREADS - 1, default min(8, CPUs) - 1) that the library creates on
 * the first batch call and keeps for the life of the process.
 * HOST outputs: sample_host [D_total]; item i's bitcode at
 * bits_host[bits_off[i], bits_off[i+1]) (bits_off: HOST int64 [n_items + 1],
 * written); item i's group_start_indices (local, incl. its trailing D_i):
 * n_starts[i] entries (HOST int64 [n_items], written) at starts_host +
 * item_off[i] + 2 i (starts_cap >= D_total + 2 n_items).  host_workspace:
 * HOST staging of host_workspace_bytes >=
 * cwq_code_grouped_greedy_batch_host_workspace_size (per-dim KL, group
 * offsets, seeds, indices), page-locked for asynchronous copies (hipHostMalloc,
 * or torch's pinned memory); NULL = library-owned pageable staging (slower
 * copies).  sample_host is best page-locked as well.  Returns the total number
 * of groups, or a negative error code.  Returns only after all of its device
 * work has finished (also on error): it SYNCHRONISES the stream and is NOT
 * graph-capturable. */
size_t cwq_code_grouped_greedy_batch_workspace_size(int64_t D_total, int64_t n_items,
                                                    int n_steps);
size_t cwq_code_grouped_greedy_batch_host_workspace_size(int64_t D_total, int64_t n_items,
                                                         int n_steps);
int64_t cwq_code_grouped_greedy_batch(
    int64_t n_items, const int64_t* item_off, const float* q_loc, const float* q_scale,
    const float* p_loc, const float* p_scale, int n_steps, int n_bits_per_step,
    const int32_t* seeds, float rho, int64_t size_threshold, double n_nats, float* sample_host,
    char* bits_host, int64_t bits_cap, int64_t* bits_off, int64_t* starts_host,
    int64_t starts_cap, int64_t* n_starts, void* workspace, size_t workspace_bytes,
    void* host_workspace, size_t host_workspace_bytes, const cwq_options* opts, void* stream);

/* ---- Importance sampler (code/coded_importance_sampler.py) ------------- */
/* Workspace bytes for cwq_importance_encode. */
size_t cwq_importance_workspace_size(int64_t nb, int64_t total_dims);

/* code_importance_sample (:29-79) for nb CSR groups at once.  Group g draws
 * n_samples[g] (device int64) candidates x = p_loc + p_scale*z from the
 * stateless stream with seed (seed + block_id_base + g) -- the group seed
 * itself (:55, :243) -- scores sum_j log q(x_j) - log p(x_j) (:60) and writes
 * the 0-based argmax out_index[g] (device int64; the reference codes
 * index + 1 with Elias-delta) and that candidate into out_sample. */
int cwq_importance_encode(const float* t_loc, const float* t_scale, const float* p_loc,
                          const float* p_scale, const int64_t* block_off,
                          const int64_t* n_samples, int64_t nb, int64_t total_dims, int32_t seed,
                          int64_t block_id_base, int64_t* out_index, float* out_sample,
                          void* workspace, size_t workspace_bytes, const cwq_options* opts,
                          void* stream);

/* decode_importance_sample (:82-109): the last of index+1 samples, i.e. row
 * `index` of group g's stream. */
int cwq_importance_decode(const int64_t* index, const float* p_loc, const float* p_scale,
                          const int64_t* block_off, int64_t nb, int64_t total_dims, int32_t seed,
                          int64_t block_id_base, float* out_sample, void* stream);

/* HOST (:178-203): the importance coder's partition; as cwq_group_starts but
 * with the reference's strict comparisons (`group_bits > max bits`,
 * `kl_sum > n_nats`).  size_threshold: the smallest s with
 * np.log(s + 1) / np.log(2) > max_group_size_bits. */
int64_t cwq_importance_group_starts(const float* kl, int64_t D, int64_t size_threshold,
                                    double n_nats, int64_t* starts, int64_t cap);

/* HOST (:48-51): n_samples[g] = int32(ceil(expf(sum of group g's float32 KLs in
 * Eigen inner-dim order))), for groups [starts[g], starts[g+1]) of HOST kl. */
int cwq_importance_plan(const float* kl, const int64_t* starts, int64_t ng, int64_t* n_samples);

/* coded_importance_sampler.py:112-274 code_grouped_importance_sample in one
 * call (the counterpart of cwq_code_grouped_greedy): device standardisation,
 * KL and outlier masking (kl / ln 2 > dim_kl_bit_limit, float32), the seeded
 * outlier target draw q_loc + q_scale z, z from [seed - 1, 42],
 * the host partition (size_threshold and n_nats as cwq_importance_group_starts)
 * and sample-count plan, one encode launch, device destandardisation.
 * Device inputs; HOST outputs: sample_host [D] (outlier dims hold the target
 * draw, :267), index_host [G] (argmax index, the reference codes index + 1),
 * starts_host (group starts incl. the trailing D; starts_cap >= D + 2), the
 * outlier dims and their unquantised draws (outlier_*_host, capacity D,
 * *n_outliers of them), and optionally (kl_sum_out) the total standardised KL
 * in nats for the reference's log line.  Returns G or a negative error code.
 * Blocks the host until the results are on it: SYNCHRONISES the stream, NOT
 * graph-capturable. */
size_t cwq_code_grouped_importance_workspace_size(int64_t D);
int64_t cwq_code_grouped_importance(const float* q_loc, const float* q_scale,
                                    const float* p_loc, const float* p_scale, int64_t D,
                                    int32_t seed, float dim_kl_bit_limit, int64_t size_threshold,
                                    double n_nats, float* sample_host, int64_t* index_host,
                                    int64_t* starts_host, int64_t starts_cap,
                                    int64_t* outlier_idx_host, float* outlier_val_host,
                                    int64_t* n_outliers, double* kl_sum_out, void* workspace,
                                    size_t workspace_bytes, const cwq_options* opts,
                                    void* stream);

/* A batch of independent code_grouped_importance_sample calls
 * (coded_importance_sampler.py:112-274 once per item: the level-2 latents of
 * a dataset's images, pln.py:350-359) in one call.  Item i is dims
 * [item_off[i], item_off[i+1]) of the concatenated DEVICE q_* / p_* (item_off:
 * HOST int64 [n_items + 1], item_off[0] == 0) and is coded exactly as
 * cwq_code_grouped_importance on that slice with seed seeds[i] (HOST int32
 * [n_items]): its own outliers and outlier draw ([seeds[i] - 1, 42] over its
 * own dims), its own partition and plan, its groups numbered from 0 and coded
 * with seeds[i] + g.  One preparation launch and one encode launch serve every
 * item.  HOST outputs, item i's at the offsets shown:
 *   sample_host [D_total] (item i's dims in place);
 *   index_host + item_off[i] + i: its G_i argmax indices (capacity D_total +
 *     n_items);
 *   starts_host + item_off[i] + 2 i: its group starts incl. its trailing D_i,
 *     n_starts[i] (= G_i + 1) of them (starts_cap >= D_total + 2 n_items);
 *   outlier_idx_host / outlier_val_host + item_off[i]: its n_outliers[i]
 *     outlier dims (local indices) and their unquantised draws;
 *   kl_sum_out [n_items] (optional): each item's standardised KL in nats.
 * opts->eval_ms_out receives the encode launches' milliseconds.  Returns the
 * total number of groups, or a negative error code.  Blocks the host until
 * the results are on it: SYNCHRONISES the stream, NOT graph-capturable. */
size_t cwq_code_grouped_importance_batch_workspace_size(int64_t D_total, int64_t n_items);
int64_t cwq_code_grouped_importance_batch(
    int64_t n_items, const int64_t* item_off, const float* q_loc, const float* q_scale,
    const float* p_loc, const float* p_scale, const int32_t* seeds, float dim_kl_bit_limit,
    int64_t size_threshold, double n_nats, float* sample_host, int64_t* index_host,
    int64_t* starts_host, int64_t starts_cap, int64_t* n_starts, int64_t* outlier_idx_host,
    float* outlier_val_host, int64_t* n_outliers, double* kl_sum_out, void* workspace,
    size_t workspace_bytes, const cwq_options* opts, void* stream);

/* ---- Batched grouped decoders ------------------------------------------- */
/* A batch of independent decode_grouped_greedy_sample calls
 * (coded_greedy_sampler.py:299-364 once per item) in one call.  Item i is dims
 * [item_off[i], item_off[i+1]) of the concatenated DEVICE p_loc / p_scale
 * (item_off: HOST int64 [n_items + 1], item_off[0] == 0).  HOST inputs: its
 * code, the '0'/'1' chars bits_host[bits_off[i], bits_off[i+1]), and its
 * group_start_indices (local to the item, as its encoder returned them, with
 * or without the trailing D_i), starts_host[starts_off[i], starts_off[i+1]);
 * seeds: HOST int32 [n_items].  The item is decoded exactly as the reference
 * decodes it alone: D_i is appended to its starts (:323), its groups are
 * numbered from 0 and seeded seeds[i] + g (int32 wrap), group g is decoded
 * while its bit slice is non-empty (:345-347), and chars past the end of the
 * code read as '0' (cwq_bitcode_to_indices' rule).  The groups so decoded must
 * cover its D_i dims: otherwise CWQ_ERR_INVALID, with the item named, before
 * anything is launched.
 * The call parses the codes and plans the global group offsets, slot prefix
 * and seeds into host_workspace (on the library's host threads, item by item),
 * copies that plan to the device once, decodes every group of every item in
 * one launch (standard proposal, then sample * p_scale + p_loc, :362) and, if
 * sample_host is given, copies the D_total samples to it and synchronises the
 * stream once.  sample_dev (DEVICE [D_total]) receives the samples on the
 * device; either may be NULL, not both.  With sample_host == NULL the call
 * only enqueues work: host_workspace is the source of an asynchronous copy and
 * must stay valid and unchanged until the stream has reached this point, as
 * starts_host of cwq_code_grouped_greedy_begin must until _end.  Either way
 * the launch follows a plan made on the host from the codes: NOT
 * graph-capturable.
 * G_total of the size functions: the total number of starts entries
 * (starts_off[n_items] - starts_off[0]).  host_workspace is best page-locked.
 * opts: only eval_start_event / eval_stop_event are read (recorded around the
 * launch).  Returns the total number of groups decoded, or a negative code. */
size_t cwq_decode_grouped_greedy_batch_workspace_size(int64_t D_total, int64_t G_total,
                                                      int n_steps);
size_t cwq_decode_grouped_greedy_batch_host_workspace_size(int64_t D_total, int64_t G_total,
                                                           int n_steps);
int64_t cwq_decode_grouped_greedy_batch(
    int64_t n_items, const int64_t* item_off, const float* p_loc, const float* p_scale,
    const char* bits_host, const int64_t* bits_off, const int64_t* starts_host,
    const int64_t* starts_off, int n_steps, int n_bits_per_step, const int32_t* seeds, float rho,
    float* sample_host, float* sample_dev, void* workspace, size_t workspace_bytes,
    void* host_workspace, size_t host_workspace_bytes, const cwq_options* opts, void* stream);

/* The same for decode_grouped_importance_sample (coded_importance_sampler.py:
 * 277-363) up to the rescale (:347); the outlier overwrite (:351-361) stays
 * with the caller.  HOST inputs: item i's 0-based indices (the decoded
 * Elias-delta values - 1), index_host[index_off[i] ...], one per group, and its
 * group_start_indices WITHOUT the trailing D_i (the reference appends it,
 * :294), starts_host[starts_off[i], starts_off[i+1]).  Group g of item i is row
 * index[g] of the stream seeded seeds[i] + g.  One plan copy, one launch, one
 * copy out; workspace, staging, sample_host / sample_dev, opts and the return
 * value as above (G_total: the total number of starts entries); NOT
 * graph-capturable, as above. */
size_t cwq_decode_grouped_importance_batch_workspace_size(int64_t D_total, int64_t G_total);
size_t cwq_decode_grouped_importance_batch_host_workspace_size(int64_t D_total, int64_t G_total);
int64_t cwq_decode_grouped_importance_batch(
    int64_t n_items, const int64_t* item_off, const float* p_loc, const float* p_scale,
    const int64_t* index_host, const int64_t* index_off, const int64_t* starts_host,
    const int64_t* starts_off, const int32_t* seeds, float* sample_host, float* sample_dev,
    void* workspace, size_t workspace_bytes, void* host_workspace, size_t host_workspace_bytes,
    const cwq_options* opts, void* stream);

/* ---- Arithmetic coder (code/coding.pyx:27-310), HOST functions ---------- */
/* ArithmeticCoder(P, precision).encode(message): writes the code as '0'/'1'
 * chars to out_bits (if non-null, at most cap) and returns the number of bits
 * (or a negative error).  counts: P[K] (non-negative, sum > 0); message
 * symbols in [0, K) with non-zero counts (CWQ_ERR_INVALID otherwise: the
 * reference loops forever on a zero-count symbol) and, as the reference's
 * callers do, ending with the EOF symbol 0.  precision in [3, 62] (the
 * reference uses 32). */
int64_t cwq_ac_encode(const int64_t* counts, int64_t K, int precision, const int64_t* message,
                      int64_t n, char* out_bits, int64_t cap);

/* .decode / .decode_fast (:129-310): decodes until the EOF symbol 0 and
 * returns the number of symbols written to out_msg (EOF included),
 * CWQ_ERR_CAPACITY if cap is too small, or CWQ_ERR_INVALID for a corrupt code
 * (where the reference would loop forever). */
int64_t cwq_ac_decode(const int64_t* counts, int64_t K, int precision, const char* bits,
                      int64_t nbits, int64_t* out_msg, int64_t cap);

/* Elias-delta codes of the importance sampler's index + 1 values
 * (code/binary_io.py:7-39), concatenated.  Host memory.  encode writes the
 * '0'/'1' chars of x[0..n) to out (NULL: only count) and returns their
 * number; values must lie in [1, 2^30) (CWQ_ERR_INVALID otherwise, where the
 * reference's float64 log formulas may differ from the bit lengths).  decode
 * parses `count` codes from bits[0..nbits) into out and returns the chars
 * consumed (coded_importance_sampler.py:325-336). */
int64_t cwq_elias_delta_encode(const int64_t* x, int64_t n, char* out, int64_t cap);
int64_t cwq_elias_delta_decode(const char* bits, int64_t nbits, int64_t count, int64_t* out);

/* The greedy coder's bit parse (code/coded_greedy_sampler.py:107-126 and
 * :330-342, binary_io.py:55-67 from_bit_string of each num_bits substring):
 * count indices of num_bits LSB-first chars each from bits[0..nbits) into
 * out.  Chars past nbits read as '0' (the short substring tf.strings.substr
 * yields at the end of the string); any char other than '1' reads as 0.  Host
 * memory.  Returns count, or CWQ_ERR_INVALID (num_bits outside
 * [0, CWQ_MAX_BITS_PER_STEP], negative sizes, null pointers). */
int64_t cwq_bitcode_to_indices(const char* bits, int64_t nbits, int num_bits, int64_t count,
                               int32_t* out);

/* Diagnostics (used by the parity tests): evaluate the device restatement of
 * the Box-Muller transcendentals for the 23-bit mantissas m0 .. m0+count-1:
 *   radius[i] = sqrtf(-2 logf(max(m*2^-23, 1e-7f)))    (BoxMullerFloat u2)
 *   sin[i], cos[i] = sincosf((float)(2*pi * m*2^-23))   (BoxMullerFloat v1)
 * and logf(x[i]) for arbitrary floats (the per-dimension normaliser's log). */
int cwq_selftest_bm_tables(uint32_t m0, int64_t count, float* radius, float* sin_out,
                           float* cos_out, void* stream);
int cwq_selftest_logf(const float* x, int64_t n, float* out, void* stream);
/* The screening passes' approximations of the same three tables (hardware
 * v_log/v_sqrt/v_sin/v_cos); radius[i] holds r~ / sqrt(2 ln 2), the form the
 * kernels carry.  The tests bound their deviation from the exact tables by the
 * constants the screening bounds are built on. */
int cwq_selftest_screen_tables(uint32_t m0, int64_t count, float* radius, float* sin_out,
                               float* cos_out, void* stream);
/* out[i] = the device's fast correctly-rounded quotient a[i] / b[i]
 * (Markstein sequence with y = RN(1/b); only valid in the ranges documented in
 * DESIGN.md -- the test feeds it exactly those). */
int cwq_selftest_div(const float* a, const float* b, int64_t n, float* out, void* stream);
/* out[w] = max(x[64 w .. 64 w + 63]): the wave-wide DPP max the pruned encoder
 * shares its threshold with. */
int cwq_selftest_wave_max(const float* x, int64_t n_waves, float* out, void* stream);
/* cwq_greedy_encode (same arguments without opts, same workspace from
 * cwq_greedy_encode_workspace_size, same validation and results) with every
 * block scored by the wave-per-row kernel that cwq_greedy_encode_var uses for
 * buckets of long blocks at few candidates, whatever the blocks' length or
 * number: the tests reach short, odd and empty rows on that kernel this way. */
int cwq_selftest_encode_rows_wave(const float* t_loc, const float* t_scale, const float* p_loc,
                                  const float* p_scale, const int64_t* block_off, int64_t nb,
                                  int64_t total_dims, int64_t max_block_dim, int n_bits_per_step,
                                  int n_steps, int32_t seed, float rho, int64_t block_id_base,
                                  int32_t* out_idx, float* out_sample, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* cwq_greedy_encode_uniform (same arguments, validation, workspace and
 * results) with the pruned kernel's tau guess set by guess_mode instead of by
 * opts->prune_mode: 0 = off (the threshold of a tile starts at -inf or at the
 * block's best so far), 1 = on (it starts at the lower bound of a row at the
 * level that CWQ_TAU_GUESS_M of the tile's candidates are expected to fall
 * below; the default where prune_mode is 2), 2 = every screened tile's guess
 * replaced by FLT_MAX, so that each is run again without it.  The guess only
 * has an effect where the screening pass runs (prune_mode 2). */
int cwq_selftest_encode_uniform_tau_guess(const float* t_loc, const float* t_scale,
                                          const float* p_loc, const float* p_scale, int64_t nb,
                                          int64_t d, int n_bits_per_step, int n_steps,
                                          int32_t seed, float rho, int64_t block_id_base,
                                          int32_t* out_idx, float* out_sample, void* workspace,
                                          size_t workspace_bytes, const cwq_options* opts,
                                          void* stream, int guess_mode);
/* The bytes of a cwq_greedy_encode_uniform workspace with which the call may
 * defer the pruned kernel's exact work: the layout of
 * cwq_greedy_encode_uniform_workspace_size with, for blocks of d % 8 == 0,
 * 8 <= d <= 64 dims, per-block survivor slots, counts and a list of deferred
 * blocks behind it.  With workspace_bytes of at least this, a call whose
 * blocks run one tile each scores in three launches: the screening-only
 * kernel, the listed rows' exact values, and the full kernel over the blocks
 * the first launch could not settle.  With fewer bytes (at least
 * cwq_greedy_encode_uniform_workspace_size) it runs as before.  Same results
 * either way.  Equal to cwq_greedy_encode_uniform_workspace_size for every
 * other d; 0 for invalid arguments. */
size_t cwq_greedy_encode_uniform_defer_bytes(int64_t nb, int64_t d);
/* cwq_greedy_encode_uniform (same arguments, validation and results; the
 * workspace of cwq_greedy_encode_uniform_defer_bytes) with every block one
 * tile and the deferral set by defer_mode: 0 = off (the single launch), 1 = on
 * at any size, 2 = on with every tile deferred, 3 = on with no slot per block
 * (Q = 0: every tile with a row to score is deferred). */
int cwq_selftest_encode_uniform_defer(const float* t_loc, const float* t_scale,
                                      const float* p_loc, const float* p_scale, int64_t nb,
                                      int64_t d, int n_bits_per_step, int n_steps, int32_t seed,
                                      float rho, int64_t block_id_base, int32_t* out_idx,
                                      float* out_sample, void* workspace, size_t workspace_bytes,
                                      const cwq_options* opts, void* stream, int defer_mode);

/* ---- Beam search over the greedy coder's steps (csrc/cwq_beam.hip) --------
 * cwq_greedy_encode keeps the one best partial sum after each step; this
 * encoder keeps the `beam` best.  State after step i: L_i live beams (L_0 = 1,
 * the all-zero sum; L_{i+1} = min(beam, L_i 2^b)), each a float32 running sum
 * and its path of i row indices.  Step i scores every live beam k against the
 * rows r < 2^b of the step's candidate stream (the same rows for every beam,
 * the stream cwq_greedy_encode draws): candidate c = k 2^b + r has the value
 * v = sum_j log N(sum_k[j] + row_r[j]; t_loc[j], t_scale[j]) (float32, the
 * greedy coder's arithmetic and summation order) and the key (v, c), where a
 * NaN or a value <= -FLT_MAX counts as -FLT_MAX, -0 as +0, and the lower c
 * wins a tie.  The L_{i+1} candidates with the largest keys, in decreasing
 * order, become the new beams: sum_k + row_r, path_k followed by r.  After
 * the last step beam 0 is the result.  The selection is a function of the
 * candidate set alone; results never depend on the launch geometry.
 *   beam       1 <= beam <= CWQ_MAX_BEAM, any value; beam * 2^n_bits_per_step
 *              <= 2^31.  With beam = 1 the outputs are cwq_greedy_encode's.
 *   block_off  device [nb + 1], or NULL for uniform blocks of max_block_dim
 *              dims (total_dims = nb * max_block_dim)
 *   out_idx    [nb * n_steps] int32: beam 0's row index of every step; any
 *              greedy decoder turns them back into out_sample (the bit string
 *              and every file format are those of the greedy coder)
 *   out_sample [total_dims] f32: beam 0's sum
 *   out_value  [nb] f32 or NULL: beam 0's value v of the last step as its key
 *              holds it (an empty block: indices 0, value +0)
 *   opts       prune_mode is accepted and ignored (every row is scored
 *              exactly); the eval events bracket the scoring launches.
 * Blocks whose longest has at most 64 dims are scored with a lane per
 * candidate row, longer ones with a wave per row; a row is drawn once and
 * scored against all beams.  Asynchronous on `stream`, no host
 * synchronisation, no other stream: capturable into a graph.
 * Workspace bytes (each array rounded up to 256): 3 * 4 * total_dims (shard
 * constants) + 2 * beam * 4 * total_dims (the beams' sums, ping-pong) +
 * 8 * beam * nb * T(nb) (per-tile key lists, T(nb) = 4 * the power of two at
 * or above ceil(2048 / nb)) + 8 * beam * nb * n_steps (the selected keys).
 * It is large: a call whose workspace does not fit is the caller's to split. */
#define CWQ_MAX_BEAM 16
size_t cwq_beam_encode_workspace_size(int64_t nb, int64_t total_dims, int64_t max_block_dim,
                                      int n_steps, int beam);
int cwq_beam_encode(const float* t_loc, const float* t_scale, const float* p_loc,
                    const float* p_scale, const int64_t* block_off, int64_t nb,
                    int64_t total_dims, int64_t max_block_dim, int n_bits_per_step, int n_steps,
                    int beam, int32_t seed, float rho, int64_t block_id_base, int32_t* out_idx,
                    float* out_sample, float* out_value, void* workspace, size_t workspace_bytes,
                    const cwq_options* opts, void* stream);
/* The same call on the scoring kernel `path` names instead of the one the
 * block lengths select: 0 lane per row (max_block_dim <= 64 only), 1 wave per
 * row; 2 and 3: the same two with tiles a quarter of the size.  The tests hold
 * all four to the same bits. */
int cwq_selftest_beam_encode(const float* t_loc, const float* t_scale, const float* p_loc,
                             const float* p_scale, const int64_t* block_off, int64_t nb,
                             int64_t total_dims, int64_t max_block_dim, int n_bits_per_step,
                             int n_steps, int beam, int32_t seed, float rho,
                             int64_t block_id_base, int32_t* out_idx, float* out_sample,
                             float* out_value, void* workspace, size_t workspace_bytes,
                             const cwq_options* opts, void* stream, int path);

/* ---- Beam search under per-block bit budgets (csrc/cwq_beam.hip) -----------
 * cwq_beam_encode with a bit count per block.  Block g is coded exactly as
 * cwq_beam_encode codes it in a call of its own with n_bits_per_step = b_g and
 * block seed seed + block_id_base + g (int32 wrap), where
 *   b_g = clamp(n_bits[g], 0, max_bits),
 *   L_0 = 1, L_{i+1} = min(beam, L_i 2^b_g), i.e. L_i = min(beam, 2^(b_g i)),
 *   candidate c = k 2^b_g + r for live beam k and row r < 2^b_g;
 * the keys, the tie rule, the handling of NaN, values <= -FLT_MAX and -0,
 * out_idx, out_sample and out_value are those of cwq_beam_encode.  A block at 0
 * bits has one row per step: indices 0, one beam for ever.  An empty block
 * gives indices 0 and value +0.  Row g of out_idx lies in [0, 2^b_g): it is the
 * table cwq_greedy_decode_var, cwq_pack_indices_var and cwq_greedy_backfit_var
 * read; there is no new decoder and no new format.
 *   n_bits     device [nb] int32, the blocks' bit counts
 *   max_bits   the bound on them the caller vouches for: 0 <= max_bits <=
 *              CWQ_MAX_BITS_PER_STEP and beam * 2^max_bits <= 2^31 (these take
 *              the place of cwq_beam_encode's checks on n_bits_per_step)
 * The counts live on the device and the call does not wait for the device, so
 * it cannot check them: a count outside [0, max_bits] is READ AS CLAMPED to
 * that range.  This is deterministic and memory-safe (every loop bound and
 * every index derived from a count uses the clamped value), but such a block's
 * indices then need the clamped count to decode.  Check the counts first where
 * they are not known to be in range; the Python binding does.
 * Every other argument is cwq_beam_encode's.  The workspace is that of
 * cwq_beam_encode_workspace_size(nb, total_dims, max_block_dim, n_steps,
 * beam): the size does not depend on the bit counts, the layout is the same,
 * and there is no size function of its own.  One launch sequence serves every
 * budget (3 launches per step, one before and one after, whatever the number
 * of distinct budgets): one stream, no fork, no host synchronisation, no
 * allocation; capturable into a graph.  nb == 0 returns CWQ_OK without
 * touching the device.  prune_mode is accepted and ignored; the eval events
 * bracket the scoring launches. */
int cwq_beam_encode_var(const float* t_loc, const float* t_scale, const float* p_loc,
                        const float* p_scale, const int64_t* block_off, int64_t nb,
                        int64_t total_dims, int64_t max_block_dim, const int32_t* n_bits,
                        int max_bits, int n_steps, int beam, int32_t seed, float rho,
                        int64_t block_id_base, int32_t* out_idx, float* out_sample,
                        float* out_value, void* workspace, size_t workspace_bytes,
                        const cwq_options* opts, void* stream);
/* The same call with the kernel and tiling forced: paths 0-3 as in
 * cwq_selftest_beam_encode. */
int cwq_selftest_beam_encode_var(const float* t_loc, const float* t_scale, const float* p_loc,
                                 const float* p_scale, const int64_t* block_off, int64_t nb,
                                 int64_t total_dims, int64_t max_block_dim, const int32_t* n_bits,
                                 int max_bits, int n_steps, int beam, int32_t seed, float rho,
                                 int64_t block_id_base, int32_t* out_idx, float* out_sample,
                                 float* out_value, void* workspace, size_t workspace_bytes,
                                 const cwq_options* opts, void* stream, int path);

/* ---- Backfitting for the greedy coder (csrc/cwq_backfit.hip) ---------------
 * Coordinate ascent over the steps of a finished code: it refines any index
 * table (cwq_greedy_encode's, cwq_beam_encode's, the caller's own) and returns
 * a table of the same form, so every decoder, the bit string and every file
 * format stay as they are.
 *
 * Setup, per block g: the greedy coder's.  Block seed s_g = seed +
 * block_id_base + g (int32 wrap), step i's stream seed [1000 s_g + i, 42], the
 * shard constants and normalisers, N = 2^n_bits_per_step rows per step;
 * row(i, r) is row r of step i's stream; dec(idx) is the decoder's float32
 * sum in step order, ((+0 + row(0, idx_0)) + row(1, idx_1)) + ...; val(x) is
 * the value a key holds for x: sum_j log N(x[j]; t_loc[j], t_scale[j]) in
 * float32 (the greedy coder's arithmetic and summation order), where a NaN or
 * a value <= -FLT_MAX reads as -FLT_MAX and -0 as +0.
 *
 * State: idx[n_steps], initialised from the caller's table, v = val(dec(idx)).
 * One sweep visits s = 0 .. n_steps - 1 in order:
 *   1. base_s = the decoder-order sum with step s skipped;
 *   2. r* = the row with the largest key (val(base_s + row(s, r)), r) over
 *      r < N; among equal values the lowest r wins;
 *   3. r* == idx[s]: nothing changes;
 *   4. otherwise idx' = idx with idx'[s] = r*, v' = val(dec(idx')), and the
 *      replacement is accepted (idx = idx', v = v') iff v' > v, compared as
 *      floats.  base_s + row and the decoder's order differ by rounding unless
 *      s is the last step, hence the test: the output is exactly what the
 *      decoder rebuilds, and no block ever ends below the code it came with.
 * After `sweeps` sweeps: idx, out_sample = dec(idx), out_value = v and
 * out_accepted[g] = the number of accepts of block g.  sweeps = 0 returns the
 * table with its decoded sample and value.  A code of one step is returned as
 * given for any `sweeps` (there is no other step to fit it to), as is an empty
 * block and every block at n_bits_per_step = 0.
 *   sweeps        0 <= sweeps <= CWQ_MAX_BACKFIT_SWEEPS
 *   block_off     device [nb + 1], or NULL for uniform blocks of max_block_dim
 *                 dims (total_dims = nb * max_block_dim)
 *   idx_inout     [nb * n_steps] int32, device: the table, refined in place.
 *                 Every entry must lie in [0, N).  The table is device memory
 *                 and this call does not wait for the device, so the host
 *                 cannot check it: the bindings check before they call.  An
 *                 entry outside the range touches no memory it should not
 *                 (an index only selects a row of the stream) but the block's
 *                 results are then unspecified.
 *   out_sample    [total_dims] f32 (also the vector carried between launches)
 *   out_value     [nb] f32 or NULL
 *   out_accepted  [nb] int32 or NULL
 *   opts          prune_mode selects the scoring kernels as in
 *                 cwq_greedy_encode (results never depend on it); the eval
 *                 events bracket the scoring launches.
 * Each step of a sweep is one scoring launch of the greedy encoder in its
 * step > 0 form against base_s, so a sweep costs about one cwq_greedy_encode.
 * A block is handled by one wave (or lane) alone: results do not depend on
 * timing.  Asynchronous on `stream`, no host synchronisation, no other stream:
 * capturable into a graph.  Workspace: cwq_greedy_encode_workspace_size(nb,
 * total_dims, max_block_dim) (each array rounded up to 256) + 4 * n_steps *
 * total_dims (the selected rows) + 2 * 4 * nb (v and the counts). */
#define CWQ_MAX_BACKFIT_SWEEPS 16
size_t cwq_greedy_backfit_workspace_size(int64_t nb, int64_t total_dims, int64_t max_block_dim,
                                         int n_steps);
int cwq_greedy_backfit(const float* t_loc, const float* t_scale, const float* p_loc,
                       const float* p_scale, const int64_t* block_off, int64_t nb,
                       int64_t total_dims, int64_t max_block_dim, int n_bits_per_step,
                       int n_steps, int sweeps, int32_t seed, float rho, int64_t block_id_base,
                       int32_t* idx_inout, float* out_sample, float* out_value,
                       int32_t* out_accepted, void* workspace, size_t workspace_bytes,
                       const cwq_options* opts, void* stream);

/* Backfitting under per-block bit budgets.  Block g is refined exactly as
 * cwq_greedy_backfit refines it in a call of its own with n_bits_per_step =
 * n_bits[g] and block seed seed + block_id_base + g: N_g = 2^n_bits[g] rows per
 * step, the same sweeps, the same accept test.  A block at n_bits[g] = 0, an
 * empty block and a code of one step are returned as given; sweeps = 0 returns
 * the table with its decoded sample and value.  The table is that of
 * cwq_greedy_encode_var / cwq_greedy_encode_uniform_var (or any other whose row
 * g lies in [0, N_g)), the result goes to the same decoders and
 * cwq_pack_indices_var.
 *   block_off     device [nb + 1], or NULL for uniform blocks of max_block_dim
 *                 dims (total_dims = nb * max_block_dim)
 *   n_bits        device [nb] int32, each in [0, CWQ_MAX_BITS_PER_STEP]
 *   idx_inout, out_sample, out_value, out_accepted, sweeps, opts: as above; the
 *                 eval events bracket the first to the last scoring launch of
 *                 the call (an empty bracket when there is none).
 * The blocks are sorted by budget as in cwq_greedy_encode_var; a step of a
 * sweep is one scoring launch sequence per budget in use (none for budget 0)
 * between two launches over all blocks, all on `stream`.  Results never depend
 * on prune_mode, launch geometry or timing.
 * The call waits for the device once, as cwq_greedy_encode_var does, because
 * the bucket sizes decide the launches: it cannot be captured into a graph.
 * In that one wait it also validates what lives on the device, so unlike
 * cwq_greedy_backfit it refuses an out-of-range table itself: CWQ_ERR_INVALID
 * with the number of entries outside [0, N_g), and likewise for n_bits outside
 * [0, 30] and a decreasing block_off.  On every refusal idx_inout, out_sample,
 * out_value and out_accepted have not been written: the call works on a sorted
 * copy of the table in the workspace and writes the caller's arrays only in its
 * last launches.
 * Workspace (no size function of its own; less returns CWQ_ERR_WORKSPACE):
 *   ragged   cwq_greedy_encode_var_workspace_size(nb, total_dims, max_block_dim,
 *            n_steps) + cwq_greedy_backfit_workspace_size(nb, total_dims,
 *            max_block_dim, n_steps) - cwq_greedy_encode_workspace_size(nb,
 *            total_dims, max_block_dim)
 *   uniform  cwq_greedy_encode_uniform_var_workspace_size(nb, d) +
 *            round256(4 * nb * n_steps) + cwq_greedy_backfit_workspace_size(nb,
 *            nb * d, d, n_steps) - cwq_greedy_encode_workspace_size(nb, nb * d, d)
 * with d = max_block_dim and round256 the next multiple of 256. */
int cwq_greedy_backfit_var(const float* t_loc, const float* t_scale, const float* p_loc,
                           const float* p_scale, const int64_t* block_off /* NULL: uniform */,
                           int64_t nb, int64_t total_dims, int64_t max_block_dim,
                           const int32_t* n_bits /* device [nb], each in [0, 30] */,
                           int n_steps, int sweeps, int32_t seed, float rho,
                           int64_t block_id_base, int32_t* idx_inout, float* out_sample,
                           float* out_value, int32_t* out_accepted, void* workspace,
                           size_t workspace_bytes, const cwq_options* opts, void* stream);


/* ---- rate tables: the winning index at every budget ----
 * Single-step codes only.  Candidate row n of a block is drawn from the flat
 * indices n d + j of the block's one stream whatever the budget, so the 2^b
 * rows of a b-bit code are the first 2^b rows of a B-bit code, and one call can
 * answer for every budget b = 0 .. max_bits:
 *   out_idx[g * (max_bits + 1) + b]    the index cwq_greedy_encode /
 *                 cwq_greedy_encode_uniform writes for block g with
 *                 n_bits_per_step = b, n_steps = 1 and the same seed, rho and
 *                 block_id_base;
 *   out_value[g * (max_bits + 1) + b]  the value that row's argmax key holds:
 *                 the float32 log-density of the row in the coder's summation
 *                 order, NaN and anything <= -FLT_MAX as -FLT_MAX, -0 as +0.
 * A block none of whose rows scores above -FLT_MAX gets index 0 at -FLT_MAX, an
 * empty block index 0 at +0, in every column.
 *   block_off     device [nb + 1], or NULL for uniform blocks of max_block_dim
 *                 dims (total_dims = nb * max_block_dim)
 *   max_bits      B in [0, CWQ_MAX_BITS_PER_STEP]
 *   out_idx       device [nb, B + 1] int32; out_value device [nb, B + 1] float
 *   opts          prune_mode selects the scoring kernels of the budgets from 12
 *                 bits on, as in cwq_greedy_encode; results never depend on it.
 *                 The eval events are not recorded.
 * Budgets 0 .. min(B, 11) come from one launch that scores rows [0, 2^11) of
 * every block once; each budget from 12 on takes the launches of one
 * cwq_greedy_encode at that budget, so the call costs about two encodes at B
 * bits.  Everything is enqueued on `stream`: no host wait, no allocation, no
 * memset or copy; the call can be captured into a graph.
 * Workspace: cwq_rate_table_workspace_bytes(nb, total_dims, max_block_dim,
 * max_bits) (for uniform blocks total_dims = nb * max_block_dim), which is the
 * encoder's layout plus 8 * 12 * nb + 8 * max(B - 11, 0) * nb bytes of keys, a
 * scratch sample (4 * total_dims) and, from 12 bits on, scratch indices (4 * nb);
 * less returns CWQ_ERR_WORKSPACE.  Its contents before the call do not matter. */
size_t cwq_rate_table_workspace_bytes(int64_t nb, int64_t total_dims, int64_t max_block_dim,
                                      int max_bits);
int cwq_rate_table(const float* t_loc, const float* t_scale, const float* p_loc,
                   const float* p_scale, const int64_t* block_off /* NULL: uniform */,
                   int64_t nb, int64_t total_dims, int64_t max_block_dim, int max_bits,
                   int32_t seed, float rho, int64_t block_id_base, int32_t* out_idx,
                   float* out_value, void* workspace, size_t workspace_bytes,
                   const cwq_options* opts, void* stream);

/* Budgets from a rate table.  out_bits[g] = the lowest b in [min_bits,
 * min(max_bits, max_bits_table)] that maximises
 *     (double)value[g * (max_bits_table + 1) + b] - lam * (double)b,
 * a float64 multiply, then a float64 subtract (no fused multiply-add), compared
 * with >: lam is the price of a bit in nats.
 *   value         device [nb, max_bits_table + 1], cwq_rate_table's out_value
 *   lam           finite and >= 0 (anything else, a NaN included, is refused)
 *   out_bits      device [nb] int32: cwq_greedy_encode_var's n_bits
 *   out_total     device, one int64: the sum of out_bits; or NULL
 * Two launches on `stream` (one without out_total); no host wait. */
int cwq_choose_bits(const float* value, int64_t nb, int max_bits_table, double lam, int min_bits,
                    int max_bits, int32_t* out_bits, int64_t* out_total, void* stream);

/* Budgets from a rate table whose sum is at most total_bits:
 * cwq_choose_bits at the price lam that 60 halvings of an interval find.  With
 * lo = min_bits, hi = min(max_bits, max_bits_table) and total(lam) the sum of
 * cwq_choose_bits(value, ..., lam, lo, hi):
 *   total(0) <= total_bits: lam = 0.  Else the interval starts as (0, the largest
 *   (double)value[g, b] - (double)value[g, lo] over g and b in [lo, hi]); 60
 *   times mid = 0.5 * (low end + high end) in float64 and the high end moves to
 *   mid when total(mid) <= total_bits, the low end otherwise; lam = the high end.
 * The totals are taken three halvings at a time, for the 7 mids those halvings
 * can reach, in one pass over the table; the result is bit for bit the one of
 * the 60 single steps.
 *   out_bits      device [nb] int32: cwq_choose_bits at lam
 *   out_lam       device, one double: lam
 *   out_total     device, one int64: the sum of out_bits; at most total_bits for
 *                 every finite table
 * Refused with CWQ_ERR_INVALID before any launch: the ranges cwq_choose_bits
 * refuses, and nb * min_bits > total_bits (no budgets fit).
 * Enqueues 44 launches on `stream`: no host wait, no allocation, no memset or
 * copy; the call can be captured into a graph.  nb = 0: nothing is launched.
 * Workspace: cwq_choose_bits_total_workspace_bytes(max_bits_table); less returns
 * CWQ_ERR_WORKSPACE.  Its contents before the call do not matter. */
size_t cwq_choose_bits_total_workspace_bytes(int max_bits_table);
int cwq_choose_bits_total(const float* value, int64_t nb, int max_bits_table, int64_t total_bits,
                          int min_bits, int max_bits, int32_t* out_bits, double* out_lam,
                          int64_t* out_total, void* workspace, size_t workspace_bytes,
                          void* stream);

/* A single-step code under a bit total from the distributions, in one call:
 * cwq_rate_table's launches into a table inside the workspace,
 * cwq_choose_bits_total on it with budgets in [min_bits, max_bits], the table's
 * index at each block's budget, and the decoder for the sample.  The first nine
 * arguments, seed, rho, block_id_base and opts are cwq_rate_table's.
 *   out_idx       device [nb] int32: block g's index at out_bits[g] bits, what
 *                 cwq_greedy_encode_var writes for these budgets at n_steps = 1
 *   out_sample    device [total_dims]: cwq_greedy_decode(_uniform) of out_idx
 *   out_bits, out_lam, out_total   as cwq_choose_bits_total writes them
 *   out_value     device [nb, max_bits + 1], or NULL: the table's values
 * Refusals: cwq_rate_table's and cwq_choose_bits_total's.  Everything is
 * enqueued on `stream`: no host wait, no allocation, no memset or copy; the
 * call can be captured into a graph.  nb = 0: nothing is launched.
 * Workspace: cwq_greedy_encode_rate_workspace_bytes(nb, total_dims,
 * max_block_dim, max_bits): cwq_rate_table's, the table (8 * nb * (max_bits + 1)
 * bytes) and the solver's; less returns CWQ_ERR_WORKSPACE.  Its contents before
 * the call do not matter. */
size_t cwq_greedy_encode_rate_workspace_bytes(int64_t nb, int64_t total_dims,
                                              int64_t max_block_dim, int max_bits);
int cwq_greedy_encode_rate(const float* t_loc, const float* t_scale, const float* p_loc,
                           const float* p_scale, const int64_t* block_off /* NULL: uniform */,
                           int64_t nb, int64_t total_dims, int64_t max_block_dim, int max_bits,
                           int64_t total_bits, int min_bits, int32_t seed, float rho,
                           int64_t block_id_base, int32_t* out_idx, float* out_sample,
                           int32_t* out_bits, double* out_lam, int64_t* out_total,
                           float* out_value /* or NULL */, void* workspace,
                           size_t workspace_bytes, const cwq_options* opts, void* stream);

/* ---- PLN image codec plumbing (csrc/cwq_pln.hip) ----
 * The ladder network's transforms are library convolutions; these three
 * stream kernels connect them to the coders.  Latent tensors are NCHW with
 * batch 1 (C channels, HW = H*W positions); the reference flattens them in
 * TF's NHWC order, index f = hw*C + c. */

/* pln.py:165-185: level-1 posterior = precision-weighted combination of the
 * likelihood N(lik_loc, lik_scale) (AnalysisTransform_1) and the prior
 * N(prior_loc, prior_scale) (SynthesisTransform_2), float32 in the
 * reference's order: lp = 1/(lik_scale^2 + eps), pp = 1/(prior_scale^2 + eps),
 * var = 1/(lp + pp), scale = sqrt(var), loc = (lik_loc*pp + prior_loc*lp)*var.
 * Elementwise over n values; any layout. */
int cwq_pln_posterior(const float* lik_loc, const float* lik_scale, const float* prior_loc,
                      const float* prior_scale, int64_t n, float eps, float* loc, float* scale,
                      void* stream);

/* pln.py:264-273 + :316-324: out[i] = src_nhwc[perm[i]] for i < C*HW, i.e.
 * tfp.bijectors.Permute(perm).forward(tf.reshape(x_nhwc, [-1])), reading the
 * NCHW tensor src.  perm: device int32 [C*HW] permutation, or NULL for the
 * identity (use_permutation=False). */
int cwq_permute_gather(const float* src, int64_t C, int64_t HW, const int32_t* perm, float* out,
                       void* stream);

/* pln.py:394-397, :770-772, :801-803: the inverse, Permute.inverse and the
 * reshape back to the latent shape, written NCHW: out_nchw[c*HW + hw] = src[i]
 * where perm[i] = hw*C + c. */
int cwq_permute_scatter(const float* src, int64_t C, int64_t HW, const int32_t* perm, float* out,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CWQ_H_ */
