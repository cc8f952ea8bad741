// cwq_workspace.h -- how every caller-provided workspace is cut into arrays,
// each layout defined once: the *_workspace_size functions read its total, the
// entry points and launchers take their pointers from its regions, and
// tests/test_workspace_layout.py checks every layout on the host (DESIGN.md
// 3b "Workspace state").
//
// Everything here is a pure function of the call's shape; no pointer is read
// except by at<T>().  Host only: it includes nothing from HIP.  The layouts
// are plain structs computed on the stack: the per-call paths run them on
// every call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "cwq_dispatch.h"
#include "cwq_rate_plan.h"
#include "cwq_rate_solve.h"

// Tuning switches of the sizes (tools/variants.sh builds with -D...).
#ifndef CWQ_CSR_GTAU_STRIDE
#define CWQ_CSR_GTAU_STRIDE 1  // words between blocks' shared thresholds (tuning builds)
#endif
#ifndef CWQ_DEFER_Q
// rows per block that k_encode_prune's screening-only form lists for
// k_score_survivors (at most kDeferSlots); a block with more is deferred.  The
// smallest that defers under 0.1% of C4's blocks: 0.599% of them have more than
// one such row, 0.0025% more than two (tools/defer_stats.py)
#define CWQ_DEFER_Q 2
#endif
#define CWQ_SLIST_PER_BLOCK 8  // survivor slots per block of the screened small-candidate path

namespace cwq {

// ---- sizing constants the kernels share with the layouts -------------------
constexpr int kTileQueueSlots = 64;  // k_encode_prune's tile queue counters (one per fork part)
// First entry of a long block's visit-order records (abp, 32 B per entry) is
// csr_rec_base(off) (cwq_kernels.h).  Only blocks of more than CWQ_CSR_LDS_DIMS
// dims have records, and two of them start at least CWQ_CSR_LDS_DIMS + 1 dims
// apart, so each gets a disjoint region of d + 12 entries and the array needs
// csr_rec_entries(total_dims) entries however many short blocks there are.
inline int64_t csr_rec_entries(int64_t total_dims) {
  return total_dims + 12 * (total_dims / (CWQ_CSR_LDS_DIMS + 1) + 1);
}
// variable budgets (cwq_varbits.hip)
constexpr int kVbThreads = 256;
constexpr int kVbPerThread = 8;
constexpr int kVbTile = kVbThreads * kVbPerThread;  // blocks per workgroup (sort, offsets)
constexpr int kVbBins = 32;                         // bit counts 0..30, 31: out of range
constexpr int kVbcFactsRow = 2 * kVbBins + 2;       // u64 per workgroup of the buckets' facts
constexpr size_t kVbcFactsBytes = 1032;             // sizeof(VbcFacts) (cwq_kernels.h asserts it)
inline int64_t vb_tiles(int64_t nb) { return (nb + kVbTile - 1) / kVbTile; }
// the device partition (cwq_partition.hip)
constexpr int kPartW = 1024;      // dims per chunk
constexpr int kPartSuper = 256;   // chunks per superchunk (k_part_sup's sums)
constexpr size_t kBatchItemBytes = 80;  // sizeof(BatchItem) (cwq_kernels.h asserts it)

// ---- the arena --------------------------------------------------------------
// A region of a workspace: where it starts and the bytes asked for it (the
// room up to the next region may be larger by the rounding).
struct Region {
  size_t off, bytes;
};
// A running offset.  take() starts the next region at the next multiple of 256
// past this one; take_packed() right behind it (the few unrounded steps: arrays
// that cross PCIe in one copy, the partition's counters).
struct Arena {
  size_t o = 0;
  static size_t up(size_t v) { return (v + 255) / 256 * 256; }
  Region take(size_t bytes) {
    const Region r{o, bytes};
    o = up(o + bytes);
    return r;
  }
  Region take_packed(size_t bytes) {
    const Region r{o, bytes};
    o += bytes;
    return r;
  }
  // A region that holds what `inner`, an arena started at this one's offset,
  // has taken: its sub-regions are laid out before their container is.
  Region take(const Arena& inner) { return take(inner.o - o); }
};
template <class T>
inline T* at(void* base, const Region& r) {
  return (T*)((char*)base + r.off);
}

// ---- the block coder (cwq_greedy_encode*, launch_encode) ----------------------
// screen (has_screen_arrays, cwq_dispatch.h): 24 B/dim + 244 B/block; recs
// (has_long_block_records): 32 B/dim + 384 B per CWQ_CSR_LDS_DIMS + 1 dims
// (csr_rec_entries: short blocks take no room, so a grouped call sized for
// D + 1 possible groups does not pay 384 B for each).  Arrays a shape does not
// have are empty regions.
struct EncWs {
  Region keys, tq, loc_s, scale_s, lognorm, slist, sab, cdim, bpre, ordu, grp, gtau, sdmap, abp;
  size_t total;
  bool screen;  // has_screen_arrays: the general pruned kernel's and the small paths' arrays
  bool recs;    // has_long_block_records: visit-order records of blocks > CWQ_CSR_LDS_DIMS
};
inline EncWs enc_ws(int64_t nb, int64_t total_dims, bool screen, bool recs) {
  EncWs l;
  Arena a;
  const size_t n = (size_t)nb, D = (size_t)total_dims;
  l.screen = screen;
  l.recs = screen && recs;
  l.keys = a.take(n * 8);
  l.tq = a.take((size_t)kTileQueueSlots * 4);  // k_encode_prune's tile queue counters
  l.loc_s = a.take(D * 4);
  l.scale_s = a.take(D * 4);
  l.lognorm = a.take(D * 4);
  // the screened small-candidate path's survivor slots (8 B each)
  l.slist = a.take(screen ? n * CWQ_SLIST_PER_BLOCK * 8 : 0);
  l.sab = a.take(screen ? (D + 8 * n + 4) * 8 : 0);  // + 4 zeros (pad unit)
  l.cdim = a.take(screen ? D * 4 : 0);
  l.bpre = a.take(screen ? (D + 12 * n) * 4 : 0);
  l.ordu = a.take(screen ? (D + 12 * n) * 4 : 0);
  l.grp = a.take(screen ? n * 16 : 0);
  l.gtau = a.take(screen ? n * 4 * CWQ_CSR_GTAU_STRIDE : 0);
  l.sdmap = a.take(screen ? D * 4 : 0);  // the small-candidate pipeline's dim -> block map
  l.abp = a.take(l.recs ? (size_t)csr_rec_entries(total_dims) * 32 : 0);
  l.total = a.o;
  return l;
}
// CSR blocks of at most max_block_dim dims
inline EncWs enc_ws_csr(int64_t nb, int64_t total_dims, int64_t max_block_dim) {
  return enc_ws(nb, total_dims, has_screen_arrays(true, 0, nb),
                has_long_block_records(true, max_block_dim, nb));
}
inline EncWs enc_ws_uniform(int64_t nb, int64_t d) {
  return enc_ws(nb, nb * d, has_screen_arrays(false, d, nb), has_long_block_records(false, d, nb));
}

// ---- deferred exact work of the pruned uniform encoder (DESIGN.md 4 "Deferral") ----
// Behind the encoder's layout, for the shapes k_encode_prune runs one tile per
// block at (defer_shape): the screening-only launch leaves per block
//   surv   [nb][kDeferSlots] u32: the rows that reach the tile's final tau
//   count  [nb] u32: how many of its slots are filled, 0 .. Q <= kDeferSlots;
//          0 also for a block that is on the deferred list
//   dlist  [nb] u32: the blocks whose tile runs again in the full kernel
//   dcount one u32: their number (zeroed on the stream before the launch)
// The encoder's own layout and cwq_greedy_encode_uniform_workspace_size stay
// what they were: a caller that sizes its workspace with
// cwq_greedy_encode_uniform_defer_bytes gets these regions behind it and the
// three-launch form; one that gives the smaller size gets the single launch.
constexpr int kDeferSlots = 4;  // slots per block: the largest Q
constexpr int kDeferQ = CWQ_DEFER_Q;  // Q: rows per block that the dense scoring launch takes
inline bool defer_shape(int64_t nb, int64_t d) {
  return nb > 0 && nb < (1LL << 31) && d % 8 == 0 && d >= 8 && d <= 64;
}
// (constexpr: the kernels index with it too)
constexpr size_t defer_slot(int64_t g, int q) { return (size_t)g * kDeferSlots + (size_t)q; }
// the count word of a block with c rows listed (c > Q: deferred, no row listed)
constexpr uint32_t defer_count_word(uint32_t c, int Q) { return c <= (uint32_t)Q ? c : 0u; }
struct DeferWs {
  Region surv, count, dlist, dcount;
  size_t total;
};
inline DeferWs defer_ws(size_t enc_total, int64_t nb, int64_t d) {
  DeferWs l;
  Arena a{Arena::up(enc_total)};
  const size_t n = defer_shape(nb, d) ? (size_t)nb : 0;
  l.surv = a.take(n * kDeferSlots * 4);
  l.count = a.take(n * 4);
  l.dlist = a.take(n * 4);
  l.dcount = a.take(n ? 4 : 0);
  l.total = a.o;
  return l;
}
inline DeferWs defer_ws_uniform(int64_t nb, int64_t d) {
  return defer_ws(enc_ws_uniform(nb, d).total, nb, d);
}

// ---- blocks sorted by bit budget: the sorted view (cwq_capi.hip sort_blocks) ----
// What the three budget calls share.  Uniform blocks have the four sorted inputs
// back to back (unrounded) in `sorted_in`; ragged blocks have a region for each,
// and the sorted layout's arrays (launch_vbc_layout) behind the counts.  Regions
// the blocks' form does not have are empty.
struct SortedWs {
  Region sorted_in, t_loc, t_scale, p_loc, p_scale;  // sorted_in: the four behind it (uniform)
  Region sample, seeds, perm, hist, counts;
  Region wgfacts, facts, soff, roff, src, partial;  // ragged blocks only
};
inline SortedWs sorted_ws(Arena& a, bool csr, int64_t nb, int64_t total_dims) {
  SortedWs l{};
  const size_t n = (size_t)nb, row = (size_t)total_dims * 4, tiles = (size_t)vb_tiles(nb);
  Arena in{a.o};
  auto input = [&] { return csr ? a.take(row) : in.take_packed(row); };
  l.t_loc = input(), l.t_scale = input(), l.p_loc = input(), l.p_scale = input();
  if (!csr) l.sorted_in = a.take(in);
  l.sample = a.take(row);
  l.seeds = a.take(n * 4);
  l.perm = a.take(n * 4);
  l.hist = a.take(tiles * kVbBins * 4);
  l.counts = a.take(32 * 4);
  if (csr) {
    l.wgfacts = a.take(tiles * kVbcFactsRow * 8);
    l.facts = a.take(kVbcFactsBytes);
    l.soff = a.take((n + 1) * 8);
    l.roff = a.take((n + 33) * 8);
    l.src = a.take(n * 8);
    l.partial = a.take(tiles * 8);
  }
  return l;
}

// ---- uniform blocks with a bit budget each (cwq_greedy_encode_uniform_var) ----
// Every bucket's encode runs in `enc`, sized for the whole call (no bucket's
// layout exceeds it).  The encoders write the sorted index rows into the
// caller's out_idx; they are staged for the scatter in the sorted inputs'
// region (16 nb d bytes, dead by then) when 4 nb n_steps bytes fit there, i.e.
// n_steps <= 4 d, else in a tail of that size:
// cwq_greedy_encode_uniform_var_workspace_size is n_steps = 1.
struct VarWs {
  SortedWs s;
  Region enc, stage;
  size_t total;
  bool stage_aliases_sorted_in;
};
inline VarWs var_ws(int64_t nb, int64_t d, int64_t n_steps) {
  VarWs l;
  Arena a;
  l.s = sorted_ws(a, false, nb, nb * d);
  l.enc = a.take(enc_ws_uniform(nb, d).total);
  l.stage_aliases_sorted_in = n_steps <= 4 * d;
  const size_t stage = (size_t)nb * (size_t)n_steps * 4;
  l.stage = l.stage_aliases_sorted_in ? Region{l.s.sorted_in.off, stage} : a.take(stage);
  l.total = a.o;
  return l;
}

// cwq_pack_indices_var / cwq_unpack_indices_var
struct PackWs {
  Region off, partial, flag;
  size_t total;
};
inline PackWs pack_ws(int64_t nb) {
  PackWs l;
  Arena a;
  l.off = a.take((size_t)(nb + 1) * 8);
  l.partial = a.take((size_t)vb_tiles(nb) * 8);
  l.flag = a.take(4);
  l.total = a.o;
  return l;
}

// ---- ragged blocks with a bit budget each (cwq_greedy_encode_var) -------------
// Every bucket is a CSR encode in `enc`, sized for the whole call's nb,
// total_dims and max_block_dim, which no bucket exceeds (enc_ws_csr is monotone).
inline VarWs var_csr_ws(int64_t nb, int64_t total_dims, int64_t max_block_dim, int64_t n_steps) {
  VarWs l{};
  Arena a;
  l.s = sorted_ws(a, true, nb, total_dims);
  l.stage = a.take((size_t)nb * (size_t)n_steps * 4);  // a region of its own
  l.enc = a.take(enc_ws_csr(nb, total_dims, max_block_dim).total);
  l.total = a.o;
  return l;
}

// ---- the device partition (launch_partition) ----------------------------------
// Counters per dim, per chunk and per superchunk, back to back, and 64 spare
// words; the total is rounded, callers place 8-byte words right after it.
struct PartWs {
  Region nxt, exg, node, gnode, conv, cnt, sup, spare;
  size_t total;
};
inline PartWs part_ws(int64_t D) {
  PartWs l;
  Arena a;
  const int64_t nch = (D + kPartW - 1) / kPartW, nsup = (nch + kPartSuper - 1) / kPartSuper;
  l.nxt = a.take_packed((size_t)(D + 64) * 4);
  l.exg = a.take_packed((size_t)(D + 64) * 4);
  l.node = a.take_packed((size_t)(D + 64) * 4);
  l.gnode = a.take_packed((size_t)(D + 64) * 4);
  l.conv = a.take_packed((size_t)(nch + 64) * 4);
  l.cnt = a.take_packed((size_t)(nch + 64) * 4);
  l.sup = a.take_packed((size_t)(nsup + 64) * 4);
  l.spare = a.take(64 * 8);
  l.total = a.o;
  return l;
}
// cwq_debug_group_starts_device: the partition and its info block (partition
// info[8] + item info[2], 16 words), unrounded
struct PartDebugWs {
  PartWs part;
  Region info;
  size_t total;
};
inline PartDebugWs part_debug_ws(int64_t D) {
  PartDebugWs l;
  l.part = part_ws(D);
  Arena a{l.part.total};
  l.info = a.take_packed(16 * 8);
  l.total = a.o;
  return l;
}

// ---- the grouped greedy coder (cwq_code_grouped_greedy*) ----------------------
// D dims in at most max_groups groups (a partition of D dims has at most D + 1:
// the reference's forced boundary at D - 1 can leave an empty first group).
// `enc` is sized for (G, D, D) and runs at (groups, D, longest group) with
// groups <= G and a longest group <= D, which is never more (monotone).
struct GroupedWs {
  Region t_loc, t_scale, kl, zeros, ones, sample, out, offs, idx, part, pinfo, enc;
  size_t total;
};
inline GroupedWs grouped_ws(int64_t D, int n_steps, int64_t max_groups) {
  GroupedWs l;
  Arena a;
  const int64_t Dz = D > 0 ? D : 0, G = max_groups > 1 ? max_groups : 1;
  const size_t fd = (size_t)Dz * 4;
  l.t_loc = a.take(fd);
  l.t_scale = a.take(fd);
  l.kl = a.take(fd);
  l.zeros = a.take(fd);
  l.ones = a.take(fd);
  l.sample = a.take(fd);
  l.out = a.take(fd);
  l.offs = a.take((size_t)(G + 1) * 8);
  l.idx = a.take((size_t)G * (size_t)(n_steps > 0 ? n_steps : 1) * 4);
  l.part = a.take(part_ws(Dz).total);  // device partition scratch
  l.pinfo = a.take(16 * 8);            // partition info[8] + item info[2]
  l.enc = a.take(enc_ws_csr(G, D, D).total);
  l.total = a.o;
  return l;
}
// Device workspace of the batch: the grouped layout for D dims, with the
// per-chunk regions of the group-indexed arrays (chunk c of a call owns
// [a_c + i0_c, ...) of them, a_c its first dim and i0_c its first item, so
// chunks never share a slot however their group counts come out): offsets
// D + 2 n + 1 entries, indices / seeds D + n.  Then the device partition's:
// item offsets, the items' start lists (the host layout: item i at
// item_off[i] + 2 i), per-item counts, the layout table, and the start lists
// packed back to back (at most D_i + 2 entries each).
struct BatchWs {
  GroupedWs g;
  Region seeds, ioff, dstarts, iinfo, itab, pstarts;
  size_t total;
};
inline BatchWs batch_ws(int64_t D, int64_t n_items, int n_steps) {
  BatchWs l;
  const int64_t n = n_items > 0 ? n_items : 0;
  l.g = grouped_ws(D, n_steps, D + 2 * n + 1);
  Arena a{l.g.total};
  l.seeds = a.take((size_t)(D + n + 1) * 4);
  l.ioff = a.take((size_t)(n + 1) * 8);
  l.dstarts = a.take((size_t)(D + 2 * n + 1) * 8);
  l.iinfo = a.take((size_t)(4 * n + 4) * 8);
  l.itab = a.take((size_t)(n + 1) * kBatchItemBytes);
  l.pstarts = a.take((size_t)(D + 2 * n + 1) * 8);
  l.total = a.o;
  return l;
}
// Host staging of the batch (the caller's pinned memory, or thread-local
// vectors): per-dim KL, then the offsets / seeds / indices regions as above.
struct BatchHostWs {
  Region kl, offs, seeds, idx;
  size_t total;
};
inline BatchHostWs batch_host_ws(int64_t D, int64_t n_items, int n_steps) {
  BatchHostWs l;
  Arena a;
  const int64_t n = n_items > 0 ? n_items : 0;
  l.kl = a.take((size_t)D * 4);
  l.offs = a.take((size_t)(D + 2 * n + 1) * 8);
  l.seeds = a.take((size_t)(D + n + 1) * 4);
  l.idx = a.take((size_t)(D + n + 1) * (size_t)(n_steps > 0 ? n_steps : 1) * 4);
  l.total = a.o;
  return l;
}

// ---- the importance coder (cwq_importance_encode, launch_importance_encode) ---
struct ImpWs {
  Region keys, tprefix, lnt, lnp, gtau, next_tile, cpt;
  size_t total;
};
inline ImpWs imp_ws(int64_t nb, int64_t total_dims) {
  ImpWs l;
  Arena a;
  l.keys = a.take((size_t)nb * 8);
  l.tprefix = a.take((size_t)(nb + 1) * 8);
  l.lnt = a.take((size_t)total_dims * 4);
  l.lnp = a.take((size_t)total_dims * 4);
  l.gtau = a.take((size_t)nb * 4);
  l.next_tile = a.take_packed(8);  // k_imp_eval's tile counter, then the candidates per tile
  l.cpt = a.take(8);
  l.total = a.o;
  return l;
}

// ---- the grouped importance coder (cwq_code_grouped_importance*) --------------
// What crosses PCIe sits in packed regions, one copy each, laid out identically
// in the device workspace and in the host staging: res = [sample | indices] (to
// the host at the end), d2h = [KL | outlier draws | kept flags] (to the host
// after the preparation launch), plan = [counts | offsets | seeds] (to the
// device; see imp_plan), items = [item offsets | seeds - 1] (to the device,
// batches).  n dims, at most g groups, ni items.
struct ImpXfer {
  Region out, idx, res;           // res: the two before it
  Region kl, tsamp, keep, d2h;    // d2h: the three before it
  Region plan;
  Region item_off, seed1, items;  // items: the two before it
};
inline ImpXfer imp_xfer(Arena& a, size_t n, size_t g, size_t ni) {
  ImpXfer x;
  Arena in{a.o};
  x.out = in.take(n * 4);
  x.idx = in.take_packed(g * 8);
  x.res = a.take(in);
  in = Arena{a.o};
  x.kl = in.take(n * 4);
  x.tsamp = in.take(n * 4);
  x.keep = in.take_packed(n);
  x.d2h = a.take(in);
  x.plan = a.take(Arena::up(g * 8) + Arena::up((g + 1) * 8) + g * 4);
  in = Arena{a.o};
  x.item_off = in.take((ni + 1) * 8);
  x.seed1 = in.take_packed(ni * 4);
  x.items = a.take(in);
  return x;
}
// The plan region for the G groups a call came out with (G <= g, so it stays
// inside the region): counts, offsets, seeds; copy_bytes: what one copy moves
// (the seeds only with per-item seeds).
struct ImpPlan {
  Region counts, offs, seeds;
  size_t copy_bytes;
};
inline ImpPlan imp_plan(const Region& plan, int64_t G, bool seeds) {
  ImpPlan p;
  Arena a{plan.off};
  p.counts = a.take((size_t)G * 8);
  p.offs = a.take((size_t)(G + 1) * 8);
  p.seeds = a.take_packed((size_t)G * 4);
  p.copy_bytes = (seeds ? a.o : p.offs.off + p.offs.bytes) - plan.off;
  return p;
}
// D dims in I items: at most D + I groups (an item's partition has at most
// D_i + 1 groups).
struct GroupedImpWs {
  Region t_loc, t_scale, zeros, ones, sample;
  ImpXfer x;
  Region enc;
  size_t total;
};
inline GroupedImpWs grouped_imp_ws(int64_t D, int64_t I) {
  GroupedImpWs l;
  Arena a;
  const size_t n = (size_t)(D > 0 ? D : 0), ni = (size_t)(I > 0 ? I : 0), g = n + ni;
  l.t_loc = a.take(n * 4);
  l.t_scale = a.take(n * 4);
  l.zeros = a.take(n * 4);
  l.ones = a.take(n * 4);
  l.sample = a.take(n * 4);
  l.x = imp_xfer(a, n, g, ni);
  l.enc = a.take(imp_ws((int64_t)g, (int64_t)n).total);
  l.total = a.o;
  return l;
}
// The call's host staging (thread-local, page-locked): the packed regions and,
// for a batch, the per-item plans (item i's at item_off[i] + i).
struct GroupedImpHostWs {
  ImpXfer x;
  Region nst;
  size_t total;
};
inline GroupedImpHostWs grouped_imp_host_ws(int64_t D, int64_t I) {
  GroupedImpHostWs l;
  Arena a;
  l.x = imp_xfer(a, (size_t)D, (size_t)(D + I), (size_t)I);
  l.nst = a.take(I > 1 ? (size_t)(D + I) * 8 : 0);
  l.total = a.o;
  return l;
}

// ---- the batched grouped decoders ----------------------------------------------
// The plan as it lies in the host staging and in the device workspace: group
// offsets (G + 1), the slot prefix (G + 1; greedy only), seeds (G), indices.
// One layout for both sides: a call plans the G groups it decodes, G <= the
// G_total its workspaces were sized for, so the plan fits either.
struct DecPlan {
  Region off, slot, seeds, idx;
  size_t total;
};
inline DecPlan dec_plan(int64_t G, bool slots, size_t idx_bytes_per_group) {
  DecPlan l;
  Arena a;
  const size_t Gz = (size_t)(G > 0 ? G : 0);
  l.off = a.take((Gz + 1) * 8);
  l.slot = a.take(slots ? (Gz + 1) * 8 : 0);
  l.seeds = a.take(Gz * 4);
  l.idx = a.take(Gz * idx_bytes_per_group);
  l.total = a.o;
  return l;
}
// The device workspace: the plan for G_total groups, then the decoded sample
// (used when the caller gives no device output).
struct DecWs {
  DecPlan plan;
  Region out;
  size_t total;
};
inline DecWs dec_ws(int64_t D, int64_t G, bool slots, size_t idx_bytes_per_group) {
  DecWs l;
  l.plan = dec_plan(G, slots, idx_bytes_per_group);
  Arena a{l.plan.total};
  l.out = a.take((size_t)D * 4);
  l.total = a.o;
  return l;
}

// ---- beam search over steps (cwq_beam.hip) -----------------------
//   loc_s, scale_s, lognorm  [total_dims] f32: the step's shard and normaliser
//   beams   [2][beam][total_dims] f32: the running sums, ping-pong
//   tiles   [nb][beam_tiles_cap(nb)][beam] u64: every tile's largest keys
//   sel     [nb][n_steps][beam] u64: the selected keys, sorted; key j of a step
//           names beam j's parent and row (candidate parent * 2^b + row)
// cwq_beam_encode_var takes this layout as it is: the size does
// not depend on the bit counts, and there is no layout or size function of its
// own.  It addresses `tiles` as [nb][stride][beam] with stride =
// beam_tiles_per_block at 2^max_bits <= beam_tiles_cap(nb) (the rule is
// monotone in the candidate count); block g uses the first tpb[b_g] of its
// slots.  Slots [L'_g, beam) of a block's beams are never read later, because
// L_g of the next step is L'_g.
struct BeamWs {
  Region loc_s, scale_s, lognorm, beams, tiles, sel;
  size_t total;
};
inline BeamWs beam_ws(int64_t nb, int64_t total_dims, int n_steps, int beam) {
  BeamWs l;
  Arena a;
  l.loc_s = a.take((size_t)total_dims * 4);
  l.scale_s = a.take((size_t)total_dims * 4);
  l.lognorm = a.take((size_t)total_dims * 4);
  l.beams = a.take((size_t)2 * beam * total_dims * 4);
  l.tiles = a.take((size_t)nb * beam_tiles_cap(nb) * beam * 8);
  l.sel = a.take((size_t)nb * n_steps * beam * 8);
  l.total = a.o;
  return l;
}

// ---- backfitting (cwq_backfit.hip) --------------------------------
// The encoder's layout for the shape, then
//   rows  [n_steps][total_dims] f32: the selected row of every step
//   value [nb] f32: v, the value of the block's decoded sample
//   count [nb] i32: the replacements accepted so far
// cwq_greedy_backfit_workspace_size does not know the blocks' form and answers
// for ragged ones (csr), which no uniform layout of the same blocks exceeds.
struct BackfitWs {
  EncWs enc;
  Region rows, value, count;
  size_t total;
};
inline BackfitWs backfit_ws(bool csr, int64_t nb, int64_t total_dims, int64_t max_block_dim,
                            int n_steps) {
  BackfitWs l;
  l.enc = csr ? enc_ws_csr(nb, total_dims, max_block_dim) : enc_ws_uniform(nb, max_block_dim);
  Arena a{l.enc.total};
  l.rows = a.take((size_t)n_steps * total_dims * 4);
  l.value = a.take((size_t)nb * 4);
  l.count = a.take((size_t)nb * 4);
  l.total = a.o;
  return l;
}

// ---- backfitting under per-block budgets (cwq_greedy_backfit_var) --
// The budget call's layout for the shape (var_csr_ws, or var_ws at n_steps = 1),
// then backfit's rows, value and count, all over the sorted blocks.  What the
// call uses of the budget layout:
//   t_loc .. p_scale  the sorted inputs, live through the sweeps
//   sample            the vector the scoring launches carry; the sorted result
//   table             the sorted copy of the caller's table, refined in place:
//                     ragged blocks take the budget call's `stage`; uniform
//                     blocks a region of their own behind that layout (its
//                     stage lies on the sorted inputs, which stay live here)
//   bad               one word right behind the 32 bucket counts: the table's
//                     entries outside [0, 2^n_bits[g]) (uniform blocks: the host
//                     reads the 33 words in one copy)
//   enc               every bucket's scoring launches (enc_ws_* is monotone);
//                     keys, loc_s, scale_s and lognorm are the call's, shared
// Regions the blocks' form does not have are empty.  Totals, which include/cwq.h
// states in terms of the size functions:
//   ragged   var_csr_ws(nb, D, maxd, n_steps) + backfit_ws(csr, nb, D, maxd, n_steps)
//            - enc_ws_csr(nb, D, maxd)
//   uniform  var_ws(nb, d, 1) + up(4 nb n_steps) + the same difference at
//            (nb, nb d, d, n_steps)
struct BackfitVarWs {
  SortedWs s;
  Region bad, table, enc, rows, value, count;
  size_t total;
  bool csr;
  EncWs encl;  // the arrays inside `enc` (offsets relative to it)
};
inline BackfitVarWs backfit_var_ws(bool csr, int64_t nb, int64_t total_dims, int64_t max_block_dim,
                                   int n_steps) {
  BackfitVarWs l{};
  l.csr = csr;
  const size_t n = (size_t)nb;
  const VarWs v = csr ? var_csr_ws(nb, total_dims, max_block_dim, n_steps)
                      : var_ws(nb, max_block_dim, 1);
  l.s = v.s, l.enc = v.enc;
  l.encl = csr ? enc_ws_csr(nb, total_dims, max_block_dim) : enc_ws_uniform(nb, max_block_dim);
  Arena a{v.total};
  l.table = csr ? v.stage : a.take(n * (size_t)n_steps * 4);
  l.bad = Region{l.s.counts.off + l.s.counts.bytes, 4};  // in the counts' rounding room
  l.rows = a.take((size_t)n_steps * total_dims * 4);
  l.value = a.take(n * 4);
  l.count = a.take(n * 4);
  l.total = a.o;
  return l;
}

// ---- rate tables (cwq_rate_table, cwq_ratetable.hip) --------------
//   enc     the encoder's layout for the shape (uniform blocks: with the deferral
//           regions behind it); its loc_s, scale_s and lognorm serve the levels
//           launch too, and every budget above kRateMaxLevel runs its
//           launch_encode in it
//   lkeys   [nb][kRateLevels] u64: the best key of every level of rows
//   hkeys   [B - kRateMaxLevel][nb] u64: the argmax keys of budgets 12 .. B, a
//           column per budget (none for B <= kRateMaxLevel)
//   sample  [total_dims] f32, idx [nb] i32: what launch_encode writes besides
//           its keys; nobody reads them
// cwq_rate_table_workspace_bytes does not know the blocks' form and answers
// for ragged ones, which no uniform layout of the same blocks exceeds.
struct RateWs {
  Region enc, lkeys, hkeys, sample, idx;
  size_t total;
  EncWs encl;  // the arrays inside `enc`
};
inline RateWs rate_ws(bool csr, int64_t nb, int64_t total_dims, int64_t max_block_dim,
                      int max_bits) {
  RateWs l{};
  Arena a;
  const size_t n = (size_t)nb;
  const int high = max_bits > kRateMaxLevel ? max_bits - kRateMaxLevel : 0;
  l.encl = csr ? enc_ws_csr(nb, total_dims, max_block_dim) : enc_ws_uniform(nb, max_block_dim);
  l.enc = a.take(csr ? l.encl.total : defer_ws(l.encl.total, nb, max_block_dim).total);
  l.lkeys = a.take(n * kRateLevels * 8);
  l.hkeys = a.take(n * (size_t)high * 8);
  l.sample = a.take((size_t)total_dims * 4);
  l.idx = a.take(high ? n * 4 : 0);
  l.total = a.o;
  return l;
}

// ---- budgets under a total (cwq_choose_bits_total) ------------------
//   state   one SolveState (cwq_rate_solve.h)
//   prod    [B + 1][kSolveSlots] f64: mid_k * b of the current tree's nodes
//   totals  [kSolveSlots] i64: total(mid_k) of the current tree's nodes
// The size depends on the table's B alone.
struct SolveWs {
  Region state, prod, totals;
  size_t total;
};
inline SolveWs solve_ws(size_t base, int max_bits_table) {
  SolveWs l;
  Arena a{Arena::up(base)};
  l.state = a.take(sizeof(SolveState));
  l.prod = a.take((size_t)(max_bits_table + 1) * kSolveSlots * 8);
  l.totals = a.take((size_t)kSolveSlots * 8);
  l.total = a.o;
  return l;
}

// ---- a code under a total from the distributions (cwq_greedy_encode_rate, 4k) ------
// The rate table's layout for the shape, then the table itself and the solver's:
//   rate    cwq_rate_table's workspace (rate_ws; sized for ragged blocks, as
//           cwq_rate_table_workspace_bytes is)
//   tidx    [nb][B + 1] i32: the table's indices, which the gather reads
//   tvalue  [nb][B + 1] f32: its values, when the caller does not ask for them
//   solve   cwq_choose_bits_total's workspace (offsets from the call's base)
struct EncRateWs {
  Region rate, tidx, tvalue;
  SolveWs solve;
  size_t total;
};
inline EncRateWs enc_rate_ws(int64_t nb, int64_t total_dims, int64_t max_block_dim, int max_bits) {
  EncRateWs l;
  Arena a;
  const size_t cells = (size_t)nb * (size_t)(max_bits + 1);
  l.rate = a.take(rate_ws(true, nb, total_dims, max_block_dim, max_bits).total);
  l.tidx = a.take(cells * 4);
  l.tvalue = a.take(cells * 4);
  l.solve = solve_ws(a.o, max_bits);
  l.total = l.solve.total;
  return l;
}

}  // namespace cwq
