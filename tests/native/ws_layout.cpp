// Host build of the workspace layouts (csrc/cwq_workspace.h) for
// tests/test_workspace_layout.py.  Test-only shim; not part of the product.
//
// wsl_dump writes one layout as text: "name off bytes" per region, then
// "total N".  A layout is a run of Regions up to its total, so its regions are
// read as an array and only their names are spelled here, in member order:
//   name         a region of its own: starts at a multiple of 256
//   name!        packed: starts right behind the one before it
//   name@parent  packed inside `parent`, whose bytes cover it
//   name~target  an alias: lies on `target` (dead by then) on purpose
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../compression_without_quantization_amd/csrc/cwq_dispatch.h"
#include "../../compression_without_quantization_amd/csrc/cwq_workspace.h"

namespace {
using namespace cwq;

struct Out {
  char* p;
  int cap, n;
  bool ok;
  void line(const char* name, int len, size_t a, size_t b, bool two) {
    if (!ok) return;
    const int w = two ? snprintf(p + n, cap - n, "%.*s %zu %zu\n", len, name, a, b)
                      : snprintf(p + n, cap - n, "%.*s %zu\n", len, name, a);
    if (w < 0 || w >= cap - n) ok = false; else n += w;
  }
};

// regions [first, end) under the space-separated names (one per region)
void regions(Out& o, const Region* first, const void* end, const char* names) {
  const Region* last = (const Region*)end;
  for (const Region* r = first; r < last; ++r) {
    while (*names == ' ') ++names;
    const char* e = strchr(names, ' ');
    const int len = e ? (int)(e - names) : (int)strlen(names);
    if (len == 0) o.ok = false;  // fewer names than regions
    o.line(names, len, r->off, r->bytes, true);
    names += len;
  }
  while (*names == ' ') ++names;
  if (*names) o.ok = false;  // more names than regions
}
void total(Out& o, size_t t) { o.line("total", 5, t, 0, false); }

const char* kEnc = "keys tq loc_s scale_s lognorm slist sab cdim bpre ordu grp gtau sdmap abp";
const char* kXfer = "out@res idx@res res kl@d2h tsamp@d2h keep@d2h d2h plan item_off@items "
                    "seed1@items items";
const char* kGrouped = "t_loc t_scale kl zeros ones sample out offs idx part pinfo enc";
}  // namespace

extern "C" {

// Returns the text's length, -1 for an unknown layout, -2 when cap is too small
// or the names above do not match the struct.
int wsl_dump(const char* what, const int64_t* v, char* out, int cap) {
  Out o{out, cap, 0, true};
  auto is = [&](const char* s) { return strcmp(what, s) == 0; };
  if (is("enc_csr") || is("enc_uniform")) {
    const EncWs l = is("enc_csr") ? enc_ws_csr(v[0], v[1], v[2]) : enc_ws_uniform(v[0], v[1]);
    regions(o, &l.keys, &l.total, kEnc);
    total(o, l.total);
  } else if (is("var")) {
    const VarWs l = var_ws(v[0], v[1], v[2]);
    regions(o, &l.s.sorted_in, &l.s.wgfacts,
            "sorted_in t_loc@sorted_in t_scale@sorted_in p_loc@sorted_in p_scale@sorted_in "
            "sample seeds perm hist counts");
    regions(o, &l.enc, &l.total, l.stage_aliases_sorted_in ? "enc stage~sorted_in" : "enc stage");
    total(o, l.total);
  } else if (is("pack")) {
    const PackWs l = pack_ws(v[0]);
    regions(o, &l.off, &l.total, "off partial flag");
    total(o, l.total);
  } else if (is("var_csr")) {
    const VarWs l = var_csr_ws(v[0], v[1], v[2], v[3]);
    regions(o, &l.s.t_loc, &l.enc,
            "t_loc t_scale p_loc p_scale sample seeds perm hist counts wgfacts facts soff roff src "
            "partial");
    regions(o, &l.enc, &l.total, "enc stage");
    total(o, l.total);
  } else if (is("part") || is("part_debug")) {
    const PartDebugWs l = part_debug_ws(v[0]);
    regions(o, &l.part.nxt, &l.part.total, "nxt exg! node! gnode! conv! cnt! sup! spare!");
    if (is("part_debug")) regions(o, &l.info, &l.total, "info");
    total(o, is("part") ? l.part.total : l.total);
  } else if (is("grouped")) {
    const GroupedWs l = grouped_ws(v[0], (int)v[1], v[2]);
    regions(o, &l.t_loc, &l.total, kGrouped);
    total(o, l.total);
  } else if (is("batch")) {
    const BatchWs l = batch_ws(v[0], v[1], (int)v[2]);
    regions(o, &l.g.t_loc, &l.g.total, kGrouped);
    regions(o, &l.seeds, &l.total, "seeds ioff dstarts iinfo itab pstarts");
    total(o, l.total);
  } else if (is("batch_host")) {
    const BatchHostWs l = batch_host_ws(v[0], v[1], (int)v[2]);
    regions(o, &l.kl, &l.total, "kl offs seeds idx");
    total(o, l.total);
  } else if (is("imp")) {
    const ImpWs l = imp_ws(v[0], v[1]);
    regions(o, &l.keys, &l.total, "keys tprefix lnt lnp gtau next_tile cpt!");
    total(o, l.total);
  } else if (is("grouped_imp")) {
    const GroupedImpWs l = grouped_imp_ws(v[0], v[1]);
    regions(o, &l.t_loc, &l.x, "t_loc t_scale zeros ones sample");
    regions(o, &l.x.out, &l.enc, kXfer);
    regions(o, &l.enc, &l.total, "enc");
    total(o, l.total);
  } else if (is("grouped_imp_host")) {
    const GroupedImpHostWs l = grouped_imp_host_ws(v[0], v[1]);
    regions(o, &l.x.out, &l.nst, kXfer);
    regions(o, &l.nst, &l.total, "nst");
    total(o, l.total);
  } else if (is("dec_plan") || is("dec")) {
    const bool plan = is("dec_plan");
    const DecWs l = plan ? DecWs{dec_plan(v[0], v[1] != 0, (size_t)v[2]), {0, 0}, 0}
                         : dec_ws(v[0], v[1], v[2] != 0, (size_t)v[3]);
    regions(o, &l.plan.off, &l.plan.total, "off slot seeds idx");
    if (!plan) regions(o, &l.out, &l.total, "out");
    total(o, plan ? l.plan.total : l.total);
  } else if (is("beam")) {
    const BeamWs l = beam_ws(v[0], v[1], (int)v[2], (int)v[3]);
    regions(o, &l.loc_s, &l.total, "loc_s scale_s lognorm beams tiles sel");
    total(o, l.total);
  } else if (is("backfit")) {
    const BackfitWs l = backfit_ws(v[0] != 0, v[1], v[2], v[3], (int)v[4]);
    regions(o, &l.enc.keys, &l.enc.total, kEnc);
    regions(o, &l.rows, &l.total, "rows value count");
    total(o, l.total);
  } else {
    return -1;
  }
  return o.ok ? o.n : -2;
}

// imp_plan(plan, G, seeds) of a plan region {off, bytes}: out = counts.off,
// offs.off, seeds.off, the end of the seeds, copy_bytes
void wsl_imp_plan(int64_t off, int64_t bytes, int64_t G, int seeds, int64_t* out) {
  const ImpPlan p = imp_plan(Region{(size_t)off, (size_t)bytes}, G, seeds != 0);
  out[0] = (int64_t)p.counts.off;
  out[1] = (int64_t)p.offs.off;
  out[2] = (int64_t)p.seeds.off;
  out[3] = (int64_t)(p.seeds.off + p.seeds.bytes);
  out[4] = (int64_t)p.copy_bytes;
}
}
