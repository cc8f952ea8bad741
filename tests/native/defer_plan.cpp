// Host run of the deferral layout (csrc/cwq_workspace.h defer_ws) for
// tests/test_defer_plan.py.  Test-only; not part of the product.
//
//   defer_plan layout NB D        "name off bytes" per region, "enc N", "total N"
//   defer_plan slots NB           "g q index" for the first, a middle and the last block
//   defer_plan words Q            "c word" for c = 0 .. kDeferSlots + 2
//   defer_plan consts             "slots N", "q N"
//   defer_plan walk               every region of a list of shapes written and
//                                 read back in a heap buffer of exactly `total`
//                                 bytes (the sanitizer build's run); prints "ok"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../compression_without_quantization_amd/csrc/cwq_dispatch.h"
#include "../../compression_without_quantization_amd/csrc/cwq_workspace.h"

using namespace cwq;

static void layout(int64_t nb, int64_t d) {
  const EncWs e = enc_ws_uniform(nb, d);
  const DeferWs l = defer_ws_uniform(nb, d);
  printf("enc %zu\n", e.total);
  printf("surv %zu %zu\ncount %zu %zu\ndlist %zu %zu\ndcount %zu %zu\n", l.surv.off, l.surv.bytes,
         l.count.off, l.count.bytes, l.dlist.off, l.dlist.bytes, l.dcount.off, l.dcount.bytes);
  printf("total %zu\n", l.total);
}

static int walk() {
  const int64_t shapes[][2] = {{1, 8}, {3, 16}, {7, 32}, {70, 64}, {1000, 32}, {5, 9}, {0, 32}};
  for (const auto& s : shapes) {
    const int64_t nb = s[0], d = s[1];
    const DeferWs l = defer_ws_uniform(nb, d);
    std::vector<unsigned char> heap(l.total ? l.total : 1);
    void* w = heap.data();
    const Region* rs[4] = {&l.surv, &l.count, &l.dlist, &l.dcount};
    for (int i = 0; i < 4; ++i) memset(at<unsigned char>(w, *rs[i]), i + 1, rs[i]->bytes);
    if (l.surv.bytes) {
      uint32_t* surv = at<uint32_t>(w, l.surv);
      for (int64_t g = 0; g < nb; ++g)
        for (int q = 0; q < kDeferSlots; ++q) surv[defer_slot(g, q)] = (uint32_t)(g * 7 + q);
      for (int64_t g = 0; g < nb; ++g)
        for (int q = 0; q < kDeferSlots; ++q)
          if (surv[defer_slot(g, q)] != (uint32_t)(g * 7 + q)) return 1;
      at<uint32_t>(w, l.count)[nb - 1] = 1u;
      at<uint32_t>(w, l.dlist)[nb - 1] = 2u;
      *at<uint32_t>(w, l.dcount) = 3u;
    }
  }
  printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "layout") && argc == 4) {
    layout(atoll(argv[2]), atoll(argv[3]));
  } else if (!strcmp(argv[1], "slots") && argc == 3) {
    const int64_t nb = atoll(argv[2]);
    const int64_t gs[3] = {0, nb / 2, nb - 1};
    for (int64_t g : gs)
      for (int q = 0; q < kDeferSlots; ++q)
        printf("%lld %d %zu\n", (long long)g, q, defer_slot(g, q));
  } else if (!strcmp(argv[1], "words") && argc == 3) {
    const int Q = atoi(argv[2]);
    for (uint32_t c = 0; c <= (uint32_t)kDeferSlots + 2; ++c)
      printf("%u %u\n", c, defer_count_word(c, Q));
  } else if (!strcmp(argv[1], "consts")) {
    printf("slots %d\nq %d\n", kDeferSlots, kDeferQ);
  } else if (!strcmp(argv[1], "walk")) {
    return walk();
  } else {
    return 2;
  }
  return 0;
}
