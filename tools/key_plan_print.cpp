// key_plan_print: prints key_plan (weaviate_amd/csrc/key_plan.h) for rows of
// "nqg nslots RB row_bytes spans whole_rounds" read from stdin, one
// "slots_per_span nspans" line each; with the argument "ring", ring_span_plan
// for rows of "nqg nblk", one "blocks_per_span nspans" line each
// (tests/test_key_plan.py).
#include <cstdio>
#include <cstring>

#include "../weaviate_amd/csrc/key_plan.h"

int main(int argc, char** argv) {
    long long nqg, nslots, rb, row_bytes, spans, whole;
    if (argc > 1 && !std::strcmp(argv[1], "ring")) {
        while (std::scanf("%lld %lld", &nqg, &nslots) == 2) {
            const RingSpanPlan p = ring_span_plan((int)nqg, nslots);
            std::printf("%d %d\n", p.blocks_per_span, p.nspans);
        }
        return 0;
    }
    while (std::scanf("%lld %lld %lld %lld %lld %lld", &nqg, &nslots, &rb, &row_bytes, &spans, &whole) == 6) {
        const KeyPlan p = key_plan((int)nqg, nslots, (int)rb, row_bytes, (int)spans, whole != 0);
        std::printf("%d %d\n", p.slots_per_span, p.nspans);
    }
    return 0;
}
