// key_plan_print: prints key_plan (weaviate_amd/csrc/key_plan.h) for rows of
// "nqg nslots RB row_bytes spans whole_rounds" read from stdin, one
// "slots_per_span nspans" line each (tests/test_key_plan.py).
#include <cstdio>

#include "../weaviate_amd/csrc/key_plan.h"

int main() {
    long long nqg, nslots, rb, row_bytes, spans, whole;
    while (std::scanf("%lld %lld %lld %lld %lld %lld", &nqg, &nslots, &rb, &row_bytes, &spans, &whole) == 6) {
        const KeyPlan p = key_plan((int)nqg, nslots, (int)rb, row_bytes, (int)spans, whole != 0);
        std::printf("%d %d\n", p.slots_per_span, p.nspans);
    }
    return 0;
}
