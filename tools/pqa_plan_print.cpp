// pqa_plan_print: prints pqa_plan (weaviate_amd/csrc/pqa_plan.h) for one
// multi-allow batch read from stdin (tests/test_pqa_plan.py):
//   nq k npresent qmax_ids qmax_bits split_max shared keyed own_keys quant_max
//   then per row: mode size                       (mode 0: no list, size ignored)
//   (quant_max < 0: no limit)
// Output:
//   v <via_lists>
//   l <R> <n> <row_0 .. row_{n-1}> <m_0 .. m_{n-1}>   per launch step
//   g <n> <row_0 .. row_{n-1}>                        per grouped step
#include <cstdio>
#include <vector>

#include "../weaviate_amd/csrc/pqa_plan.h"

int main() {
    long long nq, k, npresent, qmax_ids, qmax_bits, split_max, shared, keyed, own_keys, quant_max;
    if (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &nq, &k, &npresent, &qmax_ids, &qmax_bits,
                   &split_max, &shared, &keyed, &own_keys, &quant_max) != 10 || nq < 0)
        return 2;
    std::vector<int32_t> modes((size_t)nq + 1);
    std::vector<int64_t> sizes((size_t)nq + 1);
    for (long long q = 0; q < nq; q++) {
        long long mode, size;
        if (std::scanf("%lld %lld", &mode, &size) != 2 || (mode != 0 && mode != 1)) return 2;
        modes[(size_t)q] = (int32_t)mode;
        sizes[(size_t)q] = size;
    }
    const PqaRoute r{shared != 0, keyed != 0, own_keys != 0, quant_max < 0 ? INT64_MAX : (int64_t)quant_max};
    const PqaPlan p = pqa_plan(nq, (int)k, npresent, modes.data(), sizes.data(), qmax_ids, qmax_bits, split_max, r);
    std::printf("v %d\n", p.via_lists ? 1 : 0);
    for (const PqaStep& st : p.steps) {
        if (st.launch) std::printf("l %d %zu", st.R, st.q.size());
        else std::printf("g %zu", st.q.size());
        for (int64_t q : st.q) std::printf(" %lld", (long long)q);
        for (int32_t m : st.m) std::printf(" %d", m);
        std::printf("\n");
    }
    return 0;
}
