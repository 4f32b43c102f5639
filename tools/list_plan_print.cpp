// list_plan_print: prints list_plan (weaviate_amd/csrc/list_plan.h) for one
// batch read from stdin (tests/test_list_plan.py):
//   id_base hiwater budget cpw nq
//   then per query: mode n id_0 .. id_{n-1}       (mode 0: no list)
//   a query line "2 r" reuses the caller range of query r (one shared list)
// Output:
//   pool <slots...>
//   q <row> <pool_begin> <len> <e_begin>          per listed query
//   p <listed query> <first> <count>              per piece
//   g <lq0> <lq1> <piece0> <piece1> <entries>     per group
//   s <scanned> <sorted> <shared> <max_entries>
#include <cstdio>
#include <vector>

#include "../weaviate_amd/csrc/list_plan.h"

int main() {
    unsigned long long id_base;
    long long hiwater, budget, cpw, nq;
    if (std::scanf("%llu %lld %lld %lld %lld", &id_base, &hiwater, &budget, &cpw, &nq) != 5) return 2;
    std::vector<uint64_t> ids;
    std::vector<int64_t> lo((size_t)nq), hi((size_t)nq);
    for (long long q = 0; q < nq; q++) {
        long long mode, n;
        if (std::scanf("%lld %lld", &mode, &n) != 2) return 2;
        if (mode == 0) { lo[(size_t)q] = hi[(size_t)q] = -1; continue; }
        if (mode == 2) {
            if (n < 0 || n >= q) return 2;
            lo[(size_t)q] = lo[(size_t)n];
            hi[(size_t)q] = hi[(size_t)n];
            continue;
        }
        lo[(size_t)q] = (int64_t)ids.size();
        for (long long i = 0; i < n; i++) {
            unsigned long long v;
            if (std::scanf("%llu", &v) != 1) return 2;
            ids.push_back(v);
        }
        hi[(size_t)q] = (int64_t)ids.size();
    }
    ids.push_back(0);  // never read: data() of an empty batch stays valid
    const ListPlan p = list_plan(ids.data(), lo.data(), hi.data(), nq, id_base, hiwater, budget, (int)cpw);
    std::printf("pool");
    for (uint32_t s : p.pool) std::printf(" %u", s);
    std::printf("\n");
    for (const ListQuery& q : p.queries)
        std::printf("q %lld %lld %lld %lld\n", (long long)q.q, (long long)q.pool_begin, (long long)q.len, (long long)q.e_begin);
    for (const ListPiece& x : p.pieces) std::printf("p %d %lld %d\n", x.lq, (long long)x.first, x.count);
    for (const ListGroup& g : p.groups)
        std::printf("g %lld %lld %lld %lld %lld\n", (long long)g.lq0, (long long)g.lq1, (long long)g.piece0,
                    (long long)g.piece1, (long long)g.entries);
    std::printf("s %lld %lld %lld %lld\n", (long long)p.scanned, (long long)p.sorted, (long long)p.shared,
                (long long)p.max_entries);
    return 0;
}
