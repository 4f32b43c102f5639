// list_plan.h -- the host planner of the list-order hnsw flat search
// (search_hnsw_lists, list_kernels.hip).  Host-only, no HIP:
// tools/list_plan_print.cpp and tests/test_list_plan.py compile it alone.
//
// Every listed query brings an allow list of doc ids as the caller has it:
// unsorted, with duplicates, with ids below id_base or at / past id_base +
// hiwater (the reference's `candidate >= nodeSize` skip, flat_search.go).  The
// plan holds
//   pool     uint32 slots (id - id_base); each list's range ascending, distinct
//            and within [0, hiwater).  A strictly ascending list (what a roaring
//            iterator yields) is detected in the pass that copies it and is not
//            sorted; lists with identical normalised content are stored once.
//   queries  per listed query: its pool range, its batch row and e_begin, the
//            first entry of its distances in its launch group's compact buffers
//            (a multiple of LIST_CHUNK: chunk minima and absent words never
//            straddle two queries).
//   pieces   the distance kernel's work table: (listed query, first entry,
//            entry count), at most `cpw` chunks of LIST_CHUNK entries each.
//   groups   consecutive listed queries whose padded entries fit `budget`; a
//            group always holds at least one query, so a list longer than the
//            budget gets a group to itself.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

constexpr int LIST_CHUNK = 256;  // entries per chunk = threads per workgroup of k_list_dist

struct ListQuery {       // device record (32 bytes)
    int64_t pool_begin;  // first slot of the list in the pool
    int64_t e_begin;     // first entry in the group's compact buffers
    int64_t len;         // list entries
    int64_t q;           // batch row
};
struct ListPiece {  // device record (16 bytes)
    int32_t lq;     // listed query (index into queries)
    int32_t count;  // entries of this piece
    int64_t first;  // its first entry within the list (a multiple of LIST_CHUNK)
};
struct ListGroup {
    int64_t lq0, lq1;        // listed queries [lq0, lq1)
    int64_t piece0, piece1;  // pieces [piece0, piece1)
    int64_t entries;         // compact-buffer entries (every list padded to whole chunks)
};
struct ListPlan {
    std::vector<uint32_t> pool;
    std::vector<ListQuery> queries;
    std::vector<ListPiece> pieces;
    std::vector<ListGroup> groups;
    int64_t scanned = 0;     // sum of the lists' lengths: the (query, row) pairs the launch computes
    int64_t sorted = 0;      // lists that were not ascending and went through the sort
    int64_t shared = 0;      // lists stored as another query's range
    int64_t max_entries = 0; // the largest group's entries (buffer size)
};

// query q's list is ids[lo[q] .. hi[q]); lo[q] < 0: the query has no list (it
// is not part of the plan)
inline ListPlan list_plan(const uint64_t* ids, const int64_t* lo, const int64_t* hi, int64_t nq, uint64_t id_base,
                          int64_t hiwater, int64_t budget, int cpw) {
    ListPlan p;
    if (budget < 1) budget = 1;
    if (cpw < 1) cpw = 1;
    const uint64_t hw = hiwater > 0 ? (uint64_t)hiwater : 0;
    std::unordered_map<uint64_t, std::vector<int64_t>> by_range, by_content;
    int64_t total = 0;  // an upper bound of the pool: no reallocation while the lists are copied
    for (int64_t q = 0; q < nq; q++)
        if (lo[q] >= 0 && hi[q] > lo[q] && !(q > 0 && lo[q] == lo[q - 1] && hi[q] == hi[q - 1])) total += hi[q] - lo[q];
    p.pool.reserve((size_t)total);
    for (int64_t q = 0; q < nq; q++) {
        if (lo[q] < 0) continue;
        const int64_t a = lo[q], b = std::max(hi[q], lo[q]);
        ListQuery lq{0, 0, 0, q};
        bool done = false;
        // the same caller range as an earlier query (one list for the whole batch)
        const uint64_t rkey = (uint64_t)a * 0x9E3779B97F4A7C15ull ^ (uint64_t)b;
        for (int64_t o : by_range[rkey])
            if (lo[p.queries[(size_t)o].q] == a && std::max(hi[p.queries[(size_t)o].q], a) == b) {
                lq.pool_begin = p.queries[(size_t)o].pool_begin;
                lq.len = p.queries[(size_t)o].len;
                done = true;
                break;
            }
        if (!done) {
            const size_t at = p.pool.size();
            bool asc = true;
            uint64_t prev = 0;
            for (int64_t i = a; i < b; i++) {
                const uint64_t id = ids[i];
                if (i > a && id <= prev) { asc = false; break; }
                prev = id;
                if (id >= id_base && id - id_base < hw) p.pool.push_back((uint32_t)(id - id_base));
            }
            if (!asc) {
                p.pool.resize(at);
                for (int64_t i = a; i < b; i++)
                    if (ids[i] >= id_base && ids[i] - id_base < hw) p.pool.push_back((uint32_t)(ids[i] - id_base));
                std::sort(p.pool.begin() + (std::ptrdiff_t)at, p.pool.end());
                p.pool.erase(std::unique(p.pool.begin() + (std::ptrdiff_t)at, p.pool.end()), p.pool.end());
                p.sorted++;
            }
            const size_t n = p.pool.size() - at;
            uint64_t h = 0xCBF29CE484222325ull ^ (uint64_t)n;
            for (size_t i = at; i < p.pool.size(); i++) h = (h ^ p.pool[i]) * 0x100000001B3ull;
            lq.pool_begin = (int64_t)at;
            lq.len = (int64_t)n;
            for (int64_t o : by_content[h]) {
                const ListQuery& oq = p.queries[(size_t)o];
                if (oq.len == (int64_t)n &&
                    (n == 0 || std::memcmp(&p.pool[(size_t)oq.pool_begin], &p.pool[at], n * sizeof(uint32_t)) == 0)) {
                    lq.pool_begin = oq.pool_begin;
                    p.pool.resize(at);
                    done = true;
                    break;
                }
            }
            if (!done) by_content[h].push_back((int64_t)p.queries.size());
        }
        if (done) p.shared++;
        by_range[rkey].push_back((int64_t)p.queries.size());
        p.queries.push_back(lq);
        p.scanned += lq.len;
    }
    // launch groups and the work table
    const int64_t per = (int64_t)cpw * LIST_CHUNK;
    ListGroup g{0, 0, 0, 0, 0};
    for (size_t i = 0; i < p.queries.size(); i++) {
        ListQuery& lq = p.queries[i];
        const int64_t padded = (lq.len + LIST_CHUNK - 1) / LIST_CHUNK * LIST_CHUNK;
        if (g.lq1 > g.lq0 && g.entries + padded > budget) {
            p.groups.push_back(g);
            g = ListGroup{(int64_t)i, (int64_t)i, (int64_t)p.pieces.size(), (int64_t)p.pieces.size(), 0};
        }
        lq.e_begin = g.entries;
        g.entries += padded;
        g.lq1 = (int64_t)i + 1;
        for (int64_t f = 0; f < lq.len; f += per)
            p.pieces.push_back(ListPiece{(int32_t)i, (int32_t)std::min<int64_t>(per, lq.len - f), f});
        g.piece1 = (int64_t)p.pieces.size();
    }
    if (g.lq1 > g.lq0) p.groups.push_back(g);
    for (const ListGroup& x : p.groups) p.max_entries = std::max(p.max_entries, x.entries);
    return p;
}
