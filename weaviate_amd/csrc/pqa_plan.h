// pqa_plan.h -- the host planner of a multi-allow batch (per-query allow lists
// in one call: pqa_exec, runtime.hip).  Host-only, no
// HIP, no wv_index: tools/pqa_plan_print.cpp and tests/test_pqa_plan.py compile
// it alone.
//
// From the batch's sizes and the index's switches to a list of steps: which
// rows share a block-key (or quantized) launch and with which select depths,
// and which rows are searched grouped by identical list (one plain batch call
// per distinct list).  The rules, in the order they apply to a batch of n rows:
//   shared   n > 1 and the route serves min(n, qmax_ids) queries (rq-8 / rq-1:
//            round_up(min(n, qmax_ids), 256) <= quant_max); else all grouped.
//   depths   keyed route only, over the batch that is launched: tot = sum of
//            the list sizes (npresent for an unlisted row), U = max(1,
//            min(tot, npresent)); an unlisted row k + 1, a listed row
//            2 (k + 1) max(1, U / max(1, size)); m = min(960, ceil(depth)),
//            R = 16 when any m > 448, else 8.  Not keyed: m = 0, R = 8.
//   split    keyed, no per-query keys, not inside a split: the rows deeper
//            than 960 (sp) are grouped when 0 < |sp| <= split_max and
//            |sp| < n; the rest is planned as its own batch, never split again.
//   budget   more than qmax_ids rows: consecutive runs of qmax_ids, each
//            planned as a fresh batch (its own split unless inside one).
//   bitmaps  (qmax_bits > 0) shared, n <= qmax_bits and no split: one launch
//            filled from the bitmaps; else via_lists and the id-list plan.
// The rows a keyed launch flags are a run-time outcome the plan does not hold.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

struct PqaRoute {       // what the index offers, read once under its lock
    bool shared;        // pqa on, dims / k / npresent fine, and some route shares a launch
    bool keyed;         // the uncompressed block-key route: depths, split and flags apply
    bool own_keys;      // per-query masked keys (pqa_keys_route): no split
    int64_t quant_max;  // most queries a quantized shared launch takes (rq one-chunk rule;
                        // INT64_MAX for BQ); unused when keyed
};
struct PqaStep {
    bool launch;             // one shared launch; false: grouped by identical list
    std::vector<int64_t> q;  // batch rows, ascending
    std::vector<int32_t> m;  // per row of q: the select's threshold depth (launch only)
    int R;                   // 64 (R - 1)-block candidate lists (launch only)
};
struct PqaPlan {
    std::vector<PqaStep> steps;
    bool via_lists = false;  // a bitmap form whose launches are filled from id lists
};

struct PqaPlanner {
    int k;
    int64_t npresent, qmax_ids, split_max;
    const int32_t* modes;
    const int64_t* sizes;
    PqaRoute r;
    PqaPlan plan;

    bool shared(int64_t n) const {
        if (!r.shared || n <= 1) return false;
        if (r.keyed) return true;
        const int64_t g = std::min(n, qmax_ids);
        return (g + 255) / 256 * 256 <= r.quant_max;
    }
    void depths(const std::vector<int64_t>& q, std::vector<double>& md) const {
        md.assign(q.size(), 0.0);
        if (!r.keyed) return;
        int64_t tot = 0;
        for (int64_t x : q) tot += modes[x] ? sizes[x] : npresent;
        const double U = (double)std::max<int64_t>(1, std::min(tot, npresent));
        for (size_t i = 0; i < q.size(); i++)
            md[i] = modes[q[i]] ? 2.0 * (k + 1) * std::max(1.0, U / (double)std::max<int64_t>(1, sizes[q[i]]))
                                : (double)(k + 1);
    }
    // the rows too sparse for the union's keys, when they are split off
    bool split(const std::vector<int64_t>& q, const std::vector<double>& md, std::vector<int64_t>& sp,
               std::vector<int64_t>& dn) const {
        sp.clear();
        dn.clear();
        if (!r.keyed || r.own_keys) return false;
        for (size_t i = 0; i < q.size(); i++) (md[i] > 960.0 ? sp : dn).push_back(q[i]);
        return !sp.empty() && (int64_t)sp.size() <= split_max && !dn.empty();
    }
    void grouped(const std::vector<int64_t>& q) { plan.steps.push_back(PqaStep{false, q, {}, 0}); }
    void launch(const std::vector<int64_t>& q, const std::vector<double>& md) {
        PqaStep st{true, q, std::vector<int32_t>(q.size()), 8};
        for (size_t i = 0; i < q.size(); i++) st.m[i] = (int32_t)std::min(960.0, std::ceil(md[i]));
        if (*std::max_element(st.m.begin(), st.m.end()) > 448) st.R = 16;  // 960-block lists (k_blk_exact<16>)
        plan.steps.push_back(std::move(st));
    }
    void batch(const std::vector<int64_t>& q, bool in_split) {
        const int64_t n = (int64_t)q.size();
        if (n == 0) return;
        if (!shared(n)) return grouped(q);
        std::vector<double> md;
        std::vector<int64_t> sp, dn;
        depths(q, md);
        if (!in_split && split(q, md, sp, dn)) {
            grouped(sp);
            return batch(dn, true);
        }
        if (n > qmax_ids) {
            for (int64_t i = 0; i < n; i += qmax_ids)
                batch(std::vector<int64_t>(q.begin() + i, q.begin() + std::min(n, i + qmax_ids)), in_split);
            return;
        }
        launch(q, md);
    }
};

// sizes[q]: the list size of a listed row (modes[q] == 1; ignored otherwise).
// qmax_ids / qmax_bits: the rows one launch takes when its bitmaps are built
// from id lists / from the caller's bitmaps (0: the id-list form).
inline PqaPlan pqa_plan(int64_t nq, int k, int64_t npresent, const int32_t* modes, const int64_t* sizes,
                        int64_t qmax_ids, int64_t qmax_bits, int64_t split_max, const PqaRoute& r) {
    PqaPlanner p{k, npresent, std::max<int64_t>(qmax_ids, 1), split_max, modes, sizes, r, {}};
    std::vector<int64_t> all((size_t)std::max<int64_t>(nq, 0));
    for (size_t i = 0; i < all.size(); i++) all[i] = (int64_t)i;
    if (qmax_bits > 0) {
        std::vector<double> md;
        std::vector<int64_t> sp, dn;
        p.depths(all, md);
        if (p.shared(nq) && nq <= qmax_bits && !p.split(all, md, sp, dn)) {
            p.launch(all, md);
            return p.plan;
        }
        p.plan.via_lists = true;
    }
    p.batch(all, false);
    return p.plan;
}
