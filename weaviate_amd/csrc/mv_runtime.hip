// mv_runtime.hip -- the multi-vector (late-interaction) document store and its
// filtered brute-force search, hnsw.flatMultiSearch (hnsw/flat_search.go:143-212;
// DESIGN.md §3.13).  A translation unit of its own: the wv_mv handle shares no
// state with wv_index.
//
// Memory layout in HBM:
//   T        [tok_cap][dpad] fp32  token rows; a document's vectors are
//                                  contiguous rows appended at the tail,
//                                  normalised at add for cosine-dot
//                                  (insert.go:363); dpad = dims rounded up to 32
//   docs     [slot] MvSpan         tok_begin / tok_len, slot = doc id - id_base
//   present  [slots / 32] u32      slots holding a document
// The per-slot records are kept on the host and uploaded before the next search
// after a change.  Delete clears `present`; the rows stay (no compaction).
//
// Search: the host planner (list_plan.h, unchanged) turns every query's allow
// list -- or, without a list, the stored documents in id order -- into
// ascending distinct slots, a work table of one-chunk pieces and launch groups;
// per group k_mv_maxsim / k_mv_simple (mv_kernels.hip) writes the score of every
// (query, listed document) and k_list_heap (list_kernels.hip, unchanged) runs
// the reference's heap with limit k over them in ascending id order.
//
// The key route (mv_keys.hip, DESIGN.md §3.13b, WV_ROUTE_MV_KEYS): queries whose
// lists hold at least mv_keys_min ids first take k_mv_keys over bf16 planes
//   Th, Tl   [tok_cap][dpad] bf16  T = Th + Tl + r, built lazily over the rows
//                                  added since the last key search
//   tnorm    [tok_cap] fp32        row norms;  tmax [slot]: a document's largest
// and k_mv_cut; the candidates then go through the search above with limit
// k + 1, and a query whose k + 1 scores are not pairwise distinct -- or that the
// key pass flagged -- is answered by the search above over its original list.
#include "rt_index.h"
#include "mv_kernels.hip"
#include "mv_keys.hip"

#include <unordered_set>

namespace {

// k_mv_maxsim's instantiations: the AVX2 order (and the AVX-512 order below 128
// elements, where both coincide), and the AVX-512 order from 128 elements on
constexpr int MV_QT = 4, MV_RT = 2;
constexpr int MV_QT5 = 2, MV_RT5 = 2;
constexpr size_t MV_LDS_TILE = 32 * 1024;  // the query is staged whole while it fits
constexpr size_t MV_LDS_MAX = 64 * 1024;   // QT rows must fit, else the simple arm

// the key route's auto rule and its smallest list, from the crossover measured in DESIGN.md §3.13b
constexpr bool MV_KEYS_AUTO = true;
constexpr int64_t MV_KEYS_MIN = 4096;
constexpr size_t MVK_LDS_TILE = 60 * 1024;  // the query tile's hi / lo rows while more than 32 vectors fit

}  // namespace

struct wv_mv {
    std::mutex mu;
    int metric = WV_METRIC_COSINE_DOT;
    int variant = WV_VARIANT_AVX256;
    int device = 0;
    uint64_t id_base = 0;
    int dims = 0, dpad = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float* T = nullptr;
    int64_t tok_cap = 0, tok_used = 0;
    std::vector<MvSpan> h_docs;       // [hiwater]
    std::vector<uint32_t> h_present;  // [ceil(hiwater / 32)]
    int64_t hiwater = 0, ndocs = 0;
    bool meta_dirty = true;
    int mv_tile = -1;           // option mv_tile: -1 auto, 0 k_mv_simple, 1 k_mv_maxsim
    int64_t mv_list_rows = 0;   // option mv_list_rows: entries per launch group (0: 4 Mi)
    int timing = 0;             // option timing: events around the score and heap kernels
    DBuf stage, Q, qspan, dDocs, dPresent, pool, lq, pieces, Ec, Bc, Ab, oI, oD, oN;
    // the key route (mv_keys.hip): nothing below is allocated before its first search
    int mv_keys = -1;           // option mv_keys: -1 auto (MV_KEYS_AUTO), 0 never, 1 wherever eligible
    int64_t mv_keys_min = -1;   // option mv_keys_min: listed ids from which a query takes keys (-1: MV_KEYS_MIN)
    int64_t mv_keys_cap = 0;    // option mv_keys_cap: candidate slots per query (0: max(1024, 8 (k + 1)))
    uint16_t *Th = nullptr, *Tl = nullptr;
    float* tnorm = nullptr;
    int64_t plane_cap = 0, built = 0;  // rows allocated / converted
    bool tmax_valid = false;           // tmax covers every stored document
    hipEvent_t evk0 = nullptr, evk1 = nullptr;
    DBuf tmax, Kc, kAb, cS, kflags, cand, ccnt;
    // the last key search (wv_mv_debug_keys): its plan, every listed query's first entry in Kc / kAb,
    // the queries' c sum |q| and flags
    ListPlan kplan;
    std::vector<int64_t> kabs;
    std::vector<float> h_cS;
    std::vector<int32_t> h_kflags;
    bool kdbg = false;
    wv_mv_stats stats{};
};

namespace {

bool mv_present(const wv_mv* m, uint64_t slot) {
    return slot < (uint64_t)m->hiwater && ((m->h_present[slot >> 5] >> (slot & 31u)) & 1u);
}

int mv_device(wv_mv* m) {
    HIPCHK(hipSetDevice(m->device));
    if (!m->stream) HIPCHK(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    return WV_OK;
}

// the bf16 planes and row norms with room for `cap` rows; the converted rows move with them
int mv_alloc_planes(wv_mv* m, int64_t cap) {
    if (cap <= m->plane_cap) return WV_OK;
    uint16_t *nh = nullptr, *nl = nullptr;
    float* nn = nullptr;
    const size_t pb = (size_t)cap * m->dpad * sizeof(uint16_t), ob = (size_t)m->built * m->dpad * sizeof(uint16_t);
    hipError_t e = hipMalloc(&nh, pb);
    if (e == hipSuccess) e = hipMalloc(&nl, pb);
    if (e == hipSuccess) e = hipMalloc(&nn, (size_t)cap * sizeof(float));
    if (e == hipSuccess && m->built > 0) {
        e = hipMemcpyAsync(nh, m->Th, ob, hipMemcpyDeviceToDevice, m->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nl, m->Tl, ob, hipMemcpyDeviceToDevice, m->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(nn, m->tnorm, (size_t)m->built * sizeof(float), hipMemcpyDeviceToDevice, m->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) {
        if (nh) hipFree(nh);
        if (nl) hipFree(nl);
        if (nn) hipFree(nn);
        return set_err(WV_ERR_HIP, "token planes: %s", hipGetErrorString(e));
    }
    if (m->Th) hipFree(m->Th);
    if (m->Tl) hipFree(m->Tl);
    if (m->tnorm) hipFree(m->tnorm);
    m->Th = nh;
    m->Tl = nl;
    m->tnorm = nn;
    m->plane_cap = cap;
    return WV_OK;
}

// room for `rows` token rows; the rows already stored move with the buffer
int mv_ensure_tokens(wv_mv* m, int64_t rows) {
    if (rows <= m->tok_cap) return WV_OK;
    const int64_t cap = std::max<int64_t>(std::max<int64_t>(rows, m->tok_cap * 2), 1024);
    if (m->Th) {  // the planes grow with T once they exist
        const int rc = mv_alloc_planes(m, cap);
        if (rc) return rc;
    }
    float* nt = nullptr;
    HIPCHK(hipMalloc(&nt, (size_t)cap * m->dpad * sizeof(float)));
    hipError_t e = hipSuccess;
    if (m->tok_used > 0)
        e = hipMemcpyAsync(nt, m->T, (size_t)m->tok_used * m->dpad * sizeof(float), hipMemcpyDeviceToDevice, m->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(nt + m->tok_used * m->dpad, 0, (size_t)(cap - m->tok_used) * m->dpad * sizeof(float), m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) {
        hipFree(nt);
        return set_err(WV_ERR_HIP, "token matrix: %s", hipGetErrorString(e));
    }
    if (m->T) hipFree(m->T);
    m->T = nt;
    m->tok_cap = cap;
    return WV_OK;
}

// rows [n][d] of host vectors -> dst [n][dpad] on the device, normalised for
// cosine-dot (distancer.Normalize: insert.go:363, normalizeVecs index.go:911-920)
int mv_upload_rows(wv_mv* m, const float* rows, int64_t n, float* dst) {
    hipStream_t s = m->stream;
    if (m->metric == WV_METRIC_COSINE_DOT) {
        HIPCHK(m->stage.ensure((size_t)n * m->dims * sizeof(float)));
        HIPCHK(hipMemcpyAsync(m->stage.p, rows, (size_t)n * m->dims * sizeof(float), hipMemcpyHostToDevice, s));
        k_normalize_rows<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(m->stage.as<float>(), n, m->dims, dst, m->dpad);
        HIPCHK(hipGetLastError());
    } else {
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)m->dpad * sizeof(float), rows, (size_t)m->dims * sizeof(float),
                                (size_t)m->dims * sizeof(float), (size_t)n, hipMemcpyHostToDevice, s));
    }
    return WV_OK;
}

int mv_sync_meta(wv_mv* m) {
    if (!m->meta_dirty) return WV_OK;
    const size_t nd = (size_t)m->hiwater, nw = (size_t)((m->hiwater + 31) / 32);
    HIPCHK(m->dDocs.ensure(nd * sizeof(MvSpan)));
    HIPCHK(m->dPresent.ensure(nw * sizeof(uint32_t)));
    if (nd) {
        HIPCHK(hipMemcpyAsync(m->dDocs.p, m->h_docs.data(), nd * sizeof(MvSpan), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->dPresent.p, m->h_present.data(), nw * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    }
    m->meta_dirty = false;
    return WV_OK;
}

// the common checks of a query's vectors (ValidateMultiBeforeInsert's text for the length)
int mv_check_dims(const wv_mv* m, int64_t d) {
    if (d <= 0) return set_err(WV_ERR_INVALID, "multi vector query with vectors of length %lld", (long long)d);
    if (m->dims && d != m->dims)
        return set_err(WV_ERR_VECTOR_LENGTH, "%lld vs %d: vector lengths don't match", (long long)d, m->dims);
    return WV_OK;
}

bool mv_tiled(const wv_mv* m) {
    if (m->mv_tile == 0) return false;
    const bool w512 = m->variant == WV_VARIANT_AVX512 && m->dims >= 128;
    return (size_t)(w512 ? MV_QT5 : MV_QT) * m->dpad * sizeof(float) <= MV_LDS_MAX;
}

// the score kernel of np pieces; max_qv: the longest query of the batch
int mv_launch_scores(wv_mv* m, hipStream_t s, MvArgs a, unsigned np, int64_t max_qv) {
    if (np == 0) return WV_OK;
    const bool w512 = m->variant == WV_VARIANT_AVX512 && m->dims >= 128;
    if (!mv_tiled(m)) {
        if (m->variant == WV_VARIANT_AVX512) k_mv_simple<AVX512><<<np, 256, 0, s>>>(a);
        else k_mv_simple<AVX256><<<np, 256, 0, s>>>(a);
        HIPCHK(hipGetLastError());
        return WV_OK;
    }
    const int qt = w512 ? MV_QT5 : MV_QT;
    const size_t row = (size_t)m->dpad * sizeof(float);
    int64_t tile = std::max<int64_t>((int64_t)(MV_LDS_TILE / row) / qt * qt, qt);
    tile = std::min<int64_t>(tile, round_up(std::max<int64_t>(max_qv, 1), qt));
    a.qtile = (int)tile;
    const size_t lds = (size_t)tile * row;
    if (w512) k_mv_maxsim<AVX512, MV_QT5, MV_RT5><<<np, 256, lds, s>>>(a);
    else k_mv_maxsim<AVX256, MV_QT, MV_RT><<<np, 256, lds, s>>>(a);
    HIPCHK(hipGetLastError());
    return WV_OK;
}

MvArgs mv_args(const wv_mv* m) {
    MvArgs a{};
    a.pool = m->pool.as<uint32_t>();
    a.lq = m->lq.as<ListQuery>();
    a.pieces = m->pieces.as<ListPiece>();
    a.present = m->dPresent.as<uint32_t>();
    a.docs = m->dDocs.as<MvSpan>();
    a.T = m->T;
    a.Q = m->Q.as<float>();
    a.qspan = m->qspan.as<MvSpan>();
    a.Ec = m->Ec.as<float>();
    a.Bc = m->Bc.as<float>();
    a.Ab = m->Ab.as<uint64_t>();
    a.d = m->dims;
    a.dpad = m->dpad;
    return a;
}

int mv_upload_plan(wv_mv* m, const std::vector<uint32_t>& pool, const std::vector<ListQuery>& lq,
                   const std::vector<ListPiece>& pieces, int64_t entries) {
    hipStream_t s = m->stream;
    HIPCHK(m->pool.ensure(pool.size() * sizeof(uint32_t)));
    HIPCHK(m->lq.ensure(lq.size() * sizeof(ListQuery)));
    HIPCHK(m->pieces.ensure(pieces.size() * sizeof(ListPiece)));
    if (!pool.empty()) HIPCHK(hipMemcpyAsync(m->pool.p, pool.data(), pool.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (!lq.empty()) HIPCHK(hipMemcpyAsync(m->lq.p, lq.data(), lq.size() * sizeof(ListQuery), hipMemcpyHostToDevice, s));
    if (!pieces.empty())
        HIPCHK(hipMemcpyAsync(m->pieces.p, pieces.data(), pieces.size() * sizeof(ListPiece), hipMemcpyHostToDevice, s));
    const int64_t me = std::max<int64_t>(entries, LIST_CHUNK);
    HIPCHK(m->Ec.ensure((size_t)me * sizeof(float)));
    HIPCHK(m->Bc.ensure((size_t)(me / LIST_CHUNK) * sizeof(float)));
    HIPCHK(m->Ab.ensure((size_t)(me / 64) * sizeof(uint64_t)));
    return WV_OK;
}

// the query vectors of a call on the device: Q [rows][dpad], qspan by batch row
int mv_upload_queries(wv_mv* m, const float* qvecs, const int64_t* q_offsets, int64_t nq) {
    const int64_t q0 = q_offsets[0], rows = q_offsets[nq] - q0;
    HIPCHK(m->Q.ensure((size_t)rows * m->dpad * sizeof(float)));
    int rc = mv_upload_rows(m, qvecs + q0 * m->dims, rows, m->Q.as<float>());
    if (rc) return rc;
    std::vector<MvSpan> sp((size_t)nq);
    for (int64_t q = 0; q < nq; q++) sp[(size_t)q] = MvSpan{q_offsets[q] - q0, (int32_t)(q_offsets[q + 1] - q_offsets[q]), 0};
    HIPCHK(m->qspan.ensure((size_t)nq * sizeof(MvSpan)));
    HIPCHK(hipMemcpyAsync(m->qspan.p, sp.data(), (size_t)nq * sizeof(MvSpan), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));  // sp and the caller's rows are read
    return WV_OK;
}

// the exact search of the queries with lo[q] >= 0 over their lists ids[lo[q] .. hi[q]) (the uploaded
// queries and records): per launch group the score kernel and the heap with `limit`.  Rows [nq][limit]
// and counts [nq] of those queries into the host arrays; the other queries' rows are not defined.
int mv_exact_search(wv_mv* m, const uint64_t* ids, const int64_t* lo, const int64_t* hi, int64_t nq, int limit,
                    int64_t max_qv, bool count_rows, uint64_t* out_ids, float* out_dists, int32_t* out_counts) {
    hipStream_t s = m->stream;
    const int64_t budget = m->mv_list_rows > 0 ? m->mv_list_rows : (int64_t)4 << 20;
    const ListPlan plan = list_plan(ids, lo, hi, nq, m->id_base, m->hiwater, budget, 1);
    if (count_rows) {
        m->stats.last_scan_rows += (uint64_t)plan.scanned;
        for (const ListQuery& q : plan.queries)
            for (int64_t i = 0; i < q.len; i++) {
                const uint32_t sl = plan.pool[(size_t)(q.pool_begin + i)];
                if (mv_present(m, sl)) m->stats.last_token_rows += (uint64_t)m->h_docs[sl].len;
            }
    }
    int rc = mv_upload_plan(m, plan.pool, plan.queries, plan.pieces, plan.max_entries);
    if (rc) return rc;
    HIPCHK(m->oI.ensure((size_t)nq * limit * sizeof(uint64_t)));
    HIPCHK(m->oD.ensure((size_t)nq * limit * sizeof(float)));
    HIPCHK(m->oN.ensure((size_t)nq * sizeof(int32_t)));
    const size_t lds_h = replay_scan_lds(limit);
    const bool pk = limit <= PACKED_REPLAY_MAX_K;
    HIPCHK(set_dyn_lds(pk ? (const void*)k_list_heap<true> : (const void*)k_list_heap<false>, lds_h));
    if (m->timing && !m->ev0) {
        HIPCHK(hipEventCreate(&m->ev0));
        HIPCHK(hipEventCreate(&m->ev1));
    }
    if (m->timing) HIPCHK(hipEventRecord(m->ev0, s));
    MvArgs a = mv_args(m);
    for (const ListGroup& gr : plan.groups) {
        a.pieces = m->pieces.as<ListPiece>() + gr.piece0;
        rc = mv_launch_scores(m, s, a, (unsigned)(gr.piece1 - gr.piece0), max_qv);
        if (rc) return rc;
        const unsigned nl = (unsigned)(gr.lq1 - gr.lq0);
        if (pk)
            k_list_heap<true><<<nl, 64, lds_h, s>>>(a.Ec, a.Bc, a.Ab, a.pool, a.lq + gr.lq0, (int)nl, limit, m->id_base,
                                                    m->oI.as<uint64_t>(), m->oD.as<float>(), m->oN.as<int32_t>());
        else
            k_list_heap<false><<<nl, 64, lds_h, s>>>(a.Ec, a.Bc, a.Ab, a.pool, a.lq + gr.lq0, (int)nl, limit, m->id_base,
                                                     m->oI.as<uint64_t>(), m->oD.as<float>(), m->oN.as<int32_t>());
        HIPCHK(hipGetLastError());
    }
    if (m->timing) HIPCHK(hipEventRecord(m->ev1, s));
    HIPCHK(hipMemcpyAsync(out_ids, m->oI.p, (size_t)nq * limit * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_dists, m->oD.p, (size_t)nq * limit * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_counts, m->oN.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (m->timing) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, m->ev0, m->ev1);
        m->stats.last_kernel_ms += ms;
    }
    return WV_OK;
}

// the planes of the rows added since the last key search, and every document's largest row norm
int mv_build_planes(wv_mv* m) {
    hipStream_t s = m->stream;
    int rc = mv_alloc_planes(m, m->tok_cap);
    if (rc) return rc;
    if (m->built < m->tok_used) {
        const int64_t rows = m->tok_used - m->built;
        k_mv_planes<<<(unsigned)((rows + 3) / 4), 256, 0, s>>>(m->T, m->built, m->tok_used, m->dims, m->dpad, m->Th, m->Tl,
                                                               m->tnorm);
        HIPCHK(hipGetLastError());
        m->built = m->tok_used;
    }
    if (!m->tmax_valid) {
        HIPCHK(m->tmax.ensure((size_t)m->hiwater * sizeof(float)));
        k_mv_tmax<<<(unsigned)((m->hiwater + 255) / 256), 256, 0, s>>>(m->dDocs.as<MvSpan>(), m->hiwater, m->tnorm,
                                                                       m->tmax.as<float>());
        HIPCHK(hipGetLastError());
        m->tmax_valid = true;
    }
    return WV_OK;
}

int mv_launch_keys(hipStream_t s, const MvKeyArgs& a, unsigned np) {
    if (np == 0) return WV_OK;
    const size_t lds = mvk_lds_bytes(a.qtile, a.dpad);
    const void* fn = a.dpad == 32 ? (const void*)k_mv_keys<2> : a.dpad == 64 ? (const void*)k_mv_keys<4>
                   : a.dpad == 96 ? (const void*)k_mv_keys<6> : a.dpad == 128 ? (const void*)k_mv_keys<8>
                                                                              : (const void*)k_mv_keys<0>;
    HIPCHK(set_dyn_lds(fn, lds));
    if (a.dpad == 32) k_mv_keys<2><<<np, 256, lds, s>>>(a);
    else if (a.dpad == 64) k_mv_keys<4><<<np, 256, lds, s>>>(a);
    else if (a.dpad == 96) k_mv_keys<6><<<np, 256, lds, s>>>(a);
    else if (a.dpad == 128) k_mv_keys<8><<<np, 256, lds, s>>>(a);
    else k_mv_keys<0><<<np, 256, lds, s>>>(a);
    HIPCHK(hipGetLastError());
    return WV_OK;
}

// the key pass of the queries with lo[q] >= 0: keys, cut, one download.  cand[q]: the candidate slots of a
// query the pass did not flag (ascending); flagged[q]: MVK_FLAG_* of one it did.
int mv_key_pass(wv_mv* m, const uint64_t* ids, const int64_t* lo, const int64_t* hi, int64_t nq, int k,
                int64_t max_qv, std::vector<std::vector<uint32_t>>& cand, std::vector<int32_t>& flagged) {
    hipStream_t s = m->stream;
    int rc = mv_build_planes(m);
    if (rc) return rc;
    const int64_t budget = m->mv_list_rows > 0 ? m->mv_list_rows : (int64_t)4 << 20;
    m->kdbg = false;
    m->kplan = list_plan(ids, lo, hi, nq, m->id_base, m->hiwater, budget, 1);
    const ListPlan& plan = m->kplan;
    int64_t total = 0, longest = 1;
    std::vector<int64_t> gbase;
    for (const ListGroup& gr : plan.groups) {
        gbase.push_back(total);
        total += gr.entries;
    }
    m->kabs.assign(plan.queries.size(), 0);
    for (size_t g = 0; g < plan.groups.size(); g++)
        for (int64_t i = plan.groups[g].lq0; i < plan.groups[g].lq1; i++) {
            const ListQuery& q = plan.queries[(size_t)i];
            m->kabs[(size_t)i] = gbase[g] + q.e_begin;
            longest = std::max(longest, q.len);
        }
    const int64_t want = m->mv_keys_cap > 0 ? m->mv_keys_cap : std::max<int64_t>(1024, 8 * ((int64_t)k + 1));
    const int cap = (int)std::min<int64_t>(want, longest);
    HIPCHK(m->pool.ensure(plan.pool.size() * sizeof(uint32_t)));
    HIPCHK(m->lq.ensure(plan.queries.size() * sizeof(ListQuery)));
    HIPCHK(m->pieces.ensure(plan.pieces.size() * sizeof(ListPiece)));
    if (!plan.pool.empty())
        HIPCHK(hipMemcpyAsync(m->pool.p, plan.pool.data(), plan.pool.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (!plan.queries.empty())
        HIPCHK(hipMemcpyAsync(m->lq.p, plan.queries.data(), plan.queries.size() * sizeof(ListQuery), hipMemcpyHostToDevice, s));
    if (!plan.pieces.empty())
        HIPCHK(hipMemcpyAsync(m->pieces.p, plan.pieces.data(), plan.pieces.size() * sizeof(ListPiece), hipMemcpyHostToDevice, s));
    const int64_t me = std::max<int64_t>(total, LIST_CHUNK);
    HIPCHK(m->Kc.ensure((size_t)me * sizeof(float)));
    HIPCHK(m->kAb.ensure((size_t)(me / 64) * sizeof(uint64_t)));
    HIPCHK(m->cS.ensure((size_t)nq * sizeof(float)));
    HIPCHK(m->kflags.ensure((size_t)nq * sizeof(int32_t)));
    HIPCHK(m->cand.ensure((size_t)nq * cap * sizeof(uint32_t)));
    HIPCHK(m->ccnt.ensure((size_t)nq * sizeof(int32_t)));
    if (m->timing && !m->evk0) {
        HIPCHK(hipEventCreate(&m->evk0));
        HIPCHK(hipEventCreate(&m->evk1));
    }
    if (m->timing) HIPCHK(hipEventRecord(m->evk0, s));
    k_mv_qprep<<<(unsigned)nq, 256, 0, s>>>(m->Q.as<float>(), m->qspan.as<MvSpan>(), m->dims, m->dpad, m->cS.as<float>(),
                                            m->kflags.as<int32_t>());
    HIPCHK(hipGetLastError());
    MvKeyArgs a{};
    a.pool = m->pool.as<uint32_t>();
    a.lq = m->lq.as<ListQuery>();
    a.present = m->dPresent.as<uint32_t>();
    a.docs = m->dDocs.as<MvSpan>();
    a.Th = m->Th;
    a.Tl = m->Tl;
    a.tmax = m->tmax.as<float>();
    a.Q = m->Q.as<float>();
    a.qspan = m->qspan.as<MvSpan>();
    a.flags = m->kflags.as<int32_t>();
    a.d = m->dims;
    a.dpad = m->dpad;
    const int64_t fit = (int64_t)(MVK_LDS_TILE / mvk_lds_bytes(1, m->dpad)) / 32 * 32;
    a.qtile = (int)std::min<int64_t>(std::min<int64_t>(std::max<int64_t>(fit, 32), MVK_QTILE_MAX),
                                     round_up(std::max<int64_t>(max_qv, 1), 32));
    for (size_t g = 0; g < plan.groups.size(); g++) {
        const ListGroup& gr = plan.groups[g];
        a.pieces = m->pieces.as<ListPiece>() + gr.piece0;
        a.Kc = m->Kc.as<float>() + gbase[g];
        a.Ab = m->kAb.as<uint64_t>() + gbase[g] / 64;
        rc = mv_launch_keys(s, a, (unsigned)(gr.piece1 - gr.piece0));
        if (rc) return rc;
        k_mv_cut<<<(unsigned)(gr.lq1 - gr.lq0), 256, 0, s>>>(a.Kc, a.Ab, a.pool, a.lq + gr.lq0, a.tmax, m->cS.as<float>(),
                                                             a.flags, k + 1, cap, m->cand.as<uint32_t>(),
                                                             m->ccnt.as<int32_t>());
        HIPCHK(hipGetLastError());
    }
    if (m->timing) HIPCHK(hipEventRecord(m->evk1, s));
    std::vector<int32_t> cnt((size_t)nq);
    std::vector<uint32_t> slots((size_t)nq * cap);
    m->h_cS.resize((size_t)nq);
    m->h_kflags.resize((size_t)nq);
    HIPCHK(hipMemcpyAsync(cnt.data(), m->ccnt.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(m->h_kflags.data(), m->kflags.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(m->h_cS.data(), m->cS.p, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(slots.data(), m->cand.p, (size_t)nq * cap * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));  // the one synchronisation between the two stages
    if (m->timing) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, m->evk0, m->evk1);
        m->stats.last_key_ms = ms;
    }
    for (const ListQuery& q : plan.queries) {
        const size_t r = (size_t)q.q;
        flagged[r] = m->h_kflags[r];
        if (flagged[r]) continue;  // its pairs are counted by the exact search of its list
        cand[r].assign(slots.begin() + r * cap, slots.begin() + r * cap + cnt[r]);
        m->stats.last_scan_rows += (uint64_t)q.len;
        for (int64_t j = 0; j < q.len; j++) {
            const uint32_t sl = plan.pool[(size_t)(q.pool_begin + j)];
            if (mv_present(m, sl)) m->stats.last_token_rows += (uint64_t)m->h_docs[sl].len;
        }
    }
    m->kdbg = true;
    return WV_OK;
}

}  // namespace

extern "C" int wv_mv_create(const wv_mv_config* cfg, wv_mv** out) {
    if (!cfg || !out) return set_err(WV_ERR_INVALID, "invalid config: nil");
    if (cfg->metric < 0 || cfg->metric > WV_METRIC_MANHATTAN)
        return set_err(WV_ERR_INVALID, "invalid config: unknown distance metric %d", cfg->metric);
    // the multi-vector score is always -dot; the index's distance decides the normalisation only, and
    // the reference normalises for cosine-dot alone.  hamming / manhattan indexes: DESIGN.md §3.13
    if (cfg->metric == WV_METRIC_HAMMING || cfg->metric == WV_METRIC_MANHATTAN)
        return set_err(WV_ERR_UNSUPPORTED, "multivector: the %s distance is not supported",
                       cfg->metric == WV_METRIC_HAMMING ? "hamming" : "manhattan");
    if (cfg->dims < 0) return set_err(WV_ERR_INVALID, "invalid config: negative dimensions");
    wv_mv* m = new wv_mv();  // no device call: the first add or search opens the device
    m->metric = cfg->metric;
    m->variant = wv_resolve_variant(cfg->variant);
    m->device = cfg->device;
    m->id_base = cfg->id_base;
    if (cfg->dims > 0) {
        m->dims = cfg->dims;
        m->dpad = (int)round_up(cfg->dims, 32);
    }
    *out = m;
    return WV_OK;
}

extern "C" void wv_mv_destroy(wv_mv* m) {
    if (!m) return;
    if (m->stream || m->T) {
        hipSetDevice(m->device);
        if (m->stream) hipStreamSynchronize(m->stream);
        if (m->T) hipFree(m->T);
        if (m->Th) hipFree(m->Th);
        if (m->Tl) hipFree(m->Tl);
        if (m->tnorm) hipFree(m->tnorm);
        if (m->ev0) hipEventDestroy(m->ev0);
        if (m->ev1) hipEventDestroy(m->ev1);
        if (m->evk0) hipEventDestroy(m->evk0);
        if (m->evk1) hipEventDestroy(m->evk1);
        if (m->stream) hipStreamDestroy(m->stream);
    }
    delete m;
}

// hnsw.AddMultiBatch (insert.go:219-277) + ValidateMultiBeforeInsert (:63-98)
extern "C" int wv_mv_add_batch(wv_mv* m, const uint64_t* doc_ids, const int64_t* vec_offsets, const float* vecs,
                               int64_t n, int64_t d) {
    if (!m) return set_err(WV_ERR_INVALID, "nil index");
    if (n <= 0) return set_err(WV_ERR_INSERT, "addMultiBatch called with empty lists");
    if (!doc_ids || !vec_offsets) return set_err(WV_ERR_INVALID, "nil doc ids or offsets");
    if (vec_offsets[0] < 0) return set_err(WV_ERR_INVALID, "vector offsets must not decrease");
    for (int64_t i = 0; i < n; i++) {
        if (vec_offsets[i + 1] < vec_offsets[i]) return set_err(WV_ERR_INVALID, "vector offsets must not decrease");
        if (vec_offsets[i + 1] == vec_offsets[i])
            return set_err(WV_ERR_INSERT, "multi vector of document %llu has no vectors", (unsigned long long)doc_ids[i]);
        if (vec_offsets[i + 1] - vec_offsets[i] > INT32_MAX)
            return set_err(WV_ERR_INSERT, "multi vector of document %llu is too long", (unsigned long long)doc_ids[i]);
    }
    if (d <= 0) return set_err(WV_ERR_INSERT, "insert called with nil-vector");
    if (!vecs) return set_err(WV_ERR_INVALID, "nil vectors");
    std::lock_guard<std::mutex> g(m->mu);
    if (m->dims && d != m->dims)
        return set_err(WV_ERR_INSERT,
                       "new node has a multi vector with length %lld at position 0. Existing nodes have vectors with "
                       "length %d", (long long)d, m->dims);
    std::unordered_set<uint64_t> seen;
    uint64_t max_slot = 0;
    for (int64_t i = 0; i < n; i++) {
        if (doc_ids[i] < m->id_base || doc_ids[i] - m->id_base >= 0xFFFFFFFFull)
            return set_err(WV_ERR_INVALID, "doc id %llu outside this index's range", (unsigned long long)doc_ids[i]);
        const uint64_t slot = doc_ids[i] - m->id_base;
        // the reference would append to docIDVectors[docID]; the shard deletes before it re-adds
        if (mv_present(m, slot) || !seen.insert(slot).second)
            return set_err(WV_ERR_INSERT, "document %llu is already stored: delete it before adding it again",
                           (unsigned long long)doc_ids[i]);
        max_slot = std::max(max_slot, slot);
    }
    if (!m->dims) {
        m->dims = (int)d;
        m->dpad = (int)round_up(d, 32);
    }
    int rc = mv_device(m);
    if (rc) return rc;
    const int64_t v0 = vec_offsets[0], rows = vec_offsets[n] - v0;
    rc = mv_ensure_tokens(m, m->tok_used + rows);
    if (rc) return rc;
    rc = mv_upload_rows(m, vecs + v0 * d, rows, m->T + m->tok_used * m->dpad);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(m->stream));
    if ((int64_t)max_slot + 1 > m->hiwater) {
        m->hiwater = (int64_t)max_slot + 1;
        m->h_docs.resize((size_t)m->hiwater, MvSpan{0, 0, 0});
        m->h_present.resize((size_t)((m->hiwater + 31) / 32), 0u);
    }
    for (int64_t i = 0; i < n; i++) {
        const uint64_t slot = doc_ids[i] - m->id_base;
        m->h_docs[slot] = MvSpan{m->tok_used + vec_offsets[i] - v0, (int32_t)(vec_offsets[i + 1] - vec_offsets[i]), 0};
        m->h_present[slot >> 5] |= 1u << (slot & 31u);
    }
    m->tok_used += rows;
    m->ndocs += n;
    m->meta_dirty = true;
    m->tmax_valid = false;
    m->kdbg = false;
    return WV_OK;
}

// hnsw.DeleteMulti (delete.go:105-135); the token rows stay where they are
extern "C" int wv_mv_delete(wv_mv* m, const uint64_t* ids, int64_t n) {
    if (!m) return set_err(WV_ERR_INVALID, "nil index");
    std::lock_guard<std::mutex> g(m->mu);
    for (int64_t i = 0; i < n; i++) {
        if (ids[i] < m->id_base || !mv_present(m, ids[i] - m->id_base)) continue;
        const uint64_t slot = ids[i] - m->id_base;
        m->h_present[slot >> 5] &= ~(1u << (slot & 31u));
        m->ndocs--;
        m->meta_dirty = true;
    }
    return WV_OK;
}

// hnsw.ContainsDoc's multi-vector arm (index.go:767-773)
extern "C" int wv_mv_contains_doc(wv_mv* m, uint64_t id) {
    if (!m) return 0;
    std::lock_guard<std::mutex> g(m->mu);
    return id >= m->id_base && mv_present(m, id - m->id_base) ? 1 : 0;
}

extern "C" int wv_mv_search_batch(wv_mv* m, const float* qvecs, const int64_t* q_offsets, int64_t nq, int64_t d,
                                  int32_t k, const uint64_t* allow_ids, const int64_t* allow_offsets,
                                  const int32_t* allow_modes, uint64_t* out_ids, float* out_dists,
                                  int32_t* out_counts) {
    if (!m) return set_err(WV_ERR_INVALID, "nil index");
    if (k <= 0) return set_err(WV_ERR_INVALID, "k must be positive (reference heap Top() on empty queue)");
    if (nq <= 0) return WV_OK;
    if (!q_offsets || !out_counts) return set_err(WV_ERR_INVALID, "nil query offsets or outputs");
    if (q_offsets[0] < 0) return set_err(WV_ERR_INVALID, "query offsets must not decrease");
    int64_t max_qv = 0;
    for (int64_t q = 0; q < nq; q++) {
        const int64_t len = q_offsets[q + 1] - q_offsets[q];
        if (len < 0) return set_err(WV_ERR_INVALID, "query offsets must not decrease");
        if (len == 0) return set_err(WV_ERR_INVALID, "multi vector query %lld has no vectors", (long long)q);
        if (len > INT32_MAX) return set_err(WV_ERR_INVALID, "multi vector query %lld is too long", (long long)q);
        max_qv = std::max(max_qv, len);
        if (allow_modes && allow_modes[q]) {
            if (!allow_offsets) return set_err(WV_ERR_INVALID, "nil allow offsets");
            if (allow_offsets[q] < 0 || allow_offsets[q + 1] < allow_offsets[q])
                return set_err(WV_ERR_INVALID, "allow offsets must not decrease");
        }
    }
    if (replay_scan_lds(k) > 160 * 1024)
        return set_err(WV_ERR_INVALID, "k=%d exceeds the exact replay heap limit of %d results", k,
                       (int)((160 * 1024 - 272) / 12));
    std::lock_guard<std::mutex> g(m->mu);
    int rc = mv_check_dims(m, d);
    if (rc) return rc;
    m->stats.queries += (uint64_t)nq;
    m->stats.batches++;
    m->stats.last_route = WV_ROUTE_MV_MAXSIM;
    m->stats.last_scan_rows = m->stats.last_token_rows = 0;
    m->stats.last_kernel_ms = m->stats.last_key_ms = 0.0;
    m->stats.last_key_queries = m->stats.last_candidates = m->stats.last_fallback_queries = 0;
    if (m->ndocs == 0) {
        for (int64_t q = 0; q < nq; q++) out_counts[q] = 0;
        return WV_OK;
    }
    if (!qvecs || !out_ids || !out_dists) return set_err(WV_ERR_INVALID, "nil query vectors or outputs");
    // every query's list as a range of one id array: the callers' lists, then -- for the queries
    // without a list -- the stored documents in id order, once
    std::vector<int64_t> lo((size_t)nq), hi((size_t)nq);
    std::vector<uint64_t> all;
    int64_t n_allow = 0;
    bool any0 = false;
    for (int64_t q = 0; q < nq; q++) {
        if (allow_modes && allow_modes[q]) n_allow = std::max(n_allow, allow_offsets[q + 1]);
        else any0 = true;
    }
    const uint64_t* ids = allow_ids;
    if (any0) {
        all.reserve((size_t)(n_allow + m->ndocs));
        if (n_allow) all.insert(all.end(), allow_ids, allow_ids + n_allow);
        for (int64_t sl = 0; sl < m->hiwater; sl++)
            if (mv_present(m, (uint64_t)sl)) all.push_back(m->id_base + (uint64_t)sl);
        ids = all.data();
    }
    for (int64_t q = 0; q < nq; q++) {
        const bool listed = allow_modes && allow_modes[q];
        lo[(size_t)q] = listed ? allow_offsets[q] : n_allow;
        hi[(size_t)q] = listed ? allow_offsets[q + 1] : n_allow + m->ndocs;
    }
    rc = mv_device(m);
    if (rc) return rc;
    rc = mv_sync_meta(m);
    if (rc) return rc;
    rc = mv_upload_queries(m, qvecs, q_offsets, nq);
    if (rc) return rc;
    // the queries of the key route: option mv_keys, the kernel's widths, the heap's room for k + 1, a
    // list of at least mv_keys_min ids
    const bool keys_on = (m->mv_keys == 1 || (m->mv_keys < 0 && MV_KEYS_AUTO)) && m->dpad <= MVK_MAX_DPAD &&
                         max_qv <= MVK_MAX_QV && k < INT32_MAX && replay_scan_lds(k + 1) <= 160 * 1024;
    const int64_t kmin = std::max<int64_t>(m->mv_keys_min >= 0 ? m->mv_keys_min : MV_KEYS_MIN, 1);
    std::vector<int64_t> klo((size_t)nq, -1);
    int64_t nkey = 0;
    for (int64_t q = 0; q < nq && keys_on; q++)
        if (hi[(size_t)q] - lo[(size_t)q] >= kmin) {
            klo[(size_t)q] = lo[(size_t)q];
            nkey++;
        }
    if (nkey == 0)  // today's call
        return mv_exact_search(m, ids, lo.data(), hi.data(), nq, k, max_qv, true, out_ids, out_dists, out_counts);

    m->stats.last_route = WV_ROUTE_MV_KEYS;
    m->stats.last_key_queries = (uint64_t)nkey;
    std::vector<std::vector<uint32_t>> cand((size_t)nq);
    std::vector<int32_t> flagged((size_t)nq, 0);
    rc = mv_key_pass(m, ids, klo.data(), hi.data(), nq, k, max_qv, cand, flagged);
    if (rc) return rc;
    // second stage: the candidates as each query's allow list, the exact search with limit k + 1
    const int k1 = k + 1;
    std::vector<uint64_t> cids;
    std::vector<int64_t> clo((size_t)nq, -1), chi((size_t)nq, -1);
    int64_t nsecond = 0;
    for (int64_t q = 0; q < nq; q++) {
        if (klo[(size_t)q] < 0 || flagged[(size_t)q]) continue;
        clo[(size_t)q] = (int64_t)cids.size();
        for (uint32_t sl : cand[(size_t)q]) cids.push_back(m->id_base + sl);
        chi[(size_t)q] = (int64_t)cids.size();
        m->stats.last_candidates += (uint64_t)cand[(size_t)q].size();
        nsecond++;
    }
    if (cids.empty()) cids.push_back(0);
    std::vector<uint64_t> tI;
    std::vector<float> tD;
    std::vector<int32_t> tN((size_t)nq);
    if (nsecond) {
        tI.resize((size_t)nq * k1);
        tD.resize((size_t)nq * k1);
        rc = mv_exact_search(m, cids.data(), clo.data(), chi.data(), nq, k1, max_qv, false, tI.data(), tD.data(), tN.data());
        if (rc) return rc;
        for (int64_t q = 0; q < nq; q++) {
            if (clo[(size_t)q] < 0) continue;
            // k + 1 (or all) scores pairwise distinct: the first k are the reference's, whatever the heap's history
            const int n = tN[(size_t)q];
            const float* dq = tD.data() + (size_t)q * k1;
            bool distinct = true;
            for (int i = 0; i + 1 < n; i++) distinct = distinct && dq[i] < dq[i + 1];
            if (!distinct) {
                flagged[(size_t)q] = MVK_FLAG_TIE;
                continue;
            }
            const int nk = std::min(n, (int)k);
            std::copy(tI.begin() + (size_t)q * k1, tI.begin() + (size_t)q * k1 + nk, out_ids + (size_t)q * k);
            std::copy(dq, dq + nk, out_dists + (size_t)q * k);
            out_counts[q] = nk;
        }
    }
    // the flagged queries and those that took no keys: today's call over their original lists
    int64_t nrest = 0;
    for (int64_t q = 0; q < nq; q++) {
        const bool key = klo[(size_t)q] >= 0;
        if (key && flagged[(size_t)q]) m->stats.last_fallback_queries++;
        if (key && !flagged[(size_t)q]) lo[(size_t)q] = -1;
        else nrest++;
    }
    if (nrest) {
        tI.resize((size_t)nq * k);
        tD.resize((size_t)nq * k);
        rc = mv_exact_search(m, ids, lo.data(), hi.data(), nq, k, max_qv, true, tI.data(), tD.data(), tN.data());
        if (rc) return rc;
        for (int64_t q = 0; q < nq; q++) {
            if (lo[(size_t)q] < 0) continue;
            std::copy(tI.begin() + (size_t)q * k, tI.begin() + (size_t)(q + 1) * k, out_ids + (size_t)q * k);
            std::copy(tD.begin() + (size_t)q * k, tD.begin() + (size_t)(q + 1) * k, out_dists + (size_t)q * k);
            out_counts[q] = tN[(size_t)q];
        }
    }
    return WV_OK;
}

// hnsw.QueryMultiVectorDistancer (search.go:1033-1045): computeScore of one query against n documents
extern "C" int wv_mv_query_distances(wv_mv* m, const float* qvecs, int64_t nqv, int64_t d, const uint64_t* ids,
                                     int64_t n, float* out) {
    if (!m) return set_err(WV_ERR_INVALID, "nil index");
    if (nqv <= 0) return set_err(WV_ERR_INVALID, "multi vector query 0 has no vectors");
    if (nqv > INT32_MAX) return set_err(WV_ERR_INVALID, "multi vector query 0 is too long");
    std::lock_guard<std::mutex> g(m->mu);
    int rc = mv_check_dims(m, d);
    if (rc) return rc;
    if (n <= 0) return WV_OK;
    std::vector<uint32_t> pool((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (ids[i] < m->id_base || !mv_present(m, ids[i] - m->id_base))
            return set_err(WV_ERR_INVALID, "docID %llu is not in the vector index", (unsigned long long)ids[i]);
        pool[(size_t)i] = (uint32_t)(ids[i] - m->id_base);
    }
    if (!qvecs || !out) return set_err(WV_ERR_INVALID, "nil query vectors or outputs");
    // one listed query over the ids as given: a piece per chunk
    const std::vector<ListQuery> lq{ListQuery{0, 0, n, 0}};
    std::vector<ListPiece> pieces;
    for (int64_t f = 0; f < n; f += LIST_CHUNK)
        pieces.push_back(ListPiece{0, (int32_t)std::min<int64_t>(LIST_CHUNK, n - f), f});
    rc = mv_device(m);
    if (rc) return rc;
    rc = mv_sync_meta(m);
    if (rc) return rc;
    const int64_t q_offsets[2] = {0, nqv};
    rc = mv_upload_queries(m, qvecs, q_offsets, 1);
    if (rc) return rc;
    rc = mv_upload_plan(m, pool, lq, pieces, round_up(n, LIST_CHUNK));
    if (rc) return rc;
    rc = mv_launch_scores(m, m->stream, mv_args(m), (unsigned)pieces.size(), nqv);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, m->Ec.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return WV_OK;
}

extern "C" int wv_mv_set_option(wv_mv* m, const char* key, int64_t value) {
    if (!m || !key) return set_err(WV_ERR_INVALID, "nil index or key");
    std::lock_guard<std::mutex> g(m->mu);
    const std::string k = key;
    if (k == "mv_tile") {
        if (value < -1 || value > 1) return set_err(WV_ERR_INVALID, "mv_tile: -1, 0 or 1");
        m->mv_tile = (int)value;
    } else if (k == "mv_list_rows") m->mv_list_rows = std::max<int64_t>(value, 0);
    else if (k == "timing") m->timing = value ? 1 : 0;
    else if (k == "mv_keys") {
        if (value < -1 || value > 1) return set_err(WV_ERR_INVALID, "mv_keys: -1, 0 or 1");
        m->mv_keys = (int)value;
    } else if (k == "mv_keys_min") {
        if (value < 0) return set_err(WV_ERR_INVALID, "mv_keys_min: 0 or more");
        m->mv_keys_min = value;
    } else if (k == "mv_keys_cap") {
        if (value < 1 || value > INT32_MAX) return set_err(WV_ERR_INVALID, "mv_keys_cap: 1 or more");
        m->mv_keys_cap = value;
    } else return set_err(WV_ERR_INVALID, "unknown option %s", key);
    return WV_OK;
}

extern "C" int wv_mv_debug_keys(wv_mv* m, int64_t q, float* keys, float* eps, uint32_t* slots, int64_t* n) {
    if (!m || !n) return set_err(WV_ERR_INVALID, "nil index or count");
    std::lock_guard<std::mutex> g(m->mu);
    if (!m->kdbg) return set_err(WV_ERR_INVALID, "no key search to report");
    size_t i = 0;
    while (i < m->kplan.queries.size() && m->kplan.queries[i].q != q) i++;
    if (i == m->kplan.queries.size()) return set_err(WV_ERR_INVALID, "query %lld took no keys", (long long)q);
    const ListQuery& lq = m->kplan.queries[i];
    *n = lq.len;
    if (!keys || lq.len == 0) return WV_OK;
    if (!eps || !slots) return set_err(WV_ERR_INVALID, "nil eps or slots");
    HIPCHK(hipSetDevice(m->device));
    const int64_t e0 = m->kabs[i], words = (lq.len + 63) / 64;
    std::vector<uint64_t> ab((size_t)words);
    std::vector<float> tm((size_t)m->hiwater);
    HIPCHK(hipMemcpy(keys, m->Kc.as<float>() + e0, (size_t)lq.len * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ab.data(), m->kAb.as<uint64_t>() + e0 / 64, (size_t)words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tm.data(), m->tmax.p, tm.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < lq.len; j++) {
        const uint32_t sl = m->kplan.pool[(size_t)(lq.pool_begin + j)];
        slots[j] = sl;
        if ((ab[(size_t)(j >> 6)] >> (j & 63)) & 1ull) {  // a listed slot without a document
            keys[j] = __builtin_inff();
            eps[j] = 0.f;
        } else {
            eps[j] = mvk_eps(m->h_cS[(size_t)q], tm[sl], keys[j]);
        }
    }
    return WV_OK;
}

extern "C" int wv_mv_get_stats(wv_mv* m, wv_mv_stats* out) {
    if (!m || !out) return set_err(WV_ERR_INVALID, "nil index or stats");
    std::lock_guard<std::mutex> g(m->mu);
    m->stats.documents = (uint64_t)m->ndocs;
    m->stats.token_rows = (uint64_t)m->tok_used;
    m->stats.dims = (uint64_t)m->dims;
    *out = m->stats;
    return WV_OK;
}
