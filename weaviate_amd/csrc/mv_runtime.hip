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
#include "rt_index.h"
#include "mv_kernels.hip"

#include <unordered_set>

namespace {

// k_mv_maxsim's instantiations: the AVX2 order (and the AVX-512 order below 128
// elements, where both coincide), and the AVX-512 order from 128 elements on
constexpr int MV_QT = 4, MV_RT = 2;
constexpr int MV_QT5 = 2, MV_RT5 = 2;
constexpr size_t MV_LDS_TILE = 32 * 1024;  // the query is staged whole while it fits
constexpr size_t MV_LDS_MAX = 64 * 1024;   // QT rows must fit, else the simple arm

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

// room for `rows` token rows; the rows already stored move with the buffer
int mv_ensure_tokens(wv_mv* m, int64_t rows) {
    if (rows <= m->tok_cap) return WV_OK;
    const int64_t cap = std::max<int64_t>(std::max<int64_t>(rows, m->tok_cap * 2), 1024);
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
        if (m->ev0) hipEventDestroy(m->ev0);
        if (m->ev1) hipEventDestroy(m->ev1);
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
    m->stats.last_kernel_ms = 0.0;
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
    const int64_t budget = m->mv_list_rows > 0 ? m->mv_list_rows : (int64_t)4 << 20;
    const ListPlan plan = list_plan(ids, lo.data(), hi.data(), nq, m->id_base, m->hiwater, budget, 1);
    m->stats.last_scan_rows = (uint64_t)plan.scanned;
    for (const ListQuery& q : plan.queries)
        for (int64_t i = 0; i < q.len; i++) {
            const uint32_t sl = plan.pool[(size_t)(q.pool_begin + i)];
            if (mv_present(m, sl)) m->stats.last_token_rows += (uint64_t)m->h_docs[sl].len;
        }
    rc = mv_device(m);
    if (rc) return rc;
    hipStream_t s = m->stream;
    rc = mv_sync_meta(m);
    if (rc) return rc;
    rc = mv_upload_queries(m, qvecs, q_offsets, nq);
    if (rc) return rc;
    rc = mv_upload_plan(m, plan.pool, plan.queries, plan.pieces, plan.max_entries);
    if (rc) return rc;
    HIPCHK(m->oI.ensure((size_t)nq * k * sizeof(uint64_t)));
    HIPCHK(m->oD.ensure((size_t)nq * k * sizeof(float)));
    HIPCHK(m->oN.ensure((size_t)nq * sizeof(int32_t)));
    const size_t lds_h = replay_scan_lds(k);
    const bool pk = k <= PACKED_REPLAY_MAX_K;
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
            k_list_heap<true><<<nl, 64, lds_h, s>>>(a.Ec, a.Bc, a.Ab, a.pool, a.lq + gr.lq0, (int)nl, k, m->id_base,
                                                    m->oI.as<uint64_t>(), m->oD.as<float>(), m->oN.as<int32_t>());
        else
            k_list_heap<false><<<nl, 64, lds_h, s>>>(a.Ec, a.Bc, a.Ab, a.pool, a.lq + gr.lq0, (int)nl, k, m->id_base,
                                                     m->oI.as<uint64_t>(), m->oD.as<float>(), m->oN.as<int32_t>());
        HIPCHK(hipGetLastError());
    }
    if (m->timing) HIPCHK(hipEventRecord(m->ev1, s));
    HIPCHK(hipMemcpyAsync(out_ids, m->oI.p, (size_t)nq * k * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_dists, m->oD.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_counts, m->oN.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (m->timing) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, m->ev0, m->ev1);
        m->stats.last_kernel_ms = ms;
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
    else return set_err(WV_ERR_INVALID, "unknown option %s", key);
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
