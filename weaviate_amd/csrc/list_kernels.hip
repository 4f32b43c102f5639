// list_kernels.hip -- hnsw.flatSearch (hnsw/flat_search.go:28-141) in list
// order: the reference's loop is `for idPos ... candidates[idPos]`, its cost
// the allow list's length.  The planner (list_plan.h) leaves every listed
// query an ascending, distinct, in-range slot list in a shared pool; here
//
//   k_list_dist<COMP>  the compressor distance of every (query, listed row):
//                      one lane per list entry, LIST_CHUNK = 256 entries per
//                      chunk, a workgroup per work-table piece (one or several
//                      consecutive chunks of one query).  The query's
//                      compressor state is staged once per workgroup in LDS
//                      (BQ words, SQ / rq-8 code bytes, rq-1 planes, PQ LUT
//                      chunks of PQ_CH segments); each lane reads its slot,
//                      tests `present`, gathers the row's code from the
//                      index's code layout and computes the distance with the
//                      operations of k_bq_dist / k_sq_dist / k_rq8_dist /
//                      k_rq1_dist / k_pq_adc (same bits).
//                      Writes Ec[entry], the fminf minimum Bc[chunk] and one
//                      absent bit per entry (Ab, a u64 per 64 entries: rows
//                      not present and the padding of a list's last chunk).
//   k_list_heap<PK>    the worker heap (addResult == insertToHeap with
//                      `limit`) over one query's compact list in list order =
//                      ascending id order, one wave per query: k_replay_scan's
//                      loop with chunk minima for block minima, the absent bits
//                      for the bitmap and id = id_base + pool slot.  Extracted
//                      ascending into ascI / ascD / ascN by query (k_pq_finish).
//
// Entry indices are relative to the launch group's compact buffers; a query's
// first entry is a multiple of LIST_CHUNK.
#pragma once

namespace wv {
namespace {  // internal linkage: each runtime unit compiles the kernels it launches

// chunks per workgroup, chosen by measurement (1, 2, 4 and 8 timed at 64 x 10 000 entries)
constexpr int LIST_CPW = 2;     // BQ / SQ / rq-8 / rq-1 (option hnsw_list_chunks: any count)
constexpr int LIST_PQ_CPW = 2;  // PQ: chunks per staged LUT chunk (instantiated: 2, 4, 8)

enum { LC_BQ = 0, LC_SQ = 1, LC_RQ8 = 2, LC_RQ1 = 3, LC_PQ = 4, LC_PQ256 = 5 };

struct ListDistArgs {
    const uint32_t* pool;      // slots of every list (ListPlan::pool)
    const ListQuery* lq;       // listed queries
    const ListPiece* pieces;   // this launch's pieces
    const uint32_t* present;
    float* Ec;                 // [entries] distances
    float* Bc;                 // [entries / 256] chunk minima
    uint64_t* Ab;              // [entries / 64] absent bits
    const void* codes;         // stored codes (the compressor's layout)
    int64_t cap;               // BQ / rq-1: the word-major stride
    const void* meta;          // SQ uint2, rq float4
    const void* qcodes;        // BQ [W][nq] u64, SQ / rq-8 group-tiled uint4, rq-1 group-tiled planes, PQ LUT [nq][m][k]
    const void* qmeta;         // SQ uint2, rq float4
    int64_t nq;                // BQ: the query-code stride
    int D;                     // BQ words, SQ Dq, rq D, PQ m
    int K, g16;                // PQ centroids, 16-segment groups
    int metric;                // SQ / PQ: L2 / DOT / COSINE
    float f0, f1, f2;          // SQ a2, ab, ib2; rq fl2, fcos
};

// distance, chunk minimum and absent bits of one chunk (block-uniform call)
__device__ __forceinline__ void list_emit(const ListDistArgs& a, int64_t e, float dist, bool pres, float* red) {
    const int tid = threadIdx.x, lane = tid & 63, wv_ = tid >> 6;
    a.Ec[e + tid] = dist;
    const float m = wave_min(pres ? dist : __builtin_inff());
    const uint64_t ab = __ballot(!pres);
    if (lane == 0) {
        red[wv_] = m;
        a.Ab[(e >> 6) + wv_] = ab;
    }
    __syncthreads();
    if (tid == 0) a.Bc[e >> 8] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    __syncthreads();
}

// CPW: PQ only, the chunks a workgroup takes per staged LUT chunk (running sums in registers)
template <int COMP, int CPW = 1>
__global__ __launch_bounds__(256) void k_list_dist(const ListDistArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_q[];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const ListPiece pc = a.pieces[blockIdx.x];
    const ListQuery lq = a.lq[pc.lq];
    const int64_t q = lq.q;
    const uint32_t* __restrict__ slots = a.pool + lq.pool_begin + pc.first;
    const int64_t e0 = lq.e_begin + pc.first;

    if constexpr (COMP == LC_PQ || COMP == LC_PQ256) {
        float* lsm = reinterpret_cast<float*>(lds_q);  // [PQ_CH][k]
        const int k = COMP == LC_PQ256 ? 256 : a.K;
        const int m = a.D, g16 = a.g16;
        const float* __restrict__ L = reinterpret_cast<const float*>(a.qcodes) + q * m * k;
        const uint4* __restrict__ c4 = reinterpret_cast<const uint4*>(a.codes);
        float sum[CPW];
        int64_t cbase[CPW];  // uint4 index of the row's group 0, -1: no entry
        uint32_t slot[CPW];
#pragma unroll
        for (int r = 0; r < CPW; r++) {
            const int i = r * LIST_CHUNK + tid;
            sum[r] = 0.f;
            slot[r] = i < pc.count ? slots[i] : 0u;
            cbase[r] = i < pc.count ? ((int64_t)(slot[r] >> 8) * g16) * 256 + (slot[r] & 255u) : -1;
        }
        for (int s0 = 0; s0 < m; s0 += PQ_CH) {
            const int ns = m - s0 < PQ_CH ? m - s0 : PQ_CH;
            __syncthreads();
            for (int i = tid; i < ns * k; i += 256) lsm[i] = L[(int64_t)s0 * k + i];
            __syncthreads();
#pragma unroll 1
            for (int c16 = 0; c16 < ns; c16 += 16) {
                const float* lc = lsm + c16 * k;
                const int g = (s0 + c16) >> 4;
                const int nv = ns - c16 < 16 ? ns - c16 : 16;
                uint4 cw[CPW];
#pragma unroll
                for (int r = 0; r < CPW; r++)
                    cw[r] = cbase[r] >= 0 ? c4[cbase[r] + (int64_t)g * 256] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (int r = 0; r < CPW; r++) {
                    float acc = sum[r];
                    const uint32_t w4[4] = {cw[r].x, cw[r].y, cw[r].z, cw[r].w};
                    if (nv == 16) {
#pragma unroll
                        for (int w = 0; w < 4; w++)
#pragma unroll
                            for (int b = 0; b < 4; b++) acc = acc + lc[(4 * w + b) * k + ((w4[w] >> (8 * b)) & 0xFFu)];
                    } else {
#pragma unroll 1
                        for (int j = 0; j < nv; j++) {
                            const uint32_t w = j < 4 ? w4[0] : j < 8 ? w4[1] : j < 12 ? w4[2] : w4[3];
                            acc = acc + lc[j * k + ((w >> (8 * (j & 3))) & 0xFFu)];
                        }
                    }
                    sum[r] = acc;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < CPW; r++) {
            if (r * LIST_CHUNK < pc.count) {  // block-uniform
                const bool pres = cbase[r] >= 0 && ((a.present[slot[r] >> 5] >> (slot[r] & 31u)) & 1u);
                list_emit(a, e0 + r * LIST_CHUNK, pres ? pq_wrap(a.metric, sum[r]) : __builtin_inff(), pres, red);
            }
        }
    } else {
        // the query's codes, once per workgroup
        const int D = a.D;
        uint4* qs = reinterpret_cast<uint4*>(lds_q);
        if constexpr (COMP == LC_BQ) {
            uint64_t* qw = reinterpret_cast<uint64_t*>(lds_q);
            const uint64_t* __restrict__ qc = reinterpret_cast<const uint64_t*>(a.qcodes);
            for (int w = tid; w < D; w += 256) qw[w] = qc[(int64_t)w * a.nq + q];
        } else if constexpr (COMP == LC_RQ1) {
            if (tid < 64) rq_query_to_lds<1>(qs, a.qcodes, q, q, D, tid);
        } else {  // SQ / rq-8: chunk c of query q in the group-tiled layout
            const int nch = D >> 4;
            const uint4* __restrict__ qc = reinterpret_cast<const uint4*>(a.qcodes) + (q / RQ_QPB) * nch * RQ_QPB + q % RQ_QPB;
            for (int c = tid; c < nch; c += 256) qs[c] = qc[(int64_t)c * RQ_QPB];
        }
        __syncthreads();
        float4 ym4 = make_float4(0.f, 0.f, 0.f, 0.f);
        uint2 ym2 = make_uint2(0u, 0u);
        if constexpr (COMP == LC_RQ8 || COMP == LC_RQ1) ym4 = reinterpret_cast<const float4*>(a.qmeta)[q];
        if constexpr (COMP == LC_SQ) ym2 = reinterpret_cast<const uint2*>(a.qmeta)[q];
        for (int c0 = 0; c0 < pc.count; c0 += LIST_CHUNK) {
            const int i = c0 + tid;
            const uint32_t slot = i < pc.count ? slots[i] : 0u;
            const bool pres = i < pc.count && ((a.present[slot >> 5] >> (slot & 31u)) & 1u);
            float dist = __builtin_inff();
            if (pres) {
                if constexpr (COMP == LC_BQ) {  // k_bq_dist: popcount(x ^ y) over the words
                    const uint64_t* __restrict__ cd = reinterpret_cast<const uint64_t*>(a.codes) + slot;
                    const uint64_t* qw = reinterpret_cast<const uint64_t*>(lds_q);
                    uint32_t acc = 0;
#pragma unroll 8
                    for (int w = 0; w < D; w++) acc += (uint32_t)__popcll(cd[(int64_t)w * a.cap] ^ qw[w]);
                    dist = (float)acc;
                } else if constexpr (COMP == LC_SQ) {  // k_sq_dist
                    const int nch = D >> 4;
                    const uint4* __restrict__ xr =
                        reinterpret_cast<const uint4*>(a.codes) + (int64_t)(slot >> 8) * nch * 256 + (slot & 255u);
                    uint32_t acc = 0;
#pragma unroll 8
                    for (int c = 0; c < nch; c++) {
                        const uint4 x = xr[(int64_t)c * 256];
                        const uint4 y = qs[c];
                        acc = __builtin_amdgcn_udot4(x.x, y.x, acc, false);
                        acc = __builtin_amdgcn_udot4(x.y, y.y, acc, false);
                        acc = __builtin_amdgcn_udot4(x.z, y.z, acc, false);
                        acc = __builtin_amdgcn_udot4(x.w, y.w, acc, false);
                    }
                    const uint2 xm = reinterpret_cast<const uint2*>(a.meta)[slot];
                    if (a.metric == L2) {
                        const uint32_t l2 = xm.y + ym2.y - 2u * acc;  // sum (x - y)^2, exact
                        dist = a.f0 * (float)l2;
                    } else {
                        float t = a.f0 * (float)acc;
                        const float u = a.f1 * (float)(xm.x + ym2.x);
                        t = t + u;
                        t = t + a.f2;
                        dist = a.metric == DOT ? -t : 1.0f - t;
                    }
                } else if constexpr (COMP == LC_RQ8) {
                    dist = rq_row_dist<8>(a.codes, a.cap, reinterpret_cast<const float4*>(a.meta), (int64_t)slot, qs, ym4,
                                          D, a.f0, a.f1);
                } else {
                    dist = rq_row_dist<1>(a.codes, a.cap, reinterpret_cast<const float4*>(a.meta), (int64_t)slot, qs, ym4,
                                          D, a.f0, a.f1);
                }
            }
            list_emit(a, e0 + c0, dist, pres, red);
        }
    }
}

// the worker heap over query blockIdx.x's compact list (see the file header).
// Dynamic LDS as k_replay_scan: PK [k] records | [64] dists | len, else
// [k] ids | [64] dists | [k] heap dists | len.
template <bool PK>
__global__ __launch_bounds__(64) void k_list_heap(const float* __restrict__ Ec, const float* __restrict__ Bc,
                                                  const uint64_t* __restrict__ Ab, const uint32_t* __restrict__ pool,
                                                  const ListQuery* __restrict__ lqs, int nl, int k, uint64_t id_base,
                                                  uint64_t* __restrict__ out_ids, float* __restrict__ out_d,
                                                  int32_t* __restrict__ out_n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rsm[];
    HeapRec* hr = reinterpret_cast<HeapRec*>(rsm);
    uint64_t* hid = reinterpret_cast<uint64_t*>(rsm);
    float* s_d = PK ? reinterpret_cast<float*>(hr + k) : reinterpret_cast<float*>(hid + k);
    float* hd = s_d + 64;
    int* s_len = PK ? reinterpret_cast<int*>(s_d + 64) : reinterpret_cast<int*>(hd + k);
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= nl) return;
    const ListQuery lq = lqs[blockIdx.x];
    const float* Eq = Ec + lq.e_begin;
    const float* Bq = Bc + (lq.e_begin >> 8);
    const uint64_t* Aq = Ab + (lq.e_begin >> 6);
    const uint32_t* sl = pool + lq.pool_begin;
    if (lane == 0) *s_len = 0;
    __syncthreads();
    const int64_t nchunk = (lq.len + LIST_CHUNK - 1) / LIST_CHUNK;
    for (int64_t b0 = 0; b0 < nchunk; b0 += 64) {
        const float bm = (b0 + lane < nchunk) ? Bq[b0 + lane] : __builtin_inff();
        int len = *s_len;
        float top = len > 0 ? (PK ? hr[0].d : hd[0]) : 0.f;
        uint64_t bmask = __ballot((b0 + lane < nchunk) && (len < k || top > bm));
        while (bmask) {
            const int j = __builtin_ctzll(bmask);
            bmask &= bmask - 1;
            const float bmj = __shfl(bm, j);
            len = *s_len;
            top = len > 0 ? (PK ? hr[0].d : hd[0]) : 0.f;
            if (!(len < k || top > bmj)) continue;
            const int64_t r0 = (b0 + j) * LIST_CHUNK;
            for (int sub = 0; sub < LIST_CHUNK; sub += 64) {
                const int64_t i = r0 + sub + lane;
                if (r0 + sub >= lq.len) break;  // wave-uniform
                const uint64_t aw = Aq[(r0 + sub) >> 6];
                const bool ok = i < lq.len && !((aw >> lane) & 1ull);
                const float dist = ok ? Eq[i] : 0.f;
                len = *s_len;
                top = len > 0 ? (PK ? hr[0].d : hd[0]) : 0.f;
                uint64_t mask = __ballot(ok && (len < k || top > dist));
                if (mask == 0) continue;
                s_d[lane] = dist;
                __syncthreads();
                if (lane == 0) {
                    ReplayHeap h{hid, hd, *s_len};
                    PHeap ph{hr, *s_len};
                    while (mask) {
                        const int jj = __builtin_ctzll(mask);
                        mask &= mask - 1;
                        const float dj = s_d[jj];
                        const uint64_t idj = id_base + (uint64_t)sl[r0 + sub + jj];
                        if (PK) ph_offer(ph, k, idj, dj);
                        else if (h.len < k) rh_insert(h, idj, dj);
                        else if (h.dist[0] > dj) { uint64_t x; float y; rh_pop(h, &x, &y); rh_insert(h, idj, dj); }
                    }
                    *s_len = PK ? ph.len : h.len;
                }
                __syncthreads();
            }
        }
    }
    if (lane == 0) {
        // extractHeap: pop max-first, fill from the back
        ReplayHeap h{hid, hd, *s_len};
        PHeap ph{hr, *s_len};
        const int n = *s_len;
        for (int i = n - 1; i >= 0; i--) {
            uint64_t x; float y;
            if (PK) ph_pop(ph, &x, &y);
            else rh_pop(h, &x, &y);
            out_ids[lq.q * k + i] = x;
            out_d[lq.q * k + i] = y;
        }
        out_n[lq.q] = n;
    }
}

}  // namespace
}  // namespace wv
