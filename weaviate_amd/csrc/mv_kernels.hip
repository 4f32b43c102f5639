// mv_kernels.hip -- hnsw.flatMultiSearch (hnsw/flat_search.go:143-212): the
// late-interaction score of every (query, listed document),
//
//   computeScore (hnsw/search.go:954-1006):
//     similarity = 0
//     for q in the query's vectors, in order:
//         maxSim = MaxFloat32
//         for t in the document's vectors: dist = -dot(q, t); if dist < maxSim: maxSim = dist
//         similarity += maxSim
//
// with dot = the provider's SIMD order (exact_raw<DOT, VARIANT>), whatever the
// index's distance (multiDistancerProvider, hnsw/index.go:405-406).  Both
// kernels take the work table of list_plan.h (a piece = one query and up to
// LIST_CHUNK listed document slots; the host plans with one chunk per piece)
// and write what k_list_heap reads: Ec[entry] the score, Bc[chunk] the fminf
// minimum of the chunk's present entries, Ab the absent bits (list_emit).
//
//   k_mv_simple<VARIANT>          a lane per listed document, the loop above
//                                 with exact_dist<DOT, VARIANT> per pair.
//   k_mv_maxsim<VARIANT, QT, RT>  the query's vectors staged in LDS (whole, or
//                                 in tiles of a.qtile vectors with the documents'
//                                 running sums carried in LDS), one wave per
//                                 document at a time, waves round-robin over
//                                 the piece.  A wave streams the document's
//                                 contiguous token rows in exact_dist8's layout:
//                                 8 lanes per row, 8 RT rows per step, lane sub
//                                 owning float4 slot sub of every 32-element
//                                 chunk, against QT query vectors read from LDS
//                                 (the same address in the 8 row groups: a
//                                 broadcast).  4 QT RT independent FMA chains
//                                 per lane, every chain advancing in element
//                                 order; the per-pair reduction is reduce_ymm4's
//                                 tree over the 8 lanes.  The minimum uses
//                                 `d < m` from MaxFloat32 (NaN is never taken),
//                                 first over the lane's rows, then across the 8
//                                 row groups; the sum is one fp32 accumulator in
//                                 query-vector order.
//                                 VARIANT == AVX512 and d >= 128 (where
//                                 exact8_ok is false): the 128-element loop of
//                                 c/dot_avx512_amd64.c with acc5[8][16] spread
//                                 as 16 accumulators per lane, see mv_dots.
// Rows past a document's last one in a step re-read its last row and query
// vectors past the tile's last one duplicate it: a duplicate cannot change a
// minimum, and a padding query vector is never summed.
#pragma once

namespace wv {
namespace {

struct MvSpan {      // device record (16 bytes): rows [begin, begin + len) of a row matrix
    int64_t begin;
    int32_t len;
    int32_t pad;
};

struct MvArgs {
    const uint32_t* pool;     // document slots of every list (ListPlan::pool)
    const ListQuery* lq;      // listed queries
    const ListPiece* pieces;  // this launch's pieces (<= LIST_CHUNK entries each)
    const uint32_t* present;  // document slots holding a document
    const MvSpan* docs;       // [slot] token rows of the document
    const float* T;           // token matrix [rows][dpad]
    const float* Q;           // query vectors of the batch [rows][dpad]
    const MvSpan* qspan;      // [batch row] the query's vectors in Q
    float* Ec;                // [entries] scores
    float* Bc;                // [entries / 256] chunk minima
    uint64_t* Ab;             // [entries / 64] absent bits
    int d, dpad;
    int qtile;                // k_mv_maxsim: query vectors per LDS tile, a multiple of QT
};

constexpr float MV_MAXF = 3.40282346638528859811704183484516925e+38f;  // math.MaxFloat32

template <int VARIANT>
__global__ __launch_bounds__(256) void k_mv_simple(const MvArgs a) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const ListPiece pc = a.pieces[blockIdx.x];
    const ListQuery lq = a.lq[pc.lq];
    const MvSpan qs = a.qspan[lq.q];
    const uint32_t* __restrict__ slots = a.pool + lq.pool_begin + pc.first;
    ListDistArgs la{};
    la.Ec = a.Ec;
    la.Bc = a.Bc;
    la.Ab = a.Ab;
    for (int c0 = 0; c0 < pc.count; c0 += LIST_CHUNK) {
        const int i = c0 + tid;
        const uint32_t slot = i < pc.count ? slots[i] : 0u;
        const bool pres = i < pc.count && ((a.present[slot >> 5] >> (slot & 31u)) & 1u);
        float score = __builtin_inff();
        if (pres) {
            const MvSpan dc = a.docs[slot];
            float sim = 0.f;
            for (int j = 0; j < qs.len; j++) {
                const float* q = a.Q + (qs.begin + j) * a.dpad;
                float m = MV_MAXF;
                for (int t = 0; t < dc.len; t++) {
                    const float dist = exact_dist<DOT, VARIANT>(q, a.T + (dc.begin + t) * a.dpad, a.d);
                    if (dist < m) m = dist;
                }
                sim = sim + m;
            }
            score = sim;
        }
        list_emit(la, lq.e_begin + pc.first + c0, score, pres, red);
    }
}

__device__ __forceinline__ float4 mv_fma4(float4 acc, float4 a, float4 b) {
    acc.x = fmaf(a.x, b.x, acc.x);
    acc.y = fmaf(a.y, b.y, acc.y);
    acc.z = fmaf(a.z, b.z, acc.z);
    acc.w = fmaf(a.w, b.w, acc.w);
    return acc;
}

// exact_raw<DOT, VARIANT>(q_j, x_r, n) of QT query vectors (LDS rows q + j ldq)
// against RT token rows per 8-lane group, every lane of a group returning the
// group's values.  All 64 lanes active, n wave-uniform.
//
// AVX-512 order at n >= 128 (exact_raw's acc5[8][16] loop): in the 8-lane
// layout lane sub owns acc5[2c + (sub >> 2)][4 (sub & 3) .. +3] for the four
// 32-element chunks c of a 128-element step, 16 accumulators per pair.  The
// tree of c/dot_avx512_amd64.c maps onto
//   acc5[2c+1] + acc5[2c]            xor 4 (both partners hold the sum)
//   (a2 + a0), (a6 + a4), a4 + a0    two in-lane adds over c, one more
//   acc[0][l] = acc5[0][l] + acc[0][l], then acc5[0][8+l] + acc[0][l]
//                                    r + 0.0f, then xor 2: lanes 0 and 1 hold
//                                    acc[0][0..3] and acc[0][4..7] of the AVX2
//                                    remainder, every other lane's accumulator
//                                    is zero as acc[1..3] are
// and the 32- / 8-element / scalar remainder and reduce_ymm4 follow as in AVX2.
template <int VARIANT, int QT, int RT>
__device__ __forceinline__ void mv_dots(const float* q, int ldq, const float* const (&x)[RT], int n, int sub,
                                        float (&out)[QT][RT]) {
    float4 acc[QT][RT];
    float sum[QT][RT];
#pragma unroll
    for (int j = 0; j < QT; j++)
#pragma unroll
        for (int r = 0; r < RT; r++) {
            acc[j][r] = make_float4(0.f, 0.f, 0.f, 0.f);
            sum[j][r] = 0.f;
        }
    int e = 0;
    if (n >= 8) {
        if (VARIANT == AVX512 && n >= 128) {
            float4 a5[QT][RT][4];
#pragma unroll
            for (int j = 0; j < QT; j++)
#pragma unroll
                for (int r = 0; r < RT; r++)
#pragma unroll
                    for (int c = 0; c < 4; c++) a5[j][r][c] = make_float4(0.f, 0.f, 0.f, 0.f);
            do {
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    float4 b[RT], av[QT];
#pragma unroll
                    for (int r = 0; r < RT; r++) b[r] = ld4(x[r] + e + 32 * c + 4 * sub);
#pragma unroll
                    for (int j = 0; j < QT; j++) av[j] = ld4(q + j * ldq + e + 32 * c + 4 * sub);
#pragma unroll
                    for (int j = 0; j < QT; j++)
#pragma unroll
                        for (int r = 0; r < RT; r++) a5[j][r][c] = mv_fma4(a5[j][r][c], av[j], b[r]);
                }
                e += 128;
            } while (n - e >= 128);
#pragma unroll
            for (int j = 0; j < QT; j++)
#pragma unroll
                for (int r = 0; r < RT; r++) {
                    float p[4][4];
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const float4 v = a5[j][r][c];
                        p[c][0] = lane_xor4(v.x) + v.x;
                        p[c][1] = lane_xor4(v.y) + v.y;
                        p[c][2] = lane_xor4(v.z) + v.z;
                        p[c][3] = lane_xor4(v.w) + v.w;
                    }
                    float t[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const float a0 = p[1][i] + p[0][i];
                        const float a4 = p[3][i] + p[2][i];
                        const float res = a4 + a0;
                        t[i] = lane_xor2(res) + (res + 0.f);
                    }
                    if (sub < 2) acc[j][r] = make_float4(t[0], t[1], t[2], t[3]);
                }
        }
        // rows of the next chunk are loaded before the current chunk's FMAs
        float4 b[RT];
        if (n - e >= 32) {
#pragma unroll
            for (int r = 0; r < RT; r++) b[r] = ld4(x[r] + e + 4 * sub);
        }
        for (; n - e >= 32; e += 32) {
            float4 bn[RT];
            if (n - e >= 64) {
#pragma unroll
                for (int r = 0; r < RT; r++) bn[r] = ld4(x[r] + e + 32 + 4 * sub);
            } else {
#pragma unroll
                for (int r = 0; r < RT; r++) bn[r] = b[r];
            }
            float4 av[QT];
#pragma unroll
            for (int j = 0; j < QT; j++) av[j] = ld4(q + j * ldq + e + 4 * sub);
#pragma unroll
            for (int j = 0; j < QT; j++)
#pragma unroll
                for (int r = 0; r < RT; r++) acc[j][r] = mv_fma4(acc[j][r], av[j], b[r]);
#pragma unroll
            for (int r = 0; r < RT; r++) b[r] = bn[r];
        }
        for (; n - e >= 8; e += 8) {
            if (sub < 2) {
                float4 bt[RT];
#pragma unroll
                for (int r = 0; r < RT; r++) bt[r] = ld4(x[r] + e + 4 * sub);
#pragma unroll
                for (int j = 0; j < QT; j++) {
                    const float4 av = ld4(q + j * ldq + e + 4 * sub);
#pragma unroll
                    for (int r = 0; r < RT; r++) acc[j][r] = mv_fma4(acc[j][r], av, bt[r]);
                }
            }
        }
    }
    for (; e < n; e++) {
        float bt[RT];
#pragma unroll
        for (int r = 0; r < RT; r++) bt[r] = x[r][e];
#pragma unroll
        for (int j = 0; j < QT; j++) {
            const float av = q[j * ldq + e];
#pragma unroll
            for (int r = 0; r < RT; r++) sum[j][r] = fmaf(av, bt[r], sum[j][r]);
        }
    }
#pragma unroll
    for (int j = 0; j < QT; j++)
#pragma unroll
        for (int r = 0; r < RT; r++) {
            float v = sum[j][r];
            if (n >= 8) {  // reduce_ymm4 over the 8 lanes, as exact_dist8
                float4 p = acc[j][r];
                p.x = p.x + lane_xor2(p.x); p.y = p.y + lane_xor2(p.y);
                p.z = p.z + lane_xor2(p.z); p.w = p.w + lane_xor2(p.w);
                p.x = p.x + lane_xor4(p.x); p.y = p.y + lane_xor4(p.y);
                p.z = p.z + lane_xor4(p.z); p.w = p.w + lane_xor4(p.w);
                float h = (p.x + p.y) + (p.z + p.w);
                h = h + lane_xor1(h);
                v = v + h;
            }
            out[j][r] = v;
        }
}

template <int VARIANT, int QT, int RT>
__global__ __launch_bounds__(256) void k_mv_maxsim(const MvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mv_lds[];
    __shared__ float red[4];
    __shared__ float dsum[LIST_CHUNK];  // the documents' running sums across the query tiles
    float* qsm = reinterpret_cast<float*>(mv_lds);  // [qtile][dpad]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = lane & 7, grp = lane >> 3;
    const ListPiece pc = a.pieces[blockIdx.x];
    const ListQuery lq = a.lq[pc.lq];
    const MvSpan qs = a.qspan[lq.q];
    const uint32_t* __restrict__ slots = a.pool + lq.pool_begin + pc.first;
    const int d = a.d, dpad = a.dpad, c4 = dpad >> 2;
    const int count = pc.count < LIST_CHUNK ? pc.count : LIST_CHUNK;
    const uint32_t myslot = tid < count ? slots[tid] : 0u;
    const bool mypres = tid < count && ((a.present[myslot >> 5] >> (myslot & 31u)) & 1u);
    dsum[tid] = 0.f;
    for (int q0 = 0; q0 < qs.len; q0 += a.qtile) {
        const int nqt = qs.len - q0 < a.qtile ? qs.len - q0 : a.qtile;
        const int nqp = (nqt + QT - 1) / QT * QT;  // <= qtile: a multiple of QT
        __syncthreads();  // the previous tile's readers are done (and dsum is initialised)
        const float4* __restrict__ qsrc = reinterpret_cast<const float4*>(a.Q + (qs.begin + q0) * dpad);
        for (int i = tid; i < nqp * c4; i += 256) {
            const int j = i / c4, c = i - j * c4;
            reinterpret_cast<float4*>(qsm)[i] = qsrc[(int64_t)(j < nqt ? j : nqt - 1) * c4 + c];
        }
        __syncthreads();
        for (int doc = wave; doc < count; doc += 4) {  // wave-uniform
            const uint32_t slot = slots[doc];
            if (!((a.present[slot >> 5] >> (slot & 31u)) & 1u)) continue;
            const MvSpan dc = a.docs[slot];
            const float* __restrict__ Td = a.T + dc.begin * dpad;
            float sum = dsum[doc];
            for (int qg = 0; qg < nqp; qg += QT) {
                float mq[QT];
#pragma unroll
                for (int j = 0; j < QT; j++) mq[j] = MV_MAXF;
                for (int r0 = 0; r0 < dc.len; r0 += 8 * RT) {
                    const float* x[RT];
#pragma unroll
                    for (int r = 0; r < RT; r++) {
                        const int row = r0 + 8 * r + grp;
                        x[r] = Td + (int64_t)(row < dc.len ? row : dc.len - 1) * dpad;
                    }
                    float dots[QT][RT];
                    mv_dots<VARIANT, QT, RT>(qsm + qg * dpad, dpad, x, d, sub, dots);
#pragma unroll
                    for (int j = 0; j < QT; j++)
#pragma unroll
                        for (int r = 0; r < RT; r++) {
                            const float dist = -dots[j][r];
                            if (dist < mq[j]) mq[j] = dist;
                        }
                }
#pragma unroll
                for (int j = 0; j < QT; j++) {
#pragma unroll
                    for (int m = 8; m < 64; m <<= 1) {
                        const float o = __shfl_xor(mq[j], m);
                        if (o < mq[j]) mq[j] = o;
                    }
                    if (qg + j < nqt) sum = sum + mq[j];
                }
            }
            if (lane == 0) dsum[doc] = sum;
        }
    }
    __syncthreads();
    ListDistArgs la{};
    la.Ec = a.Ec;
    la.Bc = a.Bc;
    la.Ab = a.Ab;
    list_emit(la, lq.e_begin + pc.first, mypres ? dsum[tid] : __builtin_inff(), mypres, red);
}

}  // namespace
}  // namespace wv
