// sq_mfma.hip -- hnsw.flatSearch over the scalar quantizer on the integer
// matrix cores, without the B x N distance matrix.
//
// The SQ distance (DistanceBetweenCompressedVectors, scalar_quantization.go:
// 45-57) is a float expression of one exact integer, the byte dot product, and
// the per-vector sums {sum, sum2} of the codes.  With x' = x - 128, y' = y - 128
// as int8 (a second plane of the data codes, sq8_X; the u8 codes stay as they
// are),
//     sum x y = sum x'y' + 128 (Sx + Sy) - 16384 d
// exactly in int32 (d <= 4096), so one v_mfma_i32_16x16x64_i8 chain per 64
// columns is k_sq_dist's integer bit for bit.  Rows are padded to a multiple
// of 64 columns with zeros in both signed planes (a zero product), and the
// constant uses d, not the padded width.
//   k_sq_plane  the signed plane of a dirty slot range, 32-row tiles (rq_tile_u4)
//   k_sq_qprep  the encoded queries (sqq / sqm) -> signed rows, padded to 256
//   k_sq_keys   exact 32-row block minima of k_sq_dist's distance: k_rq8_keys'
//               ring as a body with a codec (i8_ring_keys, rq8_mfma.hip) and
//               SQ's side pieces and epilogue (SQ8Codec)
//   k_rq8_sel   (rq8_mfma.hip) M = the (R+1)-th smallest minimum, candidates
//   k_sq_cand   exact distances of the candidates' rows from the u8 codes as
//               k_sq_dist computes them; the R+1 smallest strictly increasing
//               -> the worker heap's ascending extraction, else oF[q] = 1 and
//               the query goes through the distance-matrix replay
// A translation unit of its own: its kernels compile beside quant_runtime.hip,
// which calls sq8_route() / sq8_candidates() / sq8_gather().
#include "rt_index.h"

namespace {

// 0x80 in the bytes of 16-byte chunk c that are real columns (< d)
__device__ __forceinline__ uint4 sq_sign_mask(int c, int d) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int left = d - (16 * c + 4 * j);  // real columns from this word on
        w[j] = left >= 4 ? 0x80808080u : left <= 0 ? 0u : (0x80808080u >> (8 * (4 - left)));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the signed plane of 32-row blocks [blk0, blk0 + nb): thread per (block,
// chunk of the padded row, row); chunks past the u8 row are zero
__global__ __launch_bounds__(256) void k_sq_plane(const uint4* __restrict__ codes, int nchq, int d, int64_t blk0,
                                                  int64_t nb, int nchp, uint4* __restrict__ plane) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nb * nchp * 32) return;
    const int64_t blk = blk0 + i / (32 * nchp);
    const int c = (int)((i >> 5) % nchp);
    const int64_t slot = blk * 32 + (i & 31);
    uint4 x = make_uint4(0u, 0u, 0u, 0u);
    if (c < nchq) {
        const uint4 m = sq_sign_mask(c, d);
        x = codes[((slot >> 8) * nchq + c) * 256 + (slot & 255)];
        x = make_uint4(x.x ^ m.x, x.y ^ m.y, x.z ^ m.z, x.w ^ m.w);
    }
    plane[rq_tile_u4(slot, c, nchp)] = x;
}

// query codes (group-tiled, RQ_QPB) -> row q of Qp ([nq_pad][16 nchp] int8) and
// {Sy, sum2_y}; rows past nq are zero.  Thread per (query, chunk).
__global__ __launch_bounds__(256) void k_sq_qprep(const uint4* __restrict__ qcodes, const uint2* __restrict__ qmeta,
                                                  int nchq, int d, int64_t nq, int64_t nq_pad, int nchp,
                                                  uint4* __restrict__ Qp, uint2* __restrict__ Qs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq_pad * nchp) return;
    const int64_t q = i / nchp;
    const int c = (int)(i % nchp);
    uint4 y = make_uint4(0u, 0u, 0u, 0u);
    if (q < nq && c < nchq) {
        const uint4 m = sq_sign_mask(c, d);
        y = qcodes[((q / RQ_QPB) * nchq + c) * RQ_QPB + q % RQ_QPB];
        y = make_uint4(y.x ^ m.x, y.y ^ m.y, y.z ^ m.z, y.w ^ m.w);
    }
    Qp[i] = y;
    if (c == 0) Qs[q] = q < nq ? qmeta[q] : make_uint2(0u, 0u);
}

struct SQ8Args {
    const unsigned char* plane;  // signed codes x' (32-row tiles of 16-byte chunks, rq_tile_u4), 64 NC bytes per row
    const uint2* meta;           // [cap] {Sx, sum2_x}
    const uint32_t* valid;       // [cap / 32] slots to scan
    const unsigned char* Qp;     // [nq_pad][64 NC] signed query codes, rows past nq zero
    const uint2* Qs;             // [nq_pad] {Sy, sum2_y}
    float* key;                  // [nq_pad][ldk] block minima
    int64_t ldk;
    int64_t nblk;                // 32-row blocks to scan
    int blocks_per_span;
    int nspans;
    int nqg;                     // query groups of 256
    int d;                       // real columns
    int cosine;                  // METRIC = DOT: 1 - t instead of -t
    float a2, ab, ib2;           // the quantizer's float32 constants (sq_set)
};

// ---------------------------------------------------------------------------
// sq_block_key<METRIC>: the epilogue of a 32-row block.  acc[m][n][r] is
// sum x'y' + 128 Sy of row 16m + 4g + r (g = lane >> 4) and query 16n +
// (lane & 15); the block's {Sx, sum2_x} (32 x 8 B) and valid word are in LDS at
// mb0 / vb.  out[n] = the minimum of k_sq_dist's distance over the block's valid
// rows for that query, in every lane; +inf for a block without one.
//   L2: l2 = sum2_x + sum2_y - 2 dot is an exact uint32; the integer minimum is
// kept and a2 * (float)l2 computed once: (float) of a uint32 and the product
// with a positive finite a2 are both non-decreasing.
//   dot / cosine: s = fl(fl(a2 (float)dot) + fl(ab (float)(Sx + Sy))) per row
// in k_sq_dist's order, unfused; the maximum is kept.  fl(s + ib2) is
// non-decreasing in s and fl(-t), fl(1 - t) non-increasing in t, so the
// block's minimum distance is that expression of the maximum s.  The host
// takes the route only where every such value is finite (sq8_route).
// ---------------------------------------------------------------------------
template <int METRIC>
__device__ __forceinline__ void sq_block_key(const i32x4_t (&acc)[2][2], unsigned mb0, unsigned vb,
                                             const uint2 (&ym)[2], const SQ8Args& a, int lane, float (&out)[2]) {
    const int g = lane >> 4;
    i32x4_t mt[2][2];  // mt[m][r >> 1]: {Sx, sum2_x} of rows r, r + 1
    const unsigned mb = mb0 + (unsigned)(g * 32);
    mt[0][0] = lds_ld16_o<0>(mb);
    mt[0][1] = lds_ld16_o<16>(mb);
    mt[1][0] = lds_ld16_o<128>(mb);
    mt[1][1] = lds_ld16_o<144>(mb);
    uint32_t vw0 = rq8_lds_ld4(vb);
    qs_wait_lgkm<0>();
    // the loaded registers are defined only after the wait: tie them to it
    asm volatile("" : "+v"(mt[0][0]), "+v"(mt[0][1]), "+v"(mt[1][0]), "+v"(mt[1][1]), "+v"(vw0));
    const uint32_t vw = __builtin_amdgcn_readfirstlane(vw0);
    const uint32_t mine = vw >> (4 * g);  // bit 16m + r: the lane's row (m, r)
    const int kd = 16384 * a.d;
    uint32_t pmin[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};  // (no l2 reaches it: l2 <= 255^2 d)
    float pmax[2] = {-__builtin_inff(), -__builtin_inff()};
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const bool ok = (mine >> (16 * m + r)) & 1u;
            const uint32_t sx = (uint32_t)mt[m][r >> 1][2 * (r & 1)];
            const uint32_t s2x = (uint32_t)mt[m][r >> 1][2 * (r & 1) + 1];
            const int kx = (int)(128u * sx) - kd;
#pragma unroll
            for (int n = 0; n < 2; n++) {
                const uint32_t dot = (uint32_t)(acc[m][n][r] + kx);
                if constexpr (METRIC == L2) {
                    const uint32_t l2 = s2x + ym[n].y - 2u * dot;
                    pmin[n] = min(pmin[n], ok ? l2 : 0xFFFFFFFFu);
                } else {
                    const float t = a.a2 * (float)dot;
                    const float u = a.ab * (float)(sx + ym[n].x);
                    const float s = t + u;
                    pmax[n] = fmaxf(pmax[n], ok ? s : -__builtin_inff());
                }
            }
        }
    // over the 4 row groups: lanes j, j + 16, j + 32, j + 48
#pragma unroll
    for (int n = 0; n < 2; n++) {
        if constexpr (METRIC == L2) {
            uint32_t v = pmin[n];
            v = min(v, (uint32_t)__shfl_xor((int)v, 32));
            v = min(v, (uint32_t)__shfl_xor((int)v, 16));
            out[n] = v == 0xFFFFFFFFu ? __builtin_inff() : a.a2 * (float)v;
        } else {
            float v = pmax[n];
            v = fmaxf(v, __shfl_xor(v, 32));
            v = fmaxf(v, __shfl_xor(v, 16));
            const float t = v + a.ib2;
            out[n] = v == -__builtin_inff() ? __builtin_inff() : (a.cosine ? 1.0f - t : -t);
        }
    }
}

template <int NC, int METRIC>
__global__ void k_sq_keys(SQ8Args a);

// SQ in i8_ring_keys (rq8_mfma.hip): behind a block's signed codes its 32
// {Sx, sum2_x} (256 B) and its valid word; the C input of the first chunk is
// 128 Sy, the epilogue (sq_block_key) adds 128 Sx - 16384 d; no debug bits
template <int METRIC>
struct SQ8Codec {
    static_assert(METRIC == L2 || METRIC == DOT, "l2-squared, or dot / cosine");
    typedef SQ8Args Args;
    template <int NC>
    static auto kernel() { return &k_sq_keys<NC, METRIC>; }  // (launch_ring_keys)
    static constexpr int SIDE = 2, META = 0, VALID = 256;
    static constexpr int slot_bytes(int NC) { return 32 * 64 * NC + VALID + 16; }
    typedef uint2 QMeta;
    static __device__ __forceinline__ const unsigned char* codes(const Args& a) { return a.plane; }
    static __device__ __forceinline__ int dbg(const Args&) { return 0; }
    static __device__ __forceinline__ void side(const Args& a, int64_t blk, int k, int lane, unsigned tail) {
        if (k == 0) {
            if (lane < 16)
                __builtin_amdgcn_global_load_lds(a.meta + blk * 32 + 2 * lane, (lds_ptr_t)(size_t)(tail + META), 16, 0, 0);
        } else {
            if (lane == 0) __builtin_amdgcn_global_load_lds(a.valid + blk, (lds_ptr_t)(size_t)(tail + VALID), 4, 0, 0);
        }
    }
    static __device__ __forceinline__ bool load_query(const Args& a, int64_t q0, int j, uint2 (&ym)[2],
                                                      i32x4_t (&C0)[2]) {
#pragma unroll
        for (int n = 0; n < 2; n++) {
            ym[n] = a.Qs[q0 + 16 * n + j];
            const int ky = (int)(128u * ym[n].x);
            C0[n] = i32x4_t{ky, ky, ky, ky};
        }
        return true;
    }
    static __device__ __forceinline__ void epilogue(const i32x4_t (&acc)[2][2], unsigned tail, const uint2 (&ym)[2], bool,
                                                    const Args& a, int, int lane, float (&out)[2]) {
        sq_block_key<METRIC>(acc, tail + META, tail + VALID, ym, a, lane, out);
    }
};

// k_sq_keys<NC, METRIC>: i8_ring_keys over the signed SQ plane, padded width
// 64 NC, at the ring depth sized for rq-8's larger slot (rq8_nbuf)
template <int NC, int METRIC>
__global__ __launch_bounds__(512, 2) void k_sq_keys(SQ8Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ssm[];
    i8_ring_keys<NC, SQ8Codec<METRIC>>(a, lds_addr(ssm));
}

// the SQ distance of stored row `slot` to one query as k_sq_dist computes it:
// v_dot4_u32_u8 over the u8 codes (256-row tiles) against the query's (qs, LDS)
__device__ __forceinline__ float sq_row_dist(const uint4* __restrict__ codes, const uint2* __restrict__ meta, int nchq,
                                             int64_t slot, const uint4* qs, const uint2& ym, int metric, float a2,
                                             float ab, float ib2) {
    const uint4* xr = codes + (slot >> 8) * nchq * 256 + (slot & 255);
    uint32_t acc = 0;
#pragma unroll 8
    for (int c = 0; c < nchq; c++) {
        const uint4 x = xr[(int64_t)c * 256];
        const uint4 y = qs[c];
        acc = __builtin_amdgcn_udot4(x.x, y.x, acc, false);
        acc = __builtin_amdgcn_udot4(x.y, y.y, acc, false);
        acc = __builtin_amdgcn_udot4(x.z, y.z, acc, false);
        acc = __builtin_amdgcn_udot4(x.w, y.w, acc, false);
    }
    const uint2 xm = meta[slot];
    if (metric == L2) {
        const uint32_t l2 = xm.y + ym.y - 2u * acc;
        return a2 * (float)l2;
    }
    float t = a2 * (float)acc;
    const float u = ab * (float)(xm.x + ym.x);
    t = t + u;
    t = t + ib2;
    return metric == DOT ? -t : 1.0f - t;
}

// ---------------------------------------------------------------------------
// k_sq_cand<RT>: wave per query (4 per block), skipped when k_rq8_sel flagged
// it (its list overflowed).  Lanes 0-31 / 32-63 take the rows of two candidate
// blocks at a time; their exact distances go to the wave's sorted list of
// 64 (RT - 1) >= R + 1.  The R + 1 smallest strictly increasing and finite:
// the worker heap keeps the R smallest whatever the insertion order and pops
// them in descending order, so the ascending list is its extraction -> ascI /
// ascD / ascN row q.  Otherwise oflag[q] = 1 (replayed).
// ---------------------------------------------------------------------------
template <int RT>
__global__ __launch_bounds__(256) void k_sq_cand(const uint4* __restrict__ codes, const uint2* __restrict__ meta, int nchq,
                                                 const uint32_t* __restrict__ valid, int64_t nslots,
                                                 const uint4* __restrict__ qcodes, const uint2* __restrict__ qmeta,
                                                 int64_t q_base, int metric, float a2, float ab, float ib2,
                                                 const uint32_t* __restrict__ cand, int Lc,
                                                 const int32_t* __restrict__ ncand, int nq, int R, uint64_t id_base,
                                                 uint64_t* __restrict__ ascI, float* __restrict__ ascD,
                                                 int32_t* __restrict__ ascN, int32_t* __restrict__ oflag) {
    extern __shared__ __attribute__((aligned(16))) uint4 cqs[];  // [4][nchq] query code bytes
    __shared__ float sbk[4][64];
    __shared__ uint32_t sbi[4][64];
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + w;
    if (q >= nq) return;
    if (oflag[q]) {
        if (lane == 0) ascN[q] = 0;
        return;
    }
    uint4* qs = cqs + w * nchq;
    const int64_t gq = q_base + q;
    for (int c = lane; c < nchq; c += 64) qs[c] = qcodes[((gq / RQ_QPB) * nchq + c) * RQ_QPB + gq % RQ_QPB];
    wave_sync_lds();
    const uint2 ym = qmeta[gq];
    const int nc = ncand[q];
    WaveTopL<RT> t;
    t.init();
    int nvalid = 0;
    bool odd = false;  // a NaN or an infinite distance of a valid row
    for (int i = 0; i < nc; i += 2) {
        const int bi = i + (lane >> 5);
        const bool has = bi < nc;
        const uint32_t blk = has ? cand[(int64_t)q * Lc + bi] : 0u;
        const int64_t slot = (int64_t)blk * 32 + (lane & 31);
        const bool ok = has && slot < nslots && ((valid[blk] >> (lane & 31)) & 1u);
        float dist = __builtin_inff();
        if (ok) {
            dist = sq_row_dist(codes, meta, nchq, slot, qs, ym, metric, a2, ab, ib2);
            odd = odd || !(fabsf(dist) < __builtin_inff());
        }
        nvalid += __popcll(__ballot(ok));
        t.offer(dist, (uint32_t)slot, sbk[w], sbi[w], lane);
    }
    t.merge(sbk[w], sbi[w], lane);
    const int nk = nvalid < R + 1 ? nvalid : R + 1;  // sorted entries that matter
    bool tie = false;
#pragma unroll
    for (int r = 0; r < RT - 1; r++) {
        const float nx0 = __shfl(t.key[r], (lane + 1) & 63);
        const float nx1 = r + 1 < RT - 1 ? __shfl(t.key[r + 1 < RT - 1 ? r + 1 : r], 0) : __builtin_inff();
        const float nx = lane < 63 ? nx0 : nx1;
        const int e = r * 64 + lane;
        tie = tie || (e + 1 < nk && t.key[r] == nx);
    }
    if (__any(tie) || __any(odd)) {
        if (lane == 0) {
            oflag[q] = 1;
            ascN[q] = 0;
        }
        return;
    }
    const int nout = nvalid < R ? nvalid : R;
#pragma unroll
    for (int r = 0; r < RT - 1; r++) {
        const int e = r * 64 + lane;
        if (e < nout) {
            ascI[(int64_t)q * R + e] = id_base + (uint64_t)t.id[r];
            ascD[(int64_t)q * R + e] = t.key[r];
        }
    }
    if (lane == 0) ascN[q] = nout;
}

// flagged queries' codes and {sum, sum2} (group-tiled) -> a compact copy for
// k_sq_dist: entry f = query list[f]; thread per (entry, 16-byte chunk)
__global__ void k_sq_gather_q(const uint4* __restrict__ qcodes, const uint2* __restrict__ qmeta, int nch,
                              const int32_t* __restrict__ list, int nf, uint4* __restrict__ ocodes,
                              uint2* __restrict__ ometa) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nf * nch) return;
    const int f = (int)(i / nch), c = (int)(i % nch);
    const int64_t q = list[f];
    ocodes[((int64_t)(f / RQ_QPB) * nch + c) * RQ_QPB + f % RQ_QPB] = qcodes[((q / RQ_QPB) * nch + c) * RQ_QPB + q % RQ_QPB];
    if (c == 0) ometa[f] = qmeta[q];
}

}  // namespace

// option sq_keys = -1: the batch sizes and corpus sizes where the route won the
// A/B by more than the same-arm spread in every measured cell (DESIGN §3.10c,
// profiles/sq_keys_ab.json): at a million rows from 256 queries on.  Below 256
// queries the outcome hangs on whether any query is flagged (the replay of one
// costs more than the whole key pass), at 500k rows it is a draw, below a loss.
static bool sq8_auto(int64_t nq, int64_t rows) { return nq >= 256 && rows >= 1000000; }

// SQ trained, 1 <= d <= 1024 (the query fragments stay in VGPRs), a worker heap
// the candidate lists hold, 256 key rows within rq8_chunk's 4 GiB, and
// constants under which every distance of the index is finite: a2 positive,
// and a2 255^2 d + |ab| 510 d + |ib2| below FLT_MAX -- then no NaN and no
// infinity can arise in k_sq_dist's expression, in either kernel
bool sq8_route(const wv_index* idx, int R, int64_t nq) {
    if (idx->compression != WV_COMPRESSION_SQ || !idx->sq_ready || idx->sq_keys == 0 || idx->dims < 1 ||
        idx->dims > 1024 || qs_R(R + 1) == 0 || idx->hiwater <= 0 || !metric_bilinear(idx->metric))
        return false;
    const double d = (double)idx->dims;
    const double big = (double)idx->sq_a2 * 65025.0 * d + fabs((double)idx->sq_ab) * 510.0 * d + fabs((double)idx->sq_ib2);
    if (!(idx->sq_a2 > 0.f) || !(big < 3.0e38)) return false;
    const int64_t nblk = (idx->hiwater + 31) / 32;
    if (256 * nblk * 4 > (4ll << 30)) return false;
    return idx->sq_keys == 1 || sq8_auto(nq, idx->hiwater);
}

// the signed plane up to date: (re)allocated with the index's capacity, the
// dirty slot range [sq8_lo, sq8_hi) rebuilt from the u8 codes in whole blocks
static int sq8_sync(wv_index* idx, hipStream_t s) {
    const int nchq = idx->sq_Dq / 16, nchp = (int)round_up(idx->dims, 64) / 16;
    int64_t lo = idx->sq8_lo, hi = idx->sq8_hi;
    if (idx->sq8_cap != idx->cap || !idx->sq8_X) {
        if (idx->sq8_X) hipFree(idx->sq8_X);
        idx->sq8_X = nullptr;
        idx->sq8_cap = 0;
        HIPCHK(hipMalloc(&idx->sq8_X, (size_t)idx->cap * nchp * 16));
        idx->sq8_cap = idx->cap;
        lo = 0;
        hi = idx->hiwater;
    }
    hi = std::min<int64_t>(hi, idx->hiwater);
    idx->sq8_lo = idx->sq8_hi = 0;
    if (hi <= lo) return WV_OK;
    const int64_t blk0 = lo / 32, nb = (hi + 31) / 32 - blk0;  // (cap is a multiple of 256: whole blocks exist)
    const int64_t chunk = (int64_t)1 << 16;                    // blocks per launch
    for (int64_t b = 0; b < nb; b += chunk) {
        const int64_t n = std::min<int64_t>(chunk, nb - b);
        k_sq_plane<<<(unsigned)((n * nchp * 32 + 255) / 256), 256, 0, s>>>(idx->sq_codes, nchq, idx->dims, blk0 + b, n,
                                                                           nchp, reinterpret_cast<uint4*>(idx->sq8_X));
    }
    HIPCHK(hipGetLastError());
    return WV_OK;
}

// exact SQ block minima -> candidate blocks -> exact distances of their rows:
// the worker heap's ascending extraction (ascI / ascD / ascN) of every query
// whose R + 1 smallest are strictly increasing, oF[q] = 1 for the others
int sq8_candidates(wv_index* idx, hipStream_t s, int64_t nq, int R, const uint32_t* valid) {
    int rc = sq8_sync(idx, s);
    if (rc) return rc;
    const int NC = (int)round_up(idx->dims, 64) / 64, DP = 64 * NC, nchq = idx->sq_Dq / 16;
    const int64_t nblk = (idx->hiwater + 31) / 32;
    const int RT = qs_R(R + 1);
    const int Lc = 64 * (RT - 1);
    const int64_t nq_pad = round_up(nq, 256);
    const int64_t QC = std::min<int64_t>(rq8_chunk(idx), nq_pad);
    HIPCHK(idx->rq8Qp.ensure((size_t)nq_pad * DP));
    HIPCHK(idx->rq8Qcs.ensure((size_t)nq_pad * sizeof(uint2)));
    HIPCHK(idx->qsKey.ensure((size_t)QC * nblk * sizeof(float)));
    HIPCHK(idx->qsCand.ensure((size_t)nq * Lc * sizeof(uint32_t)));
    HIPCHK(idx->qsNc.ensure((size_t)nq * sizeof(int32_t)));
    HIPCHK(idx->oF.ensure((size_t)nq * sizeof(int32_t)));
    unsigned char* Qp = idx->rq8Qp.as<unsigned char>();
    uint2* Qs = idx->rq8Qcs.as<uint2>();
    k_sq_qprep<<<(unsigned)((nq_pad * (DP / 16) + 255) / 256), 256, 0, s>>>(idx->sqq.as<uint4>(), idx->sqm.as<uint2>(), nchq,
                                                                            idx->dims, nq, nq_pad, DP / 16,
                                                                            reinterpret_cast<uint4*>(Qp), Qs);
    HIPCHK(hipGetLastError());
    const int metric = idx->metric == WV_METRIC_L2_SQUARED ? L2 : idx->metric == WV_METRIC_DOT ? DOT : COSINE;
    SQ8Args a{};
    a.plane = idx->sq8_X;
    a.meta = idx->sq_meta;
    a.valid = valid;
    a.key = idx->qsKey.as<float>();
    a.ldk = nblk;
    a.nblk = nblk;
    a.d = idx->dims;
    a.cosine = metric == COSINE;
    a.a2 = idx->sq_a2;
    a.ab = idx->sq_ab;
    a.ib2 = idx->sq_ib2;
    rc = ring_query_chunks(
        idx, s, nq, QC, 256, Lc, a,
        [&](int64_t c0, unsigned grid) {
            a.Qp = Qp + c0 * DP;
            a.Qs = Qs + c0;
            if (metric == L2) launch_ring_keys<SQ8Codec<L2>>(a, NC, grid, s);
            else launch_ring_keys<SQ8Codec<DOT>>(a, NC, grid, s);
            return WV_OK;
        },
        [&](int64_t c0, int64_t cn, unsigned gw, uint32_t* cand, int32_t* ncand, int32_t* of) {
            for_rt(RT, [&](auto rt) {
                constexpr int RTV = decltype(rt)::value;
                k_rq8_sel<RTV><<<gw, 256, 0, s>>>(a.key, nblk, nblk, (int)cn, R, cand, Lc, ncand, of, nullptr);
                k_sq_cand<RTV><<<gw, 256, (size_t)4 * idx->sq_Dq, s>>>(
                    idx->sq_codes, idx->sq_meta, nchq, valid, idx->hiwater, idx->sqq.as<uint4>(), idx->sqm.as<uint2>(), c0,
                    metric, a.a2, a.ab, a.ib2, cand, Lc, ncand, (int)cn, R, idx->id_base,
                    idx->ascI.as<uint64_t>() + c0 * R, idx->ascD.as<float>() + c0 * R, idx->ascN.as<int32_t>() + c0, of);
            });
        });
    if (rc) return rc;
    idx->stats.last_group_queries = (uint64_t)nq;
    idx->stats.mfma_launches++;
    idx->stats.last_route = WV_ROUTE_SQ_INT8;
    return WV_OK;
}

// the nf flagged queries' codes as a compact group for hnsw_dist's SQ arm
// (k_sq_dist reads queries by position): sq8Fq / sq8Fm, padded to RQ_QPB with zeros
int sq8_gather(wv_index* idx, hipStream_t s, const int32_t* list, int64_t nf) {
    if (nf <= 0) return WV_OK;
    const int nch = idx->sq_Dq / 16;
    const int64_t nf32 = round_up(nf, RQ_QPB);
    HIPCHK(idx->sq8Fq.ensure((size_t)nf32 * idx->sq_Dq));
    HIPCHK(idx->sq8Fm.ensure((size_t)nf32 * sizeof(uint2)));
    HIPCHK(hipMemsetAsync(idx->sq8Fq.p, 0, (size_t)nf32 * idx->sq_Dq, s));
    HIPCHK(hipMemsetAsync(idx->sq8Fm.p, 0, (size_t)nf32 * sizeof(uint2), s));
    k_sq_gather_q<<<(unsigned)((nf * nch + 255) / 256), 256, 0, s>>>(idx->sqq.as<uint4>(), idx->sqm.as<uint2>(), nch, list,
                                                                     (int)nf, idx->sq8Fq.as<uint4>(), idx->sq8Fm.as<uint2>());
    HIPCHK(hipGetLastError());
    return WV_OK;
}
