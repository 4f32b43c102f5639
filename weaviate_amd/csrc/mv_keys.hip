// mv_keys.hip -- the matrix-core candidate pass of the multi-vector flat search
// (route WV_ROUTE_MV_KEYS): a cheap MaxSim key with a proven
// error bound for every (query, listed document), a cut, and the exact kernel
// (mv_kernels.hip) on the survivors only.
//
//   k_mv_planes    rows of T -> bf16 planes Th = bf16(T), Tl = bf16(T - Th)
//                  (round to nearest even, integer code) and the row's 2-norm,
//                  rounded up, summed in double.
//   k_mv_tmax      per document slot the largest row norm (NaN when any is NaN).
//   k_mv_qprep     per query cS = c(dpad, n_q) * sum_j |q_j|_2, rounded up, and
//                  the guard flag when the sum is outside [2^-60, 2^60].
//   k_mv_keys<NK>  Key(Q, D) = sum over the query's vectors of min over D's
//                  tokens of -(th qh + th ql + tl qh), on
//                  v_mfma_f32_32x32x16_bf16: tokens on M, query vectors on N.
//                  A workgroup of 4 waves takes one piece (one query, <= 256
//                  listed documents), waves take documents round-robin.  The
//                  query's vectors are split into bf16 hi / lo once per
//                  workgroup in LDS (rows padded by 16 bytes against bank
//                  conflicts, the count padded to 32 with copies of the last
//                  vector), in tiles of a.qtile vectors with the documents'
//                  partial sums carried in LDS.  A wave walks a document's
//                  token rows in tiles of 32: the A fragments are 16-byte loads
//                  from the row-major planes, kept in registers across the
//                  query groups when dpad == 16 NK (NK > 0), streamed per k-step
//                  otherwise (NK == 0).  The last, partial token tile re-reads
//                  the document's last row: a duplicate cannot change a minimum.
//                  Epilogue: in-lane minimum of the 16 negated values of the
//                  lane's query column, one cross-lane step (lane ^ 32), a
//                  running minimum across the token tiles in LDS.
//   k_mv_cut       one workgroup per query: tau = the (k+1)-th smallest
//                  Key + eps over the present entries (radix select on the
//                  float bits, LDS histograms), candidates = entries with
//                  Key - eps <= tau, compacted in ascending list position.
#pragma once

namespace wv {
namespace {

typedef short mvk_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mvk_f32x16 __attribute__((ext_vector_type(16)));

constexpr int MVK_PAD = 8;            // bf16 elements appended to every LDS query row
constexpr int MVK_QTILE_MAX = 256;    // query vectors per LDS tile, a multiple of 32
constexpr int MVK_MAX_DPAD = 1024;
constexpr int MVK_MAX_QV = 65536;     // query vectors per query the bound's sums are written for
constexpr float MVK_NORM_LO = 0x1p-60f, MVK_NORM_HI = 0x1p60f;
// products below the normal range may be flushed by the matrix cores: <= 3 dpad products of
// <= MVK_MAX_QV minima, 2^-126 each, is below 2^-98
constexpr float MVK_EPS_FLOOR = 0x1p-96f;
// why a query leaves the key route: the norm guard, a non-finite key, more candidates than slots (device);
// the k + 1 exact scores not pairwise distinct (host)
enum { MVK_FLAG_GUARD = 1, MVK_FLAG_NONFINITE = 2, MVK_FLAG_CAP = 4, MVK_FLAG_TIE = 8 };

__host__ __device__ __forceinline__ uint32_t mvk_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
__host__ __device__ __forceinline__ float mvk_float(uint32_t u) { return __builtin_bit_cast(float, u); }

// bf16 by round to nearest even; a NaN stays one
__host__ __device__ __forceinline__ uint32_t mvk_bf16(float f) {
    const uint32_t u = mvk_bits(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// x = hi + lo + r with |r| <= 2^-16 |x|: x - hi is exact in fp32
__host__ __device__ __forceinline__ void mvk_split(float x, uint32_t& hi, uint32_t& lo) {
    hi = mvk_bf16(x);
    lo = mvk_bf16(x - mvk_float(hi << 16));
}

// c(dpad, nqv) of eps = c tmax(D) sum_q |q|, DESIGN.md §3.13b: the split's residuals and the dropped lo lo
// term (3.01 2^-16), the matrix cores' fp32 sum of 3 dpad products in any order under any rounding mode
// (3.1 dpad 2^-23), the reference's dot product (dpad 2^-24), the two nqv-term sums; 1 % slack
__host__ __device__ __forceinline__ double mvk_c(int dpad, int64_t nqv) {
    const double c1 = 3.01 * 0x1p-16 + (double)dpad * (3.1 * 0x1p-23 + 0x1p-24);
    return 1.01 * (c1 + 2.02 * (double)nqv * 0x1p-24 * (1.0 + c1));
}
// the bound of one entry in fp32, erring upward: 2^-13 relative slack for its own roundings, the
// absolute floor, and 2^-22 |key| so that fl(key +- eps) stays outside [key - eps', key + eps']
__host__ __device__ __forceinline__ float mvk_eps(float cS, float tmax, float key) {
    return cS * tmax * 1.0001f + MVK_EPS_FLOOR + fabsf(key) * 0x1p-22f;
}
// float bits -> unsigned in the floats' order
__device__ __forceinline__ uint32_t mvk_ord(float f) {
    const uint32_t u = mvk_bits(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mvk_unord(uint32_t o) { return mvk_float((o >> 31) ? (o & 0x7FFFFFFFu) : ~o); }

// rows [row0, row1) of T: a wave per row
__global__ __launch_bounds__(256) void k_mv_planes(const float* __restrict__ T, int64_t row0, int64_t row1, int d,
                                                   int dpad, uint16_t* __restrict__ Th, uint16_t* __restrict__ Tl,
                                                   float* __restrict__ tnorm) {
    const int lane = threadIdx.x & 63;
    const int64_t row = row0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= row1) return;  // wave-uniform
    double ss = 0.0;
    for (int c = lane; c < dpad; c += 64) {
        const float v = c < d ? T[row * dpad + c] : 0.f;
        uint32_t hi, lo;
        mvk_split(v, hi, lo);
        Th[row * dpad + c] = (uint16_t)hi;
        Tl[row * dpad + c] = (uint16_t)lo;
        ss += (double)v * (double)v;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m);
    if (lane == 0) tnorm[row] = (float)sqrt(ss) * 1.000001f;
}

__global__ __launch_bounds__(256) void k_mv_tmax(const MvSpan* __restrict__ docs, int64_t nslots,
                                                 const float* __restrict__ tnorm, float* __restrict__ tmax) {
    const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (slot >= nslots) return;
    const MvSpan dc = docs[slot];
    float mx = 0.f;
    bool nan = false;
    for (int t = 0; t < dc.len; t++) {
        const float n = tnorm[dc.begin + t];
        if (n != n) nan = true;
        else if (n > mx) mx = n;
    }
    tmax[slot] = nan ? __builtin_nanf("") : mx;
}

// a workgroup per query of the batch
__global__ __launch_bounds__(256) void k_mv_qprep(const float* __restrict__ Q, const MvSpan* __restrict__ qspan, int d,
                                                  int dpad, float* __restrict__ cS, int32_t* __restrict__ flags) {
    __shared__ double part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MvSpan qs = qspan[blockIdx.x];
    double sum = 0.0;
    for (int j = wave; j < qs.len; j += 4) {  // wave-uniform
        const float* q = Q + (qs.begin + j) * dpad;
        double ss = 0.0;
        for (int c = lane; c < d; c += 64) ss += (double)q[c] * (double)q[c];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m);
        sum += sqrt(ss);
    }
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        const double S = (part[0] + part[1]) + (part[2] + part[3]);
        const bool ok = S >= (double)MVK_NORM_LO && S <= (double)MVK_NORM_HI;  // false for a NaN
        cS[blockIdx.x] = ok ? (float)(mvk_c(dpad, qs.len) * S) * 1.000001f : 0.f;
        flags[blockIdx.x] = ok ? 0 : MVK_FLAG_GUARD;
    }
}

struct MvKeyArgs {
    const uint32_t* pool;     // as MvArgs
    const ListQuery* lq;
    const ListPiece* pieces;
    const uint32_t* present;
    const MvSpan* docs;
    const uint16_t* Th;       // bf16 planes [rows][dpad]
    const uint16_t* Tl;
    const float* tmax;        // [slot]
    const float* Q;           // query vectors of the batch [rows][dpad] fp32
    const MvSpan* qspan;
    float* Kc;                // [entries] keys of this launch group
    uint64_t* Ab;             // [entries / 64] absent bits
    int32_t* flags;           // [batch row] MVK_FLAG_*
    int d, dpad;
    int qtile;                // query vectors per LDS tile, a multiple of 32, <= MVK_QTILE_MAX
};

__host__ __device__ __forceinline__ size_t mvk_lds_bytes(int qtile, int dpad) {
    return (size_t)qtile * (size_t)(dpad + MVK_PAD) * 2 * sizeof(uint16_t);
}

template <int NK>
__global__ __launch_bounds__(256, 2) void k_mv_keys(const MvKeyArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mvk_lds[];
    __shared__ float dsum[LIST_CHUNK];          // the documents' sums across the query tiles
    __shared__ float wmin[4][MVK_QTILE_MAX];    // per wave: the running minima of the tile's query vectors
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n32 = lane & 31, half = lane >> 5;
    const ListPiece pc = a.pieces[blockIdx.x];
    const ListQuery lq = a.lq[pc.lq];
    const MvSpan qs = a.qspan[lq.q];
    const uint32_t* __restrict__ slots = a.pool + lq.pool_begin + pc.first;
    const int d = a.d, dpad = a.dpad, c4 = dpad >> 2, ldq = dpad + MVK_PAD;
    const int nk = NK > 0 ? NK : dpad >> 4;
    uint16_t* qh = reinterpret_cast<uint16_t*>(mvk_lds);  // [qtile][ldq]
    uint16_t* ql = qh + (size_t)a.qtile * ldq;
    const int count = pc.count < LIST_CHUNK ? pc.count : LIST_CHUNK;
    const uint32_t myslot = tid < count ? slots[tid] : 0u;
    const bool mypres = tid < count && ((a.present[myslot >> 5] >> (myslot & 31u)) & 1u);
    int myflag = 0;
    if (mypres) {
        const float tm = a.tmax[myslot];
        if (!(tm >= MVK_NORM_LO && tm <= MVK_NORM_HI)) myflag = MVK_FLAG_GUARD;
    }
    dsum[tid] = 0.f;
    for (int q0 = 0; q0 < qs.len; q0 += a.qtile) {
        const int nqt = qs.len - q0 < a.qtile ? qs.len - q0 : a.qtile;
        const int nqp = (nqt + 31) & ~31;  // <= qtile
        __syncthreads();  // the previous tile's readers are done (and dsum is initialised)
        const float4* __restrict__ qsrc = reinterpret_cast<const float4*>(a.Q + (qs.begin + q0) * dpad);
        for (int i = tid; i < nqp * c4; i += 256) {
            const int j = i / c4, c = i - j * c4;
            const float4 v = qsrc[(int64_t)(j < nqt ? j : nqt - 1) * c4 + c];
            const float x[4] = {v.x, v.y, v.z, v.w};
            uint32_t hi[4], lo[4];
#pragma unroll
            for (int e = 0; e < 4; e++) mvk_split(4 * c + e < d ? x[e] : 0.f, hi[e], lo[e]);
            *reinterpret_cast<uint2*>(qh + j * ldq + 4 * c) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
            *reinterpret_cast<uint2*>(ql + j * ldq + 4 * c) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
        }
        __syncthreads();
        for (int doc = wave; doc < count; doc += 4) {  // wave-uniform
            const uint32_t slot = slots[doc];
            if (!((a.present[slot >> 5] >> (slot & 31u)) & 1u)) continue;
            const MvSpan dc = a.docs[slot];
            if (dc.len <= 0) continue;
            for (int j = lane; j < nqp; j += 64) wmin[wave][j] = __builtin_inff();
            for (int t0 = 0; t0 < dc.len; t0 += 32) {
                const int row = t0 + n32 < dc.len ? t0 + n32 : dc.len - 1;
                const uint16_t* __restrict__ ph = a.Th + (dc.begin + row) * dpad + 8 * half;
                const uint16_t* __restrict__ pl = a.Tl + (dc.begin + row) * dpad + 8 * half;
                mvk_bf16x8 ah[NK > 0 ? NK : 1], al[NK > 0 ? NK : 1];
                if constexpr (NK > 0) {
#pragma unroll
                    for (int c = 0; c < NK; c++) {
                        ah[c] = *reinterpret_cast<const mvk_bf16x8*>(ph + 16 * c);
                        al[c] = *reinterpret_cast<const mvk_bf16x8*>(pl + 16 * c);
                    }
                }
                for (int g = 0; g < nqp; g += 32) {
                    const uint16_t* bhp = qh + (g + n32) * ldq + 8 * half;
                    const uint16_t* blp = ql + (g + n32) * ldq + 8 * half;
                    mvk_f32x16 acc0, acc1;  // hi hi, and the two cross terms
#pragma unroll
                    for (int r = 0; r < 16; r++) acc0[r] = acc1[r] = 0.f;
                    if constexpr (NK > 0) {
#pragma unroll
                        for (int c = 0; c < NK; c++) {
                            const mvk_bf16x8 bh = *reinterpret_cast<const mvk_bf16x8*>(bhp + 16 * c);
                            const mvk_bf16x8 bl = *reinterpret_cast<const mvk_bf16x8*>(blp + 16 * c);
                            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[c], bh, acc0, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[c], bl, acc1, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[c], bh, acc1, 0, 0, 0);
                        }
                    } else {
#pragma unroll 2
                        for (int c = 0; c < nk; c++) {
                            const mvk_bf16x8 th = *reinterpret_cast<const mvk_bf16x8*>(ph + 16 * c);
                            const mvk_bf16x8 tl = *reinterpret_cast<const mvk_bf16x8*>(pl + 16 * c);
                            const mvk_bf16x8 bh = *reinterpret_cast<const mvk_bf16x8*>(bhp + 16 * c);
                            const mvk_bf16x8 bl = *reinterpret_cast<const mvk_bf16x8*>(blp + 16 * c);
                            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, bh, acc0, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, bl, acc1, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tl, bh, acc1, 0, 0, 0);
                        }
                    }
                    // the lane holds 16 token rows of query column g + n32; lane ^ 32 the other 16
                    float mn = __builtin_inff();
#pragma unroll
                    for (int r = 0; r < 16; r++) mn = fminf(mn, -(acc0[r] + acc1[r]));
                    mn = fminf(mn, __shfl_xor(mn, 32));
                    if (half == 0) wmin[wave][g + n32] = fminf(wmin[wave][g + n32], mn);
                }
            }
            float s = 0.f;
            for (int j = lane; j < nqt; j += 64) s += wmin[wave][j];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
            if (lane == 0) dsum[doc] += s;
        }
    }
    __syncthreads();
    const float key = mypres ? dsum[tid] : __builtin_inff();
    if (mypres && !(fabsf(key) < __builtin_inff())) myflag |= MVK_FLAG_NONFINITE;
    if (myflag) atomicOr(&a.flags[lq.q], myflag);
    const int64_t e = lq.e_begin + pc.first;
    a.Kc[e + tid] = key;
    const uint64_t ab = __ballot(!mypres);
    if (lane == 0) a.Ab[(e >> 6) + wave] = ab;
}

// the cut of listed query blockIdx.x of a launch group: cand[q][cap] slots in ascending list position,
// cnt[q] their number (above cap: MVK_FLAG_CAP).  A query flagged by the key pass gets no candidates.
__global__ __launch_bounds__(256) void k_mv_cut(const float* __restrict__ Kc, const uint64_t* __restrict__ Ab,
                                                const uint32_t* __restrict__ pool, const ListQuery* __restrict__ lqs,
                                                const float* __restrict__ tmax, const float* __restrict__ cS,
                                                int32_t* __restrict__ flags, int k1, int cap,
                                                uint32_t* __restrict__ cand, int32_t* __restrict__ cnt) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_need;
    __shared__ int s_all, wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ListQuery lq = lqs[blockIdx.x];
    const int64_t q = lq.q;
    if (flags[q]) {  // block-uniform: written by the key pass, before this launch
        if (tid == 0) cnt[q] = 0;
        return;
    }
    const float* __restrict__ Kq = Kc + lq.e_begin;
    const uint64_t* __restrict__ Aq = Ab + (lq.e_begin >> 6);
    const uint32_t* __restrict__ sl = pool + lq.pool_begin;
    const float cs = cS[q];
    // key and bound of present entry i
    auto entry = [&](int64_t i, float& key, float& eps) -> bool {
        if ((Aq[i >> 6] >> (i & 63)) & 1ull) return false;
        key = Kq[i];
        eps = mvk_eps(cs, tmax[sl[i]], key);
        return true;
    };
    // the k1-th smallest Key + eps: a byte of its ordered bits per pass, most significant first
    uint32_t prefix = 0, mask = 0, need = (uint32_t)k1;
    bool all = false;  // fewer than k1 present entries: every one is a candidate
    for (int pass = 3; pass >= 0; pass--) {
        hist[tid] = 0;
        __syncthreads();
        for (int64_t i = tid; i < lq.len; i += 256) {
            float key, eps;
            if (!entry(i, key, eps)) continue;
            const uint32_t u = mvk_ord(key + eps);
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> (8 * pass)) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t cum = 0;
            int b = 0;
            for (; b < 256; b++) {
                if (cum + hist[b] >= need) break;
                cum += hist[b];
            }
            s_all = b == 256;
            s_prefix = prefix | ((uint32_t)(b & 255) << (8 * pass));
            s_need = need - cum;
        }
        __syncthreads();
        all = s_all != 0;
        prefix = s_prefix;
        need = s_need;
        mask |= 0xFFu << (8 * pass);
        if (all) break;  // block-uniform
    }
    const float tau = all ? __builtin_inff() : mvk_unord(prefix);
    int base = 0;
    for (int64_t i0 = 0; i0 < lq.len; i0 += 256) {
        const int64_t i = i0 + tid;
        float key = 0.f, eps = 0.f;
        const bool keep = i < lq.len && entry(i, key, eps) && key - eps <= tau;
        const uint64_t bal = __ballot(keep);
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        int wbase = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            if (w < wave) wbase += wtot[w];
            tot += wtot[w];
        }
        const int pos = base + wbase + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && pos < cap) cand[q * cap + pos] = sl[i];
        base += tot;
        __syncthreads();
    }
    if (tid == 0) {
        cnt[q] = base;
        if (base > cap) atomicOr(&flags[q], MVK_FLAG_CAP);
    }
}

}  // namespace
}  // namespace wv
