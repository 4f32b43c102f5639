// l1_kernels.hip -- the manhattan (L1) all-rows kernel of the exact replay.
//
//   k_l1_rows    exact L1 distance of every stored row to each listed query,
//                plus the per-256-row block minima: the outputs of
//                k_exact_rows<MANHATTAN, .> (kernels.hip), bit for bit, in
//                run_replay's buffers.  k_replay_scan consumes them unchanged.
//
// The reference's L1 (distancer/manhattan.go:20-30) is one fp32 accumulator
// advanced in element order, sum = sum + |a[i] - b[i]|.  It is no bilinear
// form, so no MFMA and no block-key filter applies: a kernel spends the same
// v_sub_f32 + v_add_f32(|.|) per element pair for an approximate key as for
// the exact value, and this one computes the exact value once.
//
// Register tile: a workgroup serves one 256-row block and QT listed queries;
// a lane owns RT rows x QT queries = RT*QT independent accumulators, each
// advanced strictly in element order i = 0 .. d-1.  The ILP comes from the
// independent (query, row) pairs, never from splitting one pair's sum.  Per 4
// elements a lane issues RT global float4 loads (its rows, reused for the QT
// queries) and QT wave-uniform ds_read_b128 (the queries staged in LDS once per
// workgroup, reused for the RT rows) for 8*RT*QT VALU instructions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hip"

namespace wv {
namespace {

constexpr int L1_RT = 2;             // rows per lane
constexpr int L1_QT = 8;             // queries per workgroup
constexpr int L1_LDS_FLOATS = 4096;  // staged query elements per workgroup (16 KiB): d is chunked above 512

// acc + |q - x| as exactly v_sub_f32 then v_add_f32 with the |.| source modifier: each an IEEE fp32
// operation, the two roundings of the reference.  Written out because plain C++ here is SLP-packed by
// the compiler into v_pk_add_f32 plus separate sign masks -- the same values, more instructions.
__device__ __forceinline__ float l1_step(float acc, float q, float x) {
    float t;
    asm("v_sub_f32 %0, %1, %2" : "=v"(t) : "v"(q), "v"(x));
    asm("v_add_f32 %0, %1, |%2|" : "=v"(acc) : "v"(acc), "v"(t));
    return acc;
}
// one element of every accumulator of query f
#define WV_L1_STEP(C)                                                             \
    _Pragma("unroll") for (int j = 0; j < RT; j++) acc[j][f] = l1_step(acc[j][f], qv.C, xv[j].C)

template <int RT, int QT>
__global__ __launch_bounds__(EBLK / RT, 8) void k_l1_rows(const float* __restrict__ X, int dpad,
                                                       const uint32_t* __restrict__ valid, int64_t nslots,
                                                       const float* __restrict__ Q, int d, int dc,
                                                       const int32_t* __restrict__ qlist, int F, int64_t ld,
                                                       float* __restrict__ E, float* __restrict__ bmin) {
    constexpr int NT = EBLK / RT;  // lanes of the workgroup; lane t owns rows t, t + NT, ..
    constexpr int NW = NT / 64;
    static_assert(NT % 64 == 0 && QT <= 64, "whole waves; one lane per query writes the block minimum");
    __shared__ float red[NW][QT];
    extern __shared__ __attribute__((aligned(16))) float4 l1q[];  // [QT][dc / 4]: broadcast ds_read_b128
    const int dc4 = dc >> 2;
    const int FB = (F + QT - 1) / QT;
    const int fb = blockIdx.x % FB;  // the chunks of one row block run back to back: rows re-read from cache
    const int64_t blk = blockIdx.x / FB;
    const int tid = threadIdx.x;

    bool ok[RT];
    const float* xr[RT];
    bool any = false;
#pragma unroll
    for (int j = 0; j < RT; j++) {
        const int64_t s = blk * EBLK + j * NT + tid;
        ok[j] = s < nslots && ((valid[s >> 5] >> (s & 31)) & 1u);
        xr[j] = X + (ok[j] ? s : (int64_t)0) * dpad;  // absent rows read row 0 (nslots > 0) and are discarded
        any |= ok[j];
    }
    float acc[RT][QT];
#pragma unroll
    for (int j = 0; j < RT; j++)
#pragma unroll
        for (int f = 0; f < QT; f++) acc[j][f] = 0.f;

    // a block without a candidate row (deleted, or outside the allow list) computes nothing
    if (__syncthreads_or(any ? 1 : 0)) {
        const int d4 = (d + 3) & ~3;  // <= dpad: rows and prepared queries are allocated to dpad floats
        for (int c0 = 0; c0 < d4; c0 += dc) {
            const int n = min(dc, d4 - c0);  // floats of this chunk, a multiple of 4
            if (c0) __syncthreads();
            for (int i = tid; i < QT * (n >> 2); i += NT) {
                const int f = i / (n >> 2);
                const int c = (i - f * (n >> 2)) << 2;
                const int ff = fb * QT + f < F ? fb * QT + f : fb * QT;  // duplicate a real query, never written
                l1q[f * dc4 + (c >> 2)] = ld4(Q + (int64_t)qlist[ff] * dpad + c0 + c);
            }
            __syncthreads();
            // The loop stops at d: the zero padding of rows and queries is not relied on.
            const int nd = min(n, d - c0);  // elements of this chunk below d
            const int full = nd & ~3;
            // the row loads of step e + 4 are in flight while step e is computed
            float4 xn[RT];
            if (full) {
#pragma unroll
                for (int j = 0; j < RT; j++) xn[j] = ld4(xr[j] + c0);
            }
            for (int e = 0; e < full; e += 4) {
                float4 xv[RT];
#pragma unroll
                for (int j = 0; j < RT; j++) xv[j] = xn[j];
                if (e + 4 < full) {
#pragma unroll
                    for (int j = 0; j < RT; j++) xn[j] = ld4(xr[j] + c0 + e + 4);
                }
#pragma unroll
                for (int f = 0; f < QT; f++) {
                    const float4 qv = l1q[f * dc4 + (e >> 2)];
                    WV_L1_STEP(x);
                    WV_L1_STEP(y);
                    WV_L1_STEP(z);
                    WV_L1_STEP(w);
                }
            }
            const int rem = nd - full;  // 1..3 elements of the last float4 (only in the last chunk)
            if (rem) {
                float4 xv[RT];
#pragma unroll
                for (int j = 0; j < RT; j++) xv[j] = ld4(xr[j] + c0 + full);
#pragma unroll
                for (int f = 0; f < QT; f++) {
                    const float4 qv = l1q[f * dc4 + (full >> 2)];
                    WV_L1_STEP(x);
                    if (rem > 1) { WV_L1_STEP(y); }
                    if (rem > 2) { WV_L1_STEP(z); }
                }
            }
        }
    }

#pragma unroll
    for (int f = 0; f < QT; f++) {
        const int ff = fb * QT + f;
        float m = __builtin_inff();
#pragma unroll
        for (int j = 0; j < RT; j++) {
            const float e = ok[j] ? acc[j][f] : __builtin_inff();
            if (ff < F) E[(int64_t)ff * ld + blk * EBLK + j * NT + tid] = e;  // < ld: ld is whole blocks
            m = fminf(m, e);
        }
        for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) red[tid >> 6][f] = m;
    }
    __syncthreads();
    if (tid < QT) {
        const int ff = fb * QT + tid;
        float m = red[0][tid];
#pragma unroll
        for (int w = 1; w < NW; w++) m = fminf(m, red[w][tid]);
        if (ff < F) bmin[(int64_t)ff * (ld / EBLK) + blk] = m;
    }
}
#undef WV_L1_STEP

// Launch over F listed queries and ld / EBLK row blocks (nslots > 0).
inline hipError_t launch_l1_rows(hipStream_t s, const float* X, int dpad, const uint32_t* valid, int64_t nslots,
                                 const float* Q, int d, const int32_t* qlist, int F, int64_t ld, float* E,
                                 float* bmin) {
    const int d4 = (d + 3) & ~3;
    const int dc = d4 < L1_LDS_FLOATS / L1_QT ? d4 : L1_LDS_FLOATS / L1_QT;
    const unsigned grid = (unsigned)(((F + L1_QT - 1) / L1_QT) * (ld / EBLK));
    k_l1_rows<L1_RT, L1_QT><<<grid, EBLK / L1_RT, (size_t)L1_QT * dc * sizeof(float), s>>>(
        X, dpad, valid, nslots, Q, d, dc, qlist, F, ld, E, bmin);
    return hipGetLastError();
}

}  // namespace
}  // namespace wv
