// bq_packed.hip -- BQ block minima on the integer matrix cores straight from
// the packed codes (route WV_ROUTE_BQ_PACKED, option bq_pack).
// A translation unit of its own: quant_runtime.hip calls wv_bq_packmin().
//
// k_bq_packmin<QT> writes the 32-row hamming block minima of a group of
// 16 * QT queries, bmin[f * nblk + blk], from the word-major store
// codes[w * ccap + slot] and the word-major query codes -- any word count from
// 1 to 64, no plane beside the codes, nothing to do at Add.
//
// Arithmetic.  v_mfma_i32_16x16x64_i8 sums 64 int8 products per step: one
// code word.  The sum runs over K, so any assignment of code bits to K bytes
// serves as long as both operands use the same one, and the two operands need
// not be expanded alike:
//   row operand    bit x_r of dword j of a lane's 16 bytes -> x_r * 2^j   (0 / 1 / 2 / 4 / 8)
//   query operand  bit x_q of dword j                      -> (1 - 2 x_q) * (8 >> j)
// Every product is 8 x_r (1 - 2 x_q), so dot = 8 (pop(r) - 2 pop(r & q)) and
//   hamming(q, r) = pop(q) + pop(r) - 2 pop(r & q) = pop(q) + dot / 8,
// exact in int32 (|dot| <= 8 * 4096).  pop(q) is a constant of the query, so
// the minimum over a block's rows is taken on dot and corrected once.  Padding
// bits are 0 in both codes: x_r = 0 contributes nothing.  Against the
// symmetric +-1 expansion this makes the row operand -- the one expanded in
// the inner loop -- one v_and_b32 per dword after a 3-op nibble spread
// (7 VALU ops per fragment instead of 12 or more); against a 0 / 1 expansion
// of both it needs no per-row popcount.
//
// Operand layout.  Lane l of the MFMA holds 16 K bytes of row (or query)
// l & 15: the bytes of K group g = l >> 4.  Here a K step is not one code word
// but one 16-bit slice of four: in step k of word chunk c (words 4c .. 4c+3)
// lane (i, g) holds slice k of word 4c + g.  A lane therefore loads one whole
// 64-bit word of its row per chunk (one global_load_dwordx2, four 128-byte
// runs per wave) and feeds four MFMA steps from it.
//
// Work split.  A workgroup = one query group x a span of 32-row blocks.  The
// group's query operand is expanded ONCE per workgroup into LDS, in fragment
// order ([chunk][step][query tile][lane] x 16 bytes: ds_read_b128, no bank
// conflicts), so the inner loop expands rows only.  That is 64 bytes per
// (query, word): 16 * QT queries x 4 * chunks KB, 128 KB for 64 queries of
// <= 32 words (QT = 4) or 32 queries of <= 64 words (QT = 2).  Each of the 8
// waves owns two blocks (four 16-row tiles) per step and every query tile:
// 4 x QT accumulator tiles, a row fragment reused QT times, a query fragment
// 4 times.  The row words of the next PK_PF chunks are in flight in a register
// ring while a chunk's MFMAs run.  Epilogue per (block, query tile): minimum
// over the lane's valid rows, across the four K groups by two shuffles, one
// store per (query, block).  Query groups are the fast grid dimension, so the
// workgroups running together stream the same span of codes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dyn_lds.h"

namespace wv {
namespace {

typedef int pk_i32x4 __attribute__((ext_vector_type(4)));

constexpr int PK_WAVES = 8;  // waves per workgroup; a wave takes two 32-row blocks per step
constexpr int PK_THREADS = 64 * PK_WAVES;
constexpr int PK_STEP = 2 * PK_WAVES;  // blocks per workgroup step
constexpr int PK_PF = 4;               // word chunks in flight per wave

template <int QT>
__global__ __launch_bounds__(PK_THREADS) void k_bq_packmin(const uint64_t* __restrict__ codes, int64_t ccap, int words,
                                                           const uint32_t* __restrict__ valid, int64_t nslots,
                                                           const uint64_t* __restrict__ qcodes, int64_t ldq,
                                                           const int32_t* __restrict__ qlist, int nlist, int64_t nblk,
                                                           int64_t blk_per_span, float* __restrict__ bmin) {
    // dynamic LDS: the expanded query operand, [4 * nch * QT][64] x 16 bytes
    extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
    pk_i32x4* qx = reinterpret_cast<pk_i32x4*>(psm);
    __shared__ int s_pop[16 * QT];
    const int tid = threadIdx.x;
    const int lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nch = (words + 3) >> 2;
    const int f0 = blockIdx.x * (16 * QT);

    // the query operand: task = (query, K group, step, chunk) -> one lane's 16 bytes
    for (int t = tid; t < 16 * QT * 16 * nch; t += PK_THREADS) {
        const int qi = t % (16 * QT);
        const int r = t / (16 * QT);
        const int gg = r & 3, k = (r >> 2) & 3, c = r >> 4;
        const int w = 4 * c + gg;
        const int qr = qlist[f0 + qi < nlist ? f0 + qi : nlist - 1];
        const uint64_t qw = w < words ? qcodes[(int64_t)w * ldq + qr] : 0ull;
        const uint32_t s = (uint32_t)(qw >> (16 * k)) & 0xFFFFu;
        pk_i32x4 v;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t d = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int mag = 8 >> j;
                d |= (uint32_t)(uint8_t)(((s >> (4 * i + j)) & 1u) ? -mag : mag) << (8 * i);
            }
            v[j] = (int)d;
        }
        qx[((c * 4 + k) * QT + (qi >> 4)) * 64 + gg * 16 + (qi & 15)] = v;
    }
    if (tid < 16 * QT) {
        const int qr = qlist[f0 + tid < nlist ? f0 + tid : nlist - 1];
        int p = 0;
        for (int w = 0; w < words; w++) p += __popcll(qcodes[(int64_t)w * ldq + qr]);
        s_pop[tid] = p;
    }
    __syncthreads();

    const int64_t sb0 = (int64_t)blockIdx.y * blk_per_span;
    const int64_t sb1 = sb0 + blk_per_span < nblk ? sb0 + blk_per_span : nblk;
    const int64_t bfirst = sb0 + 2 * wave;  // the wave's block pairs: bfirst, bfirst + PK_STEP, ...
    const int nsteps = bfirst < sb1 ? (int)((sb1 - bfirst + PK_STEP - 1) / PK_STEP) : 0;
    const int T = nsteps * nch;  // (step, chunk) iterations of this wave
    if (nslots <= 0) {           // an empty store: every block +inf, no code is read
        for (int64_t i = tid; i < (sb1 - sb0) * 16 * QT; i += PK_THREADS) {
            const int f = f0 + (int)(i % (16 * QT));
            if (f < nlist) bmin[(int64_t)f * nblk + sb0 + i / (16 * QT)] = __builtin_inff();
        }
        return;
    }

    // word 4c + g of the lane's row in each of the pair's four 16-row tiles.
    // Branch-free, so the ring's loads are counted exactly (s_waitcnt vmcnt(n)
    // for the oldest chunk only): a word or row past the end reads a clamped
    // address (nslots > 0 here) and is zeroed.
    auto load_chunk = [&](int64_t b, int c, uint64_t (&x)[4]) {
        const int w = 4 * c + g;
        const int wc = w < words ? w : words - 1;
#pragma unroll
        for (int rt = 0; rt < 4; rt++) {
            const int64_t row = b * 32 + rt * 16 + c16;
            const uint64_t v = codes[(int64_t)wc * ccap + (row < nslots ? row : nslots - 1)];
            x[rt] = (w < words && row < nslots) ? v : 0ull;
        }
    };
    uint64_t ring[PK_PF][4];
    int64_t pb = bfirst;
    int pc = 0;
    auto issue = [&](uint64_t (&x)[4]) {  // past the wave's last pair: rows past nslots or a later pair's, unused
        load_chunk(pb < sb1 ? pb : sb1 - 1, pc, x);
        if (++pc == nch) { pc = 0; pb += PK_STEP; }
    };
#pragma unroll
    for (int u = 0; u < PK_PF; u++) issue(ring[u]);

    pk_i32x4 acc[4][QT];
    auto clear = [&]() {
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int qt = 0; qt < QT; qt++) acc[rt][qt] = pk_i32x4{0, 0, 0, 0};
    };
    // a pair's minima: acc[rt][qt][r] = dot of row 16 rt + 4 g + r and query 16 qt + c16
    auto epilogue = [&](int64_t b) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int64_t blk = b + h;
            if (blk >= sb1) break;
            uint32_t vw = blk * 32 < nslots ? valid[blk] : 0u;
            if (nslots - blk * 32 < 32) vw &= (1u << (nslots > blk * 32 ? (int)(nslots - blk * 32) : 0)) - 1u;
#pragma unroll
            for (int qt = 0; qt < QT; qt++) {
                int m = 0x7FFFFFFF;
#pragma unroll
                for (int t2 = 0; t2 < 2; t2++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if ((vw >> (t2 * 16 + 4 * g + r)) & 1u) m = min(m, acc[2 * h + t2][qt][r]);
                m = min(m, __shfl_xor(m, 16));
                m = min(m, __shfl_xor(m, 32));
                const int f = f0 + qt * 16 + c16;
                if (g == 0 && f < nlist)
                    bmin[(int64_t)f * nblk + blk] = m == 0x7FFFFFFF ? __builtin_inff() : (float)(s_pop[qt * 16 + c16] + (m >> 3));
            }
        }
    };

    clear();
    int64_t b = bfirst;
    int c = 0;
    for (int i0 = 0; i0 < T; i0 += PK_PF) {
#pragma unroll
        for (int u = 0; u < PK_PF; u++) {
            if (i0 + u >= T) break;
            uint32_t xl[4], xh[4];
#pragma unroll
            for (int rt = 0; rt < 4; rt++) {
                xl[rt] = (uint32_t)ring[u][rt];
                xh[rt] = (uint32_t)(ring[u][rt] >> 32);
            }
            issue(ring[u]);  // PK_PF chunks ahead, into the slot just read
#pragma unroll
            for (int k = 0; k < 4; k++) {
                pk_i32x4 Bq[QT];
#pragma unroll
                for (int qt = 0; qt < QT; qt++) Bq[qt] = qx[((c * 4 + k) * QT + qt) * 64 + lane];
#pragma unroll
                for (int rt = 0; rt < 4; rt++) {
                    // slice k of the word: its four nibbles one per byte, then bit j of every byte
                    const uint32_t s = ((k < 2 ? xl[rt] : xh[rt]) >> (16 * (k & 1))) & 0xFFFFu;
                    uint32_t y = (s | (s << 8)) & 0x00FF00FFu;
                    y = (y | (y << 4)) & 0x0F0F0F0Fu;
                    const pk_i32x4 A = {(int)(y & 0x01010101u), (int)(y & 0x02020202u), (int)(y & 0x04040404u),
                                        (int)(y & 0x08080808u)};
#pragma unroll
                    for (int qt = 0; qt < QT; qt++)
                        acc[rt][qt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, Bq[qt], acc[rt][qt], 0, 0, 0);
                }
            }
            if (++c == nch) {
                epilogue(b);
                clear();
                c = 0;
                b += PK_STEP;
            }
        }
    }
}

}  // namespace
}  // namespace wv

// Block minima of the listed queries [0, nlist) over blocks [0, nblk) of 32
// rows, 1 <= words <= 64.  Returns a hipError_t.
int wv_bq_packmin(hipStream_t s, const uint64_t* codes, int64_t ccap, int words, const uint32_t* valid, int64_t nslots,
                  const uint64_t* qcodes, int64_t ldq, const int32_t* qlist, int nlist, int64_t nblk, float* bmin) {
    using namespace wv;
    if (words < 1 || words > 64 || nlist < 1 || nblk < 1) return (int)hipErrorInvalidValue;
    const int nch = (words + 3) / 4;
    const int QT = nch <= 8 ? 4 : 2;  // the expanded query operand stays within 128 KB
    const size_t lds = (size_t)nch * 4 * QT * 1024;
    const int64_t qg = (nlist + 16 * QT - 1) / (16 * QT);
    // about 1024 workgroups (four rounds of one per CU), a span at least one
    // workgroup step and a whole number of block pairs
    const int64_t steps = (nblk + PK_STEP - 1) / PK_STEP;
    const int64_t spans = std::max<int64_t>(1, std::min<int64_t>(steps, (1024 + qg - 1) / qg));
    const int64_t bps = ((nblk + spans - 1) / spans + 1) / 2 * 2;
    const dim3 grid((unsigned)qg, (unsigned)((nblk + bps - 1) / bps));
#define WV_PK(QTV)                                                                                                \
    do {                                                                                                          \
        const int e = set_dyn_lds((const void*)k_bq_packmin<QTV>, lds);                                           \
        if (e != (int)hipSuccess) return e;                                                                       \
        k_bq_packmin<QTV><<<grid, PK_THREADS, lds, s>>>(codes, ccap, words, valid, nslots, qcodes, ldq, qlist, nlist, \
                                                        nblk, bps, bmin);                                         \
    } while (0)
    if (QT == 4) WV_PK(4);
    else WV_PK(2);
#undef WV_PK
    return (int)hipGetLastError();
}
