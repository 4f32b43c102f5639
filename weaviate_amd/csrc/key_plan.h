// key_plan.h -- how a block-key pass splits the corpus into spans (host only,
// nothing from HIP).  A key kernel's grid is nqg query groups x nspans spans of
// slots_per_span ring slots (RB 32-row blocks each); search_qs (bf16 and int8
// keys), the PQ int8 keys and the BQ block minima all take their split here.
//
// The rule:
//   1. start from 256 / gcd(256, nqg) spans and double until nqg * nspans >= 256
//      (a workgroup per CU, the query groups of a span in whole XCD octets);
//   2. a positive `spans` option replaces that value;
//   3. raise to ceil(nslots / max_sps), max_sps = (2^32 - 512 * row_bytes) /
//      (RB * 32 * row_bytes): the kernels address a span's plane with 32-bit
//      buffer offsets from the 256-row tile its first slot lies in, so the
//      span's bytes plus that tile and one tile of slack stay below 4 GiB;
//   4. without a `spans` option, and when whole_rounds asks for it, round up to
//      a multiple of 256 / gcd(256, nqg): whole rounds of one workgroup per CU
//      (10M x 1024: 5 spans = 320 groups -> 8);
//   5. clamp to [1, nslots]; slots_per_span = ceil(nslots / nspans), and nspans
//      = ceil(nslots / slots_per_span) drops the spans left empty.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>

struct KeyPlan {
    int slots_per_span;
    int nspans;
};

// row_bytes: bytes per row of the plane the kernel streams (dpb8 for the int8
// planes, 2 * dpb for bf16)
inline KeyPlan key_plan(int nqg, int64_t nslots, int rb, int64_t row_bytes, int spans_opt, bool whole_rounds) {
    const int64_t unit = 256 / std::gcd<int64_t>(256, nqg);
    int64_t nspans = unit;
    while ((int64_t)nqg * nspans < 256) nspans *= 2;
    if (spans_opt > 0) nspans = spans_opt;
    const int64_t max_sps = ((1ll << 32) - 2 * 256ll * row_bytes) / ((int64_t)rb * 32 * row_bytes);
    nspans = std::max<int64_t>(nspans, (nslots + max_sps - 1) / max_sps);
    if (spans_opt <= 0 && whole_rounds) nspans = (nspans + unit - 1) / unit * unit;
    nspans = std::max<int64_t>(1, std::min<int64_t>(nspans, nslots));
    const int64_t sps = (nslots + nspans - 1) / nspans;
    return KeyPlan{(int)sps, (int)((nslots + sps - 1) / sps)};
}
