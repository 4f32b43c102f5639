// rq8_wide.hip -- the rq-8 / rq-1 key pass above 1024 rotated dims
// (k_rq8_keys_cp, rq8_mfma.hip).  A translation unit of its own:
// it is compiled without the packed-fp32 VALU forms, so the shared epilogue
// (rq8_block_min) is element-wise scalar float code here, and its six
// instantiations compile beside quant_runtime.hip, which calls
// wv_rq8_keys_wide().
#include "rt_index.h"

template <int NP, int BITS>
static hipError_t launch_rq8_keys_cp(const RQ8Args& a, hipStream_t s) {
    constexpr int lds = RQ8_CP_NBUF * RQ8_CP_SLOT;  // the ring: above 64 KiB
    hipError_t e = (hipError_t)set_dyn_lds((const void*)k_rq8_keys_cp<NP, BITS>, lds);
    if (e != hipSuccess) return e;
    k_rq8_keys_cp<NP, BITS><<<(unsigned)(a.nqg * a.nspans), 64 * rq8_cp_waves(NP), lds, s>>>(a);
    return hipGetLastError();
}

int wv_rq8_keys_wide(const RQ8Args& a, hipStream_t s, int bits) {
    if (a.nc <= 16 || a.nc > 64 || (bits != 8 && bits != 1)) return (int)hipErrorInvalidValue;
    const int np = rq8_cp_parts(a.nc);
    if (bits == 8) return (int)(np == 2 ? launch_rq8_keys_cp<2, 8>(a, s) : np == 3 ? launch_rq8_keys_cp<3, 8>(a, s)
                                                                                   : launch_rq8_keys_cp<4, 8>(a, s));
    return (int)(np == 2 ? launch_rq8_keys_cp<2, 1>(a, s) : np == 3 ? launch_rq8_keys_cp<3, 1>(a, s)
                                                                    : launch_rq8_keys_cp<4, 1>(a, s));
}
