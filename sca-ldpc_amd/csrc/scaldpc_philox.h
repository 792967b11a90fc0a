// Philox4x32-10 (Salmon et al., SC'11), counter-based, keyed by the seed: the generator of every device-side Monte-Carlo
// helper (K6 in scaldpc_bp_kernels.h, k_q_mc_draw in scaldpc_qary_mc.h).  counter = (block, stream, trial_lo, trial_hi) with
// the GLOBAL trial index; the four output words of block x >> 2 are the words of positions x & ~3 .. x | 3.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct U4 { unsigned x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

}  // namespace
