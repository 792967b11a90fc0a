// The bodies of the binary Monte-Carlo generators (K6 of scaldpc_bp_kernels.h; the float64 outcome draw of scaldpc_bp_mc64.hip),
// written once over the source of their trial indices (scaldpc_trials.h): the kernels of the contiguous entries pass a
// TrialRange, their list forms (scaldpc_bp_mc_at.hip) a TrialList.  Everything but the index a slot's Philox counter carries
// is the same text, so a list call and a contiguous call cannot draw differently.  What each body computes, its layouts and
// its launch shape are described at the kernels that call it.
#pragma once
#include <hip/hip_runtime.h>

#include "scaldpc_mc_law.h"
#include "scaldpc_philox.h"
#include "scaldpc_trials.h"

namespace {

constexpr int MC_LANES = 64;  // trials per tile = one wavefront of lanes (TW of scaldpc_bp_kernels.h)

template <bool XOR_INTO, class TR>
__device__ __forceinline__ void mc_bernoulli_body(unsigned long long *__restrict__ planes, int len, int batch, TR tr, unsigned stream,
                                                  unsigned k0, unsigned k1, const unsigned long long *__restrict__ thr,
                                                  unsigned long long thr0)
{
    typedef unsigned long long u64;
    const int lane = threadIdx.x & 63;
    const int x0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const int t = blockIdx.y;
    if (x0 >= len) return;
    const long b = (long)t * MC_LANES + lane;
    const u64 trial = tr.trial(b, b < batch);
    for (int q = 0; q < 4; q++) {
        const int xb = x0 + 4 * q;
        if (xb >= len) break;
        const U4 r = philox4x32_10(U4{(unsigned)(xb >> 2), stream, (unsigned)trial, (unsigned)(trial >> 32)}, k0, k1);
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int x = xb + j;
            if (x < len) {
                const u64 th = thr ? thr[x] : thr0;
                const u64 m = __ballot(b < batch && (u64)w[j] < th);
                if (lane == 0) {
                    if (XOR_INTO)
                        planes[(size_t)t * len + x] ^= m;
                    else
                        planes[(size_t)t * len + x] = m;
                }
            }
        }
    }
}

// chosen: the kernel's dynamic LDS, int [omega][64]
template <class TR>
__device__ __forceinline__ void mc_hqc_secret_body(int *chosen, unsigned long long *__restrict__ planes, int n, int N, int omega,
                                                   int batch, TR tr, unsigned k0, unsigned k1, int *__restrict__ out_y)
{
    typedef unsigned long long u64;
    const int lane = threadIdx.x, t = blockIdx.x;
    const long b = (long)t * MC_LANES + lane;
    if (b >= batch) return;
    const u64 trial = tr.trial(b, true);
    unsigned j = 0;
    U4 r{};
    for (int i = 0; i < omega; i++) {
        for (;;) {
            if ((j & 3) == 0) r = philox4x32_10(U4{j >> 2, 1u, (unsigned)trial, (unsigned)(trial >> 32)}, k0, k1);
            const unsigned w = (j & 3) == 0 ? r.x : (j & 3) == 1 ? r.y : (j & 3) == 2 ? r.z : r.w;
            j++;
            const int pos = (int)__umulhi(w, (unsigned)N);
            bool dup = false;
            for (int q = 0; q < i; q++) dup |= chosen[q * 64 + lane] == pos;
            if (!dup) {
                chosen[i * 64 + lane] = pos;
                atomicOr(planes + (size_t)t * n + pos, 1ull << lane);
                if (out_y) out_y[(size_t)b * omega + i] = pos;
                break;
            }
        }
    }
}

// LAW = McHqcLaw with plane values float (llr), or McHqcLaw64 with plane values double (ratio): McHqcPlane picks the table's row
template <class LAW>
struct McHqcPlane;
template <>
struct McHqcPlane<McHqcLaw> {
    typedef float value;
    static __device__ __forceinline__ float at(const McHqcLaw &law, int k) { return law.llr[k]; }
};
template <>
struct McHqcPlane<McHqcLaw64> {
    typedef double value;
    static __device__ __forceinline__ double at(const McHqcLaw64 &law, int k) { return law.ratio[k]; }
};

template <class LAW, class TR>
__device__ __forceinline__ void mc_hqc_outcome_body(const LAW &law, unsigned long long *synd,
                                                    typename McHqcPlane<LAW>::value *__restrict__ plane, int R, int batch, TR tr,
                                                    unsigned k0, unsigned k1, int *__restrict__ acc_flips, int *__restrict__ acc_cost,
                                                    uint8_t *__restrict__ out_outcome)
{
    typedef unsigned long long u64;
    typedef typename McHqcPlane<LAW>::value V;
    const int lane = threadIdx.x & 63;
    const int x0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const int t = blockIdx.y;
    if (x0 >= R) return;
    const long b = (long)t * MC_LANES + lane;
    const bool live = b < batch;
    const u64 trial = tr.trial(b, live);
    int nflips = 0, ncost = 0;
    for (int q = 0; q < 4; q++) {
        const int xb = x0 + 4 * q;
        if (xb >= R) break;
        const U4 r = philox4x32_10(U4{(unsigned)(xb >> 2), 0u, (unsigned)trial, (unsigned)(trial >> 32)}, k0, k1);
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int x = xb + j;
            if (x < R) {
                const size_t row = (size_t)t * R + x;
                const unsigned c = (unsigned)((synd[row] >> lane) & 1);
                const u64 word = w[j];
                int lv = 0, cost = law.cost[0];
                V val = McHqcPlane<LAW>::at(law, 0);
                for (int k = 0; k + 1 < law.K; k++) {
                    const bool past = word >= (c ? law.t[1][k] : law.t[0][k]);
                    lv += past;
                    val = past ? McHqcPlane<LAW>::at(law, k + 1) : val;
                    cost = past ? law.cost[k + 1] : cost;
                }
                const unsigned flip = live ? (law.flips >> lv) & 1u : 0u;
                const u64 m = __ballot(live && (c ^ flip));
                if (lane == 0) synd[row] = m;
                plane[row * MC_LANES + lane] = live ? val : (V)0;
                nflips += (int)flip;
                ncost += live ? cost : 0;
                if (out_outcome && live) out_outcome[(size_t)b * R + x] = (uint8_t)lv;
            }
        }
    }
    if (live) {
        atomicAdd(acc_flips + b, nflips);
        if (acc_cost) atomicAdd(acc_cost + b, ncost);
    }
}

}  // namespace
