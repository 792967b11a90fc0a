// The device code the float64 Monte-Carlo sweeps add (scaldpc_mc_fer_run_f64, scaldpc_mc_hqc_run_f64, scaldpc_mc_hqc_run_stats_f64;
// host side in scaldpc_bp.hip): the outcome draw that writes the ratio plane, and the double twin of k_gather_prior for the
// hand-over of stragglers to dense tiles.  The trials themselves are drawn by the fp32 entries' own kernels (k_mc_bernoulli,
// k_mc_hqc_secret), and the decode is scaldpc_bp_ref64.h's.
//
// A translation unit of its own, behind two launch functions: a kernel added to scaldpc_bp.hip moves every kernel defined after
// it in that unit's code object (the template instantiations of the fp32 hot path among them), and this way the code object
// the fp32 entries run from is byte for byte what it was before these sweeps existed.
#include "scaldpc_common.h"
#include "scaldpc_mc_law.h"  // McHqcLaw64: the outcome table k_mc_hqc_outcome64 takes by value
#include "scaldpc_philox.h"

typedef unsigned long long u64;

namespace {

constexpr int TW = 64;  // codewords per tile = one wavefront of lanes (scaldpc_bp_kernels.h)

// The sibling of k_mc_hqc_outcome for the float64 decode: the same words, thresholds, outcome rule, reported bits, counters and
// export -- the trial does not know the decode's precision -- and per (tile, check) one 512-B row of the ratio plane
// double [tile][R][64] that Ratio64 reads, r = probs[k] / (1 - probs[k]) of the outcome drawn (McHqcLaw64: formed on the host in
// double).  The lanes of a ragged last tile get bit 0 and ratio 0, as k_ratio64_convert leaves them, and report nothing.
//   synd   u64 [tile][R]  in: the true bits c = Hin y; out: the reported bits c ^ flips[outcome]
//   acc_flips / acc_cost  int [batch], zeroed by the caller (acc_cost may be null); out_outcome  uint8 [batch][R] or null
// grid (ceil(R/64), T), block 256: wave = (tile, 16 consecutive checks), lane = trial.
__global__ __launch_bounds__(256) void k_mc_hqc_outcome64(McHqcLaw64 law, u64 *synd, double *__restrict__ plane, int R, int batch,
                                                          long first, unsigned k0, unsigned k1, int *__restrict__ acc_flips,
                                                          int *__restrict__ acc_cost, uint8_t *__restrict__ out_outcome)
{
    const int lane = threadIdx.x & 63;
    const int x0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const int t = blockIdx.y;
    if (x0 >= R) return;
    const long b = (long)t * TW + lane;
    const bool live = b < batch;
    const u64 trial = (u64)(first + b);
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
                double ratio = law.ratio[0];
                for (int k = 0; k + 1 < law.K; k++) {
                    const bool past = word >= (c ? law.t[1][k] : law.t[0][k]);
                    lv += past;
                    ratio = past ? law.ratio[k + 1] : ratio;
                    cost = past ? law.cost[k + 1] : cost;
                }
                const unsigned flip = live ? (law.flips >> lv) & 1u : 0u;
                const u64 m = __ballot(live && (c ^ flip));
                if (lane == 0) synd[row] = m;
                plane[row * TW + lane] = live ? ratio : 0.0;
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

// k_gather_prior for the ratio plane (double [tile][cols][64]): dst[t2][j][c2] = src[id>>6][j][id&63], id = ids[64 t2 + c2];
// ratio 0 in the empty slots.  One 512-B row per (tile, column), lane = compact slot.  grid (ceil(cols/4), T2), block 256.
__global__ __launch_bounds__(256) void k_gather_prior64(const double *__restrict__ src, int cols, const int *__restrict__ ids,
                                                        double *__restrict__ dst)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t2 = blockIdx.y;
    if (j >= cols) return;
    const int id = ids[(size_t)t2 * TW + lane];
    dst[((size_t)t2 * cols + j) * TW + lane] = id >= 0 ? src[((size_t)(id >> 6) * cols + j) * TW + (id & 63)] : 0.0;
}

}  // namespace

namespace scaldpc {

// T tiles of R checks each: synd [T][R], plane [T][R][64], acc_flips / acc_cost [batch], out_outcome [batch][R]
int launch_mc_hqc_outcome64(const McHqcLaw64 &law, unsigned long long *synd, double *plane, int R, int batch, int T, long first,
                            unsigned k0, unsigned k1, int *acc_flips, int *acc_cost, uint8_t *out_outcome, hipStream_t s)
{
    hipLaunchKernelGGL(k_mc_hqc_outcome64, dim3((R + 63) / 64, T), dim3(256), 0, s, law, synd, plane, R, batch, first, k0, k1, acc_flips,
                       acc_cost, out_outcome);
    SC_HIP(hipGetLastError());
    return 0;
}

// T2 dense tiles: ids [T2][64], dst [T2][cols][64]; src is the call's plane, indexed by the ids
int launch_gather_prior64(const double *src, int cols, const int *ids, double *dst, int T2, hipStream_t s)
{
    hipLaunchKernelGGL(k_gather_prior64, dim3((cols + 3) / 4, T2), dim3(256), 0, s, src, cols, ids, dst);
    SC_HIP(hipGetLastError());
    return 0;
}

}  // namespace scaldpc
