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
#include "scaldpc_mc_draw.h"  // mc_hqc_outcome_body: one text for k_mc_hqc_outcome, this kernel and their list forms

typedef unsigned long long u64;

namespace {

constexpr int TW = 64;  // codewords per tile = one wavefront of lanes (scaldpc_bp_kernels.h)

// The sibling of k_mc_hqc_outcome for the float64 decode: the same words, thresholds, outcome rule, reported bits, counters and
// export -- the trial does not know the decode's precision -- and per (tile, check) one 512-B row of the ratio plane
// double [tile][R][64] that Ratio64 reads, r = probs[k] / (1 - probs[k]) of the outcome drawn (McHqcLaw64: formed on the host in
// double).  The lanes of a ragged last tile get bit 0 and ratio 0, as k_ratio64_convert leaves them, and report nothing.
//   synd   u64 [tile][R]  in: the true bits c = Hin y; out: the reported bits c ^ flips[outcome]
//   acc_flips / acc_cost  int [batch], zeroed by the caller (acc_cost may be null); out_outcome  uint8 [batch][R] or null
// grid (ceil(R/64), T), block 256: wave = (tile, 16 consecutive checks), lane = trial.  (The contiguous form, slot b = trial
// first + b; the list form of scaldpc_mc_hqc_run_stats_at_f64 is scaldpc_bp_mc_at.hip's.)
__global__ __launch_bounds__(256) void k_mc_hqc_outcome64(McHqcLaw64 law, u64 *synd, double *__restrict__ plane, int R, int batch,
                                                          long first, unsigned k0, unsigned k1, int *__restrict__ acc_flips,
                                                          int *__restrict__ acc_cost, uint8_t *__restrict__ out_outcome)
{
    mc_hqc_outcome_body(law, synd, plane, R, batch, scaldpc::TrialRange{first}, k0, k1, acc_flips, acc_cost, out_outcome);
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
