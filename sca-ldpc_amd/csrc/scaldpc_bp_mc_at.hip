// The list forms of the binary Monte-Carlo generators, for the entries that decode chosen trials (scaldpc_mc_fer_run_at,
// scaldpc_mc_hqc_run_stats_at and their _f64 twins; host side in scaldpc_bp.hip): slot b of a call is trial ids[b], read from a
// device copy of the caller's list, where the contiguous kernels form first + b.  The bodies are the contiguous kernels' own
// (scaldpc_mc_draw.h) over a TrialList, so the launch shapes, layouts and every drawn word are theirs: see k_mc_bernoulli,
// k_mc_hqc_secret, k_mc_hqc_outcome (scaldpc_bp_kernels.h) and k_mc_hqc_outcome64 (scaldpc_bp_mc64.hip).  ids holds `batch`
// entries; the lanes of a ragged last tile do not read it.
//
// A translation unit of its own, behind four launch functions, for scaldpc_bp_mc64.hip's reason: the code objects the
// contiguous entries run from keep the kernels they had, in the order they had them.
#include "scaldpc_common.h"
#include "scaldpc_mc_draw.h"

typedef unsigned long long u64;

namespace {

using scaldpc::TrialList;

template <bool XOR_INTO>
__global__ __launch_bounds__(256) void k_mc_bernoulli_at(u64 *__restrict__ planes, int len, int batch, const long long *__restrict__ ids,
                                                         unsigned stream, unsigned k0, unsigned k1, const u64 *__restrict__ thr,
                                                         u64 thr0)
{
    mc_bernoulli_body<XOR_INTO>(planes, len, batch, TrialList{ids}, stream, k0, k1, thr, thr0);
}

__global__ __launch_bounds__(64) void k_mc_hqc_secret_at(u64 *__restrict__ planes, int n, int N, int omega, int batch,
                                                         const long long *__restrict__ ids, unsigned k0, unsigned k1,
                                                         int *__restrict__ out_y)
{
    extern __shared__ int chosen[];  // [omega][64]
    mc_hqc_secret_body(chosen, planes, n, N, omega, batch, TrialList{ids}, k0, k1, out_y);
}

__global__ __launch_bounds__(256) void k_mc_hqc_outcome_at(McHqcLaw law, u64 *synd, float *__restrict__ plane, int R, int batch,
                                                           const long long *__restrict__ ids, unsigned k0, unsigned k1,
                                                           int *__restrict__ acc_flips, int *__restrict__ acc_cost,
                                                           uint8_t *__restrict__ out_outcome)
{
    mc_hqc_outcome_body(law, synd, plane, R, batch, TrialList{ids}, k0, k1, acc_flips, acc_cost, out_outcome);
}

__global__ __launch_bounds__(256) void k_mc_hqc_outcome64_at(McHqcLaw64 law, u64 *synd, double *__restrict__ plane, int R, int batch,
                                                             const long long *__restrict__ ids, unsigned k0, unsigned k1,
                                                             int *__restrict__ acc_flips, int *__restrict__ acc_cost,
                                                             uint8_t *__restrict__ out_outcome)
{
    mc_hqc_outcome_body(law, synd, plane, R, batch, TrialList{ids}, k0, k1, acc_flips, acc_cost, out_outcome);
}

}  // namespace

namespace scaldpc {

// planes [T][len]; thr [len] or null (then thr0 for every position)
int launch_mc_bernoulli_at(bool xor_into, u64 *planes, int len, int batch, int T, const long long *ids, unsigned stream, unsigned k0,
                           unsigned k1, const u64 *thr, u64 thr0, hipStream_t s)
{
    const dim3 grid((len + 63) / 64, T);
    if (xor_into)
        hipLaunchKernelGGL(k_mc_bernoulli_at<true>, grid, dim3(256), 0, s, planes, len, batch, ids, stream, k0, k1, thr, thr0);
    else
        hipLaunchKernelGGL(k_mc_bernoulli_at<false>, grid, dim3(256), 0, s, planes, len, batch, ids, stream, k0, k1, thr, thr0);
    SC_HIP(hipGetLastError());
    return 0;
}

// planes [T][n]; out_y [batch][omega] or null
int launch_mc_hqc_secret_at(u64 *planes, int n, int N, int omega, int batch, int T, const long long *ids, unsigned k0, unsigned k1,
                            int *out_y, hipStream_t s)
{
    hipLaunchKernelGGL(k_mc_hqc_secret_at, dim3(T), dim3(64), (size_t)omega * 64 * sizeof(int), s, planes, n, N, omega, batch, ids, k0,
                       k1, out_y);
    SC_HIP(hipGetLastError());
    return 0;
}

// T tiles of R checks each: synd [T][R], plane [T][R][64], acc_flips / acc_cost [batch], out_outcome [batch][R]
int launch_mc_hqc_outcome_at(const McHqcLaw &law, u64 *synd, float *plane, int R, int batch, int T, const long long *ids, unsigned k0,
                             unsigned k1, int *acc_flips, int *acc_cost, uint8_t *out_outcome, hipStream_t s)
{
    hipLaunchKernelGGL(k_mc_hqc_outcome_at, dim3((R + 63) / 64, T), dim3(256), 0, s, law, synd, plane, R, batch, ids, k0, k1, acc_flips,
                       acc_cost, out_outcome);
    SC_HIP(hipGetLastError());
    return 0;
}

int launch_mc_hqc_outcome64_at(const McHqcLaw64 &law, u64 *synd, double *plane, int R, int batch, int T, const long long *ids,
                               unsigned k0, unsigned k1, int *acc_flips, int *acc_cost, uint8_t *out_outcome, hipStream_t s)
{
    hipLaunchKernelGGL(k_mc_hqc_outcome64_at, dim3((R + 63) / 64, T), dim3(256), 0, s, law, synd, plane, R, batch, ids, k0, k1,
                       acc_flips, acc_cost, out_outcome);
    SC_HIP(hipGetLastError());
    return 0;
}

}  // namespace scaldpc
