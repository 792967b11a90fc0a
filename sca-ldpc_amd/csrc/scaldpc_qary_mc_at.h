// The list forms of the q-ary Monte-Carlo generators, for the entries that decode chosen trials (scaldpc_mc_qary_run_at,
// scaldpc_mc_qary_run_secret_at): slot b of a call is trial ids[b], read from a device copy of the caller's list, where
// k_q_mc_draw, k_q_mc_secret_draw and k_q_mc_secret_sums form first + b.  The bodies are those kernels' own over a TrialList
// (scaldpc_qary_mc.h, scaldpc_qary_secret.h): launch shapes, dynamic LDS, layouts and every drawn word are theirs.  ids holds
// `batch` entries; padding lanes (b >= batch) do not read it.  Included by scaldpc_qary.hip only, after every other kernel
// header, so the kernels of the contiguous entries keep their place in the code object.
#pragma once
#include "scaldpc_qary_mc.h"
#include "scaldpc_qary_secret.h"

namespace {

__global__ __launch_bounds__(256) void k_q_mc_draw_at(McLaw law, const float *__restrict__ tab, int Qb, int Qs, int BV, int N, int batch,
                                                      long Bp, const long long *__restrict__ ids, unsigned k0, unsigned k1,
                                                      const int *__restrict__ col_ptr, const int *__restrict__ csc_edge,
                                                      const int *__restrict__ edge_h, float *__restrict__ llr, float *__restrict__ msg,
                                                      int W, unsigned char *__restrict__ lvl)
{
    extern __shared__ float rows_at[];
    q_mc_draw_body(rows_at, law, tab, Qb, Qs, BV, N, batch, Bp, scaldpc::TrialList{ids}, k0, k1, col_ptr, csc_edge, edge_h, llr, msg, W, lvl);
}

__global__ __launch_bounds__(256) void k_q_mc_secret_draw_at(const unsigned long long *__restrict__ prior, const unsigned *__restrict__ law,
                                                             const float *__restrict__ tab, int K, int Q, int BV, int batch, long Bp,
                                                             const long long *__restrict__ ids, unsigned k0, unsigned k1,
                                                             const int *__restrict__ col_ptr, const int *__restrict__ csc_edge,
                                                             const int *__restrict__ edge_h, float *__restrict__ llr,
                                                             float *__restrict__ msg, int W, unsigned char *__restrict__ lvl,
                                                             signed char *__restrict__ sec)
{
    extern __shared__ float secret_lds_at[];
    q_mc_secret_draw_body(secret_lds_at, prior, law, tab, K, Q, BV, batch, Bp, scaldpc::TrialList{ids}, k0, k1, col_ptr, csc_edge, edge_h,
                          llr, msg, W, lvl, sec);
}

__global__ __launch_bounds__(256) void k_q_mc_secret_sums_at(const unsigned *__restrict__ law, const float *__restrict__ tab, int K, int QS,
                                                             int Qb, int BV, int R, int batch, long Bp, const long long *__restrict__ ids,
                                                             unsigned k0, unsigned k1, const int *__restrict__ row_ptr,
                                                             const int *__restrict__ edge_var, const int *__restrict__ edge_h,
                                                             float *__restrict__ llr, float *__restrict__ msg, int W,
                                                             unsigned char *__restrict__ lvl, signed char *__restrict__ sec)
{
    extern __shared__ float secret_lds_at[];
    q_mc_secret_sums_body(secret_lds_at, law, tab, K, QS, Qb, BV, R, batch, Bp, scaldpc::TrialList{ids}, k0, k1, row_ptr, edge_var, edge_h,
                          llr, msg, W, lvl, sec);
}

}  // namespace
