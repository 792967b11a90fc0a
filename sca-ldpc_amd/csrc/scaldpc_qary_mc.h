// Monte-Carlo trials of the q-ary decoders drawn on the device (scaldpc_mc_qary_run): the reference's q-ary sweep
// (simulate/decode.py:246-257) gives every symbol of an all-zero word one of a FEW pmf rows ("good" / "bad") and asks whether the
// decoder returns zero.  A call therefore needs no [batch][N][Q] input and no [batch][N] output:
//   k_q_mc_draw    per (variable, codeword) one Philox word picks a level of the variable's table; the level's LLR row (converted
//                  by k_q_into_llr_rows, once per table) goes to llr and to the variable's first messages -- what the conversion
//                  kernels of a plain call leave there for the materialised input, value for value
//   k_q_mc_result  per codeword: is every decided symbol 0, how many are not, how many variables drew another level than the last
// Trial law: include/scaldpc.h (scaldpc_mc_qary_run).  Included by scaldpc_qary.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include "scaldpc_philox.h"
#include "scaldpc_trials.h"

namespace {

constexpr int MC_MAX_LEVELS = 16;

// The cumulative thresholds of both tables (0: coefficient variables, 1: DecoderSpecial's row-sum variables) travel as kernel
// arguments: uniform, read through scalar loads.  A word draws the smallest level k with word < t[k]; t[K - 1] = 2^32.
struct McLaw {
    unsigned long long t[2][MC_MAX_LEVELS];
    int K[2];
};

// grid (ceil(N / 4), Bp / 64), block 256, dynamic LDS (K[0] * Qb + K[1] * Qs) floats.  lane = codeword; a block takes the four
// consecutive variables 4 blockIdx.x .. + 3 of one Philox block (counter (blockIdx.x, 0, trial)), one wave each: every wave calls
// the generator (some 80 integer instructions) and keeps its own word.  (One wave walking all four variables calls it once, but
// runs their four chains of dependent scalar loads -- col_ptr, csc_edge, edge_h -- and their stores one after the other: 17.3 us on
// config 4's graph at batch 1024, 22.1 us on DecoderN1280R512SW6 at batch 256, measured)
// tab: the tables' LLR rows, [K[0]][Qb] then [K[1]][Qs].  The variable index is uniform in a wave: its table, its edges and the
// mirroring where h < 0 are scalar; only the level differs from lane to lane (an LDS read).  Every store is 64 codewords wide.
// Padding lanes (b >= batch) get the all-zero rows the conversion kernels give them.
// The body is written over the source of the trial index (TR: scaldpc_trials.h); k_q_mc_draw is the contiguous form, slot b =
// trial first + b, and the list form of scaldpc_mc_qary_run_at is scaldpc_qary_mc_at.h's.
template <class TR>
__device__ __forceinline__ void q_mc_draw_body(float *rows, const McLaw &law, const float *__restrict__ tab, int Qb, int Qs, int BV, int N,
                                               int batch, long Bp, TR tr, unsigned k0, unsigned k1, const int *__restrict__ col_ptr,
                                               const int *__restrict__ csc_edge, const int *__restrict__ edge_h,
                                               float *__restrict__ llr, float *__restrict__ msg, int W,
                                               unsigned char *__restrict__ lvl)
{
    const int nb = law.K[0] * Qb, nt = nb + law.K[1] * Qs;
    for (int i = threadIdx.x; i < nt; i += 256) rows[i] = tab[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * 4 + j;
    if (x >= N) return;
    const long b = (long)blockIdx.y * 64 + lane;
    const bool live = b < batch;
    const unsigned long long trial = tr.trial(b, live);
    const U4 r = philox4x32_10(U4{blockIdx.x, 0u, (unsigned)trial, (unsigned)(trial >> 32)}, k0, k1);
    const unsigned long long word = j == 0 ? r.x : j == 1 ? r.y : j == 2 ? r.z : r.w;
    const int tb = x >= BV, Q = tb ? Qs : Qb, K = law.K[tb];
    int lv = 0;  // thresholds do not decrease: the smallest k with word < t[k] = the number of thresholds at or below the word
    for (int k = 0; k + 1 < K; k++) lv += word >= law.t[tb][k];
    const float *row = rows + (tb ? nb : 0) + lv * Q;
    const size_t r0 = tb ? (size_t)BV * Qb + (size_t)(x - BV) * Qs : (size_t)x * Qb;
    for (int q = 0; q < Q; q++) llr[(r0 + q) * Bp + b] = live ? row[q] : 0.0f;
    lvl[(size_t)x * Bp + b] = (unsigned char)(live ? lv : K - 1);
    for (int t = col_ptr[x]; t < col_ptr[x + 1]; t++) {  // decoder.rs:567-573: v2c = channel * h
        const int e = csc_edge[t];
        const bool rev = edge_h[e] < 0;
        for (int q = 0; q < Q; q++) msg[((size_t)e * W + q) * Bp + b] = live ? row[rev ? Q - 1 - q : q] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_q_mc_draw(McLaw law, const float *__restrict__ tab, int Qb, int Qs, int BV, int N, int batch,
                                                   long Bp, long first, unsigned k0, unsigned k1, const int *__restrict__ col_ptr,
                                                   const int *__restrict__ csc_edge, const int *__restrict__ edge_h,
                                                   float *__restrict__ llr, float *__restrict__ msg, int W,
                                                   unsigned char *__restrict__ lvl)
{
    extern __shared__ float rows[];
    q_mc_draw_body(rows, law, tab, Qb, Qs, BV, N, batch, Bp, scaldpc::TrialRange{first}, k0, k1, col_ptr, csc_edge, edge_h, llr, msg, W, lvl);
}

// hard: the staged symbols [N][Bp]; lvl: the drawn levels [N][Bp] (bytes both).  grid Bp / 64, block 1024 = the block's 64
// codewords x 64 variables a step: a thread reads FOUR codewords' bytes of one variable as one 32-bit word (16 lanes cover the
// 64 codewords, a wave four variables, the block v0 .. v0 + 63), counts per byte, and the 64 partial counts of every codeword are
// added through LDS by wave 0.  (One byte per lane and 16 variables a step took 5.8 us on config 4's 450 variables and 10.7 us
// on the Kyber decoder's 1280, more than the k_q_unpack it replaces: DESIGN.md 4.)  Padding codewords are read (they lie
// inside the planes) and not reported.  errs / wrong may be nullptr.  last_b / last_s: the last level of either table.
__global__ __launch_bounds__(1024) void k_q_mc_result(const signed char *__restrict__ hard, const unsigned char *__restrict__ lvl,
                                                      int N, int BV, int last_b, int last_s, int batch, long Bp,
                                                      unsigned char *__restrict__ success, int *__restrict__ errs,
                                                      int *__restrict__ wrong)
{
    __shared__ int part[2][64][64];  // [errs | wrong][variable slot][codeword]
    const int c4 = (threadIdx.x & 15) * 4, slot = threadIdx.x >> 4;
    const long b0 = (long)blockIdx.x * 64;
    int ne[4] = {0, 0, 0, 0}, nw[4] = {0, 0, 0, 0};
#pragma unroll 4
    for (int v = slot; v < N; v += 64) {
        const unsigned lw = *(const unsigned *)(lvl + (size_t)v * Bp + b0 + c4);  // (Bp and b0 are multiples of 64: aligned)
        const unsigned hw = *(const unsigned *)(hard + (size_t)v * Bp + b0 + c4);
        const unsigned last = v < BV ? last_b : last_s;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            ne[k] += ((lw >> (8 * k)) & 255u) != last;
            nw[k] += ((hw >> (8 * k)) & 255u) != 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        part[0][slot][c4 + k] = ne[k];
        part[1][slot][c4 + k] = nw[k];
    }
    __syncthreads();
    const long b = b0 + threadIdx.x;
    if (threadIdx.x >= 64 || b >= batch) return;
    int e = 0, w = 0;
    for (int i = 0; i < 64; i++) {
        e += part[0][i][threadIdx.x];
        w += part[1][i][threadIdx.x];
    }
    success[b] = w == 0;
    if (errs) errs[b] = e;
    if (wrong) wrong[b] = w;
}

}  // namespace
