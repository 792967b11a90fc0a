// Monte-Carlo trials of DecoderSpecial on DRAWN secrets (scaldpc_mc_qary_run_secret): the trial of the Kyber attack
// (simulate/kyber.py:95-105, 85-92, 362-376) -- a secret drawn from a prior, the row sums that follow from it and H, and per
// variable an oracle outcome drawn CONDITIONAL on the variable's true symbol, which hands the decoder a posterior pmf row.
//   k_q_mc_secret_draw    per (coefficient variable, codeword): stream-1 word -> the secret symbol (prior thresholds, uniform),
//                         stream-0 word -> the outcome (the thresholds of the lane's own symbol, LDS); secret, level, LLR row and
//                         first messages, as k_q_mc_draw leaves them
//   k_q_mc_secret_sums    per (row, codeword): t_r = -h_id * sum_j h_j s_j over the row's coefficient edges (the one value that
//                         makes the check hold over the integers), its outcome from stream-0 word N-R+r, its LLR row and the
//                         first message of its single edge
//   k_q_mc_secret_result  per codeword: decided != secret and (the drawn row's own decision) != secret, each split at N-R
// Trial law: include/scaldpc.h (scaldpc_mc_qary_run_secret).  Included by scaldpc_qary.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include "scaldpc_philox.h"
#include "scaldpc_trials.h"

namespace {

// One table of the law on the device, as both drawing kernels stage it in LDS next to the table's K LLR rows:
//   thr  unsigned [K][Q]  thr[k * Q + s]: threshold k of TRUE symbol s (lanes differ in s: neighbouring banks)
//   cnt  int      [Q]     the thresholds of s below 2^32 (a prefix: they do not decrease; at most K - 1, the last is 2^32) --
//                         2^32 itself does not fit the word, and a word is never at or above it
// The outcome of a word is the number of thresholds at or below it = the smallest k with word < T_k.
struct SecretTab {
    const float *rows;
    const unsigned *thr;
    const int *cnt;
    __device__ __forceinline__ int outcome(unsigned word, int s, int K, int Q) const
    {
        const int n = cnt[s];
        int lv = 0;
        for (int k = 0; k + 1 < K; k++) lv += (k < n) & (word >= thr[k * Q + s]);
        return lv;
    }
};

// dynamic LDS: K Q floats, K Q words, Q words (mc_secret_lds_bytes, scaldpc_mc_law.h).  law: thr then cnt, as above.
__device__ __forceinline__ SecretTab secret_stage(float *lds, const float *__restrict__ tab, const unsigned *__restrict__ law, int K, int Q)
{
    unsigned *thr = (unsigned *)(lds + K * Q);
    int *cnt = (int *)(thr + K * Q);
    for (int i = threadIdx.x; i < K * Q; i += 256) {
        lds[i] = tab[i];
        thr[i] = law[i];
    }
    for (int i = threadIdx.x; i < Q; i += 256) cnt[i] = (int)law[K * Q + i];
    __syncthreads();
    return SecretTab{lds, thr, cnt};
}

__device__ __forceinline__ unsigned word_of(const U4 &r, int j) { return j == 0 ? r.x : j == 1 ? r.y : j == 2 ? r.z : r.w; }

// grid (ceil(BV / 4), Bp / 64), block 256: lane = codeword, wave j takes coefficient variable x = 4 blockIdx.x + j, i.e. word j of
// Philox block blockIdx.x -- of stream 1 (the secret) and of stream 0 (the outcome, the word scaldpc_mc_qary_run draws x's level
// from): two generator calls per wave.  prior: Q cumulative thresholds (uniform: scalar loads).  sec [N][Bp]: the secret VALUES.
// Padding lanes (b >= batch): all-zero rows, secret 0, the last level.  Every store is 64 codewords wide.
// Both drawing kernels' bodies are written over the source of the trial index (TR: scaldpc_trials.h); the kernels here are the
// contiguous form, slot b = trial first + b, and the list forms of scaldpc_mc_qary_run_secret_at are scaldpc_qary_mc_at.h's.
template <class TR>
__device__ __forceinline__ void q_mc_secret_draw_body(float *secret_lds, const unsigned long long *__restrict__ prior,
                                                      const unsigned *__restrict__ law, const float *__restrict__ tab, int K, int Q, int BV,
                                                      int batch, long Bp, TR tr, unsigned k0, unsigned k1,
                                                      const int *__restrict__ col_ptr, const int *__restrict__ csc_edge,
                                                      const int *__restrict__ edge_h, float *__restrict__ llr, float *__restrict__ msg,
                                                      int W, unsigned char *__restrict__ lvl, signed char *__restrict__ sec)
{
    const SecretTab t = secret_stage(secret_lds, tab, law, K, Q);
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * 4 + j;
    if (x >= BV) return;
    const long b = (long)blockIdx.y * 64 + lane;
    const bool live = b < batch;
    const unsigned long long trial = tr.trial(b, live);
    const unsigned lo = (unsigned)trial, hi = (unsigned)(trial >> 32);
    const unsigned long long ws = word_of(philox4x32_10(U4{blockIdx.x, 1u, lo, hi}, k0, k1), j);
    const unsigned wo = word_of(philox4x32_10(U4{blockIdx.x, 0u, lo, hi}, k0, k1), j);
    int s = 0;  // the smallest q with word < prior[q] = the number of thresholds at or below the word (prior[Q - 1] = 2^32)
    for (int q = 0; q + 1 < Q; q++) s += ws >= prior[q];
    const int lv = t.outcome(wo, s, K, Q);
    const float *row = t.rows + lv * Q;
    const size_t r0 = (size_t)x * Q;
    for (int q = 0; q < Q; q++) llr[(r0 + q) * Bp + b] = live ? row[q] : 0.0f;
    lvl[(size_t)x * Bp + b] = (unsigned char)(live ? lv : K - 1);
    sec[(size_t)x * Bp + b] = (signed char)(live ? s - (Q - 1) / 2 : 0);
    for (int c = col_ptr[x]; c < col_ptr[x + 1]; c++) {  // decoder.rs:567-573: v2c = channel * h
        const int e = csc_edge[c];
        const bool rev = edge_h[e] < 0;
        for (int q = 0; q < Q; q++) msg[((size_t)e * W + q) * Bp + b] = live ? row[rev ? Q - 1 - q : q] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_q_mc_secret_draw(const unsigned long long *__restrict__ prior, const unsigned *__restrict__ law,
                                                          const float *__restrict__ tab, int K, int Q, int BV, int batch, long Bp,
                                                          long first, unsigned k0, unsigned k1, const int *__restrict__ col_ptr,
                                                          const int *__restrict__ csc_edge, const int *__restrict__ edge_h,
                                                          float *__restrict__ llr, float *__restrict__ msg, int W,
                                                          unsigned char *__restrict__ lvl, signed char *__restrict__ sec)
{
    extern __shared__ float secret_lds[];
    q_mc_secret_draw_body(secret_lds, prior, law, tab, K, Q, BV, batch, Bp, scaldpc::TrialRange{first}, k0, k1, col_ptr, csc_edge, edge_h,
                          llr, msg, W, lvl, sec);
}

// grid (ceil(R / 4), Bp / 64), block 256, after k_q_mc_secret_draw on the same stream: wave j takes row r = 4 blockIdx.x + j and
// its row-sum variable x = BV + r.  The row's edges are its coefficient edges and then the identity entry (creation holds H to
// [H' | I]): a scalar walk over edge_var / edge_h, 64 secret bytes per edge.  (degree - 1) B <= BSUM (creation), so t_r lies inside
// the alphabet; the clamp only keeps a broken plane from indexing past the table.  x's word is word x & 3 of stream-0 block
// x >> 2, whatever r is: the first rows share their block with the last coefficient variables.
template <class TR>
__device__ __forceinline__ void q_mc_secret_sums_body(float *secret_lds, const unsigned *__restrict__ law, const float *__restrict__ tab,
                                                      int K, int QS, int Qb, int BV, int R, int batch, long Bp, TR trials, unsigned k0,
                                                      unsigned k1, const int *__restrict__ row_ptr, const int *__restrict__ edge_var,
                                                      const int *__restrict__ edge_h, float *__restrict__ llr,
                                                      float *__restrict__ msg, int W, unsigned char *__restrict__ lvl,
                                                      signed char *__restrict__ sec)
{
    const SecretTab t = secret_stage(secret_lds, tab, law, K, QS);
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int r = (int)blockIdx.x * 4 + j;
    if (r >= R) return;
    const int x = BV + r;
    const long b = (long)blockIdx.y * 64 + lane;
    const bool live = b < batch;
    const int e_id = row_ptr[r + 1] - 1;
    int sum = 0;
    for (int e = row_ptr[r]; e < e_id; e++) sum += edge_h[e] * (int)sec[(size_t)edge_var[e] * Bp + b];
    const bool rev = edge_h[e_id] < 0;
    const int BSUM = (QS - 1) / 2;
    const int tr = live ? min(max(rev ? sum : -sum, -BSUM), BSUM) : 0;
    const unsigned long long trial = trials.trial(b, live);
    const unsigned wo = word_of(philox4x32_10(U4{(unsigned)(x >> 2), 0u, (unsigned)trial, (unsigned)(trial >> 32)}, k0, k1), x & 3);
    const int lv = t.outcome(wo, tr + BSUM, K, QS);
    const float *row = t.rows + lv * QS;
    const size_t r0 = (size_t)BV * Qb + (size_t)r * QS;
    for (int q = 0; q < QS; q++) llr[(r0 + q) * Bp + b] = live ? row[q] : 0.0f;
    lvl[(size_t)x * Bp + b] = (unsigned char)(live ? lv : K - 1);
    sec[(size_t)x * Bp + b] = (signed char)tr;
    for (int q = 0; q < QS; q++) msg[((size_t)e_id * W + q) * Bp + b] = live ? row[rev ? QS - 1 - q : q] : 0.0f;
}

__global__ __launch_bounds__(256) void k_q_mc_secret_sums(const unsigned *__restrict__ law, const float *__restrict__ tab, int K, int QS,
                                                          int Qb, int BV, int R, int batch, long Bp, long first, unsigned k0,
                                                          unsigned k1, const int *__restrict__ row_ptr, const int *__restrict__ edge_var,
                                                          const int *__restrict__ edge_h, float *__restrict__ llr,
                                                          float *__restrict__ msg, int W, unsigned char *__restrict__ lvl,
                                                          signed char *__restrict__ sec)
{
    extern __shared__ float secret_lds[];
    q_mc_secret_sums_body(secret_lds, law, tab, K, QS, Qb, BV, R, batch, Bp, scaldpc::TrialRange{first}, k0, k1, row_ptr, edge_var, edge_h,
                          llr, msg, W, lvl, sec);
}

// hard, sec: the decided and the secret values [N][Bp]; lvl: the drawn levels [N][Bp]; best: the value a variable decides from
// the row of level k alone, [32] for the coefficient table and [32] for the row-sum table.  The access shape of k_q_mc_result:
// grid Bp / 64, block 1024 = 64 codewords x 64 variables a step, four codewords per 32-bit load; the 64 partial counts of a
// codeword meet in LDS, two counters a round (four at once would take the whole 64 KB).  wrong / chan [batch][2]: coefficient
// variables, row-sum variables; either may be nullptr.
__global__ __launch_bounds__(1024) void k_q_mc_secret_result(const signed char *__restrict__ hard, const unsigned char *__restrict__ lvl,
                                                             const signed char *__restrict__ sec, const signed char *__restrict__ best,
                                                             int N, int BV, int batch, long Bp, unsigned char *__restrict__ success,
                                                             int *__restrict__ wrong, int *__restrict__ chan)
{
    __shared__ int part[2][64][64];  // [coefficient | row-sum][variable slot][codeword]
    __shared__ signed char bs[64];
    if (threadIdx.x < 64) bs[threadIdx.x] = best[threadIdx.x];
    __syncthreads();
    const int c4 = (threadIdx.x & 15) * 4, slot = threadIdx.x >> 4;
    const long b0 = (long)blockIdx.x * 64;
    int nw[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, nc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll 4
    for (int v = slot; v < N; v += 64) {
        const unsigned lw = *(const unsigned *)(lvl + (size_t)v * Bp + b0 + c4);  // (Bp and b0 are multiples of 64: aligned)
        const unsigned hw = *(const unsigned *)(hard + (size_t)v * Bp + b0 + c4);
        const unsigned sw = *(const unsigned *)(sec + (size_t)v * Bp + b0 + c4);
        const int tb = v >= BV;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned s = (sw >> (8 * k)) & 255u;
            const int wrong_here = ((hw >> (8 * k)) & 255u) != s;
            const int chan_here = (unsigned)(unsigned char)bs[32 * tb + (int)((lw >> (8 * k)) & 31u)] != s;
            nw[0][k] += tb ? 0 : wrong_here;
            nw[1][k] += tb ? wrong_here : 0;
            nc[0][k] += tb ? 0 : chan_here;
            nc[1][k] += tb ? chan_here : 0;
        }
    }
    // waves 0 and 1 add the 64 partial counts of a codeword: wave 0 the coefficient variables', wave 1 the row-sum variables'
    const int half = threadIdx.x >> 6, cw = threadIdx.x & 63;
    const long b = b0 + cw;
    const bool report = half < 2 && b < batch;
    for (int round = 0; round < 2; round++) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            part[0][slot][c4 + k] = round ? nc[0][k] : nw[0][k];
            part[1][slot][c4 + k] = round ? nc[1][k] : nw[1][k];
        }
        __syncthreads();
        if (report) {
            int n = 0;
            for (int i = 0; i < 64; i++) n += part[half][i][cw];
            int *out = round ? chan : wrong;
            if (out) out[2 * b + half] = n;
            if (!round && !half) success[b] = n == 0;
        }
        __syncthreads();
    }
}

}  // namespace
