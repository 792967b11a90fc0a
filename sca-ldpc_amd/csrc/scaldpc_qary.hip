// libscaldpc -- q-ary min-sum decoders on MI355X (gfx950).
//
// Replaces the in-tree Rust decoders of the reference's `simulate_rs` crate
// (simulate-with-python/simulate_rs/src/):
//   Decoder::new / min_sum / into_llr        decoder.rs:494-553, 560-666, 668-692
//   DecoderSpecial::new / min_sum            decoder_special.rs:387-464, 471-617
// reached from Python through pydecoder.rs:24-65 / 96-145.
//
// Arithmetic is the reference's, in its order, in f32: per check the minimum over all
// assignments d with sum d = 0 (over the integers) of S - alpha_j[d_j], S summed left to
// right from 0.0 exactly as `.sum()` does (decoder.rs:600-610); per variable channel +
// sum(c2v * h), minus self, normalised by the first minimum (decoder.rs:634-652); hard
// decision = first argmin of the total at the last iteration.  Minima are exact, so the
// order in which assignments are enumerated does not matter; everything else is
// add/subtract in the reference's order => hard decisions bit-exact with the oracle.
//
// Parallelisation: lane = codeword (batch innermost), thread = (node, codeword).
//   msg : float [edge][W][Bp]     one array, updated in place (v2c <-> c2v)
//   llr : float [var][Q][Bp]
// The enumeration indexes the alphabet with per-lane run-time digits, which rules out
// registers; per-thread alpha / beta vectors are staged in LDS laid out [slot][thread],
// so that whatever slot each lane picks, lane l always hits bank l (conflict free).
// This path is ALU/LDS bound (Q^(DC-1) assignments per check), not HBM bound; no
// roofline claim is made for it.
#include "scaldpc_common.h"
#include "scaldpc_logf.h"
#include "scaldpc_mc_law.h"
#include "scaldpc_qary_plan.h"
#include "scaldpc_trials.h"

#include <cmath>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

using namespace scaldpc;
typedef unsigned long long u64;
#include "scaldpc_qary_special.h"
#include "scaldpc_qary_rows.h"
#include "scaldpc_qary_soft.h"
#include "scaldpc_qary_mc.h"
#include "scaldpc_qary_secret.h"
#include "scaldpc_qary_mc_at.h"  // last: the list forms of the three generators

namespace {

constexpr int QERR_PMF = 3;        // decoder.rs:683-684 assert

// One pmf row as decoder.rs:668-692 reads it, symbol by symbol: the sum, left to right from 0.0, and the first strict maximum (a
// NaN is never chosen).  bad(): the reference's assert (decoder.rs:683-684: the row sums to 1 +- 1e-3) or no maximum (all NaN).
struct PmfScan {
    float sum = 0.0f, mx = 0.0f;
    bool have = false;
    __host__ __device__ __forceinline__ void step(float x)  // (host: the level tables of scaldpc_mc_qary_run, before anything is queued)
    {
        sum += x;
        if (x == x && (!have || x > mx)) {
            mx = x;
            have = true;
        }
    }
    __host__ __device__ __forceinline__ bool bad() const { return !have || !(sum < 1.0f + 0.001f) || !(sum > 1.0f - 0.001f); }
};
// key of a failing row, smaller = earlier: codeword, then alphabet (0 = coefficient rows, 1 = row-sum rows), then variable, then
// "no maximum" (scaldpc_qary_into_llr: codeword 0, alphabet 0, variable = row)
__device__ __forceinline__ u64 pmf_err_key(u64 b, int kind, u64 v, bool have)
{
    return (b << 32) | ((u64)kind << 31) | (v << 1) | (have ? 0ull : 1ull);
}

// decoder.rs:668-692 on the device: llr[q] = ln(max_p / p[q]) in f32, with glibc's logf restated
// for the device (scaldpc_logf.h) and the correctly rounded f32 division, so the LLRs are bit for bit
// what the reference's f32::ln gives on the host -- for host and device inputs alike.
// pmf: [batch][nv][Q] -> llr [nv][Q][Bp].  thread = (variable, codeword).
// A row that does not sum to 1 +- 1e-3 (or has no maximum: all NaN) is the reference's assert
// (decoder.rs:683-684): the smallest offending (codeword, variable) is left in *first_bad.
__global__ void k_q_into_llr(const float *__restrict__ pmf, int nv, int Q, int batch, long Bp,
                             float *__restrict__ llr, int *__restrict__ err, u64 *__restrict__ first_bad, int kind)
{
    const long b = (long)blockIdx.y * blockDim.x + threadIdx.x;
    const int v = blockIdx.x;
    if (b >= Bp) return;
    if (b >= batch) {  // padding lanes decode a harmless all-equal message
        for (int q = 0; q < Q; q++) llr[((size_t)v * Q + q) * Bp + b] = 0.0f;
        return;
    }
    const float *p = pmf + ((size_t)b * nv + v) * Q;
    PmfScan sc;
    for (int q = 0; q < Q; q++) sc.step(p[q]);
    if (sc.bad()) {
        atomicMax(err, QERR_PMF);
        atomicMax(first_bad, ~pmf_err_key((u64)b, kind, (u64)v, sc.have));  // (kept inverted: see scaldpc_qary::d_status)
    }
    // measured channel outputs repeat a handful of rows: no point caching across lanes, the double
    // pipe is idle anyway (18 double operations per symbol)
    for (int q = 0; q < Q; q++) llr[((size_t)v * Q + q) * Bp + b] = glibc_logf(sc.mx / p[q]);
}

// The same conversion through an LDS tile: the input is [codeword][variable][Q] (a codeword's pmf rows are contiguous), the
// output [variable][Q][codeword] -- with thread = (variable, codeword) and lane = codeword every lane read its own 12-byte
// row from a different cache line (28 us for config 4's 1024 x 450 x 3 floats).  Here a workgroup takes 64 codewords x VT
// variables, one wave per variable: the waves load each codeword's VT * Q contiguous floats with neighbouring lanes (one
// or two sectors per row), then wave w, lane = codeword, converts variable w from LDS (row stride 33: conflict free) and
// writes llr with 64 codewords per store.  Same arithmetic, same error key, as many waves as before.
// grid (ceil(nv / VT), Bp / 64), block 64 * VT, VT = max(1, 32 / Q) (at most 10).
// With col_ptr != nullptr the wave also writes the variable's first variable-to-check messages (decoder.rs:567-573:
// v2c = channel * h, i.e. the LLR row, mirrored where h < 0) to every edge of its variable -- k_q_init's job, without the
// launch and without reading the LLRs back (vbase = index of this alphabet's first variable in the graph, W = message row width).
// A SECOND alphabet can ride in the same launch (DecoderSpecial: the coefficient rows and the row-sum rows): blocks nb0 .. of
// grid.x convert pmf1 (nv1 rows of Q1 symbols, VT1 per block, kind 1, first variable vbase1) -- one launch less in a call
// that is made of ~10 us launches; the block is sized for the larger VT, the waves beyond a segment's VT only help load.
__global__ void k_q_into_llr_tiled(const float *__restrict__ pmf0, int nv0, int Q0, int VT0, int batch, long Bp,
                                   float *__restrict__ llr0, int *__restrict__ err, u64 *__restrict__ first_bad, int kind0,
                                   const int *__restrict__ col_ptr = nullptr, const int *__restrict__ csc_edge = nullptr,
                                   const int *__restrict__ edge_h = nullptr, float *__restrict__ msg = nullptr, int W = 0,
                                   int vbase0 = 0, int nb0 = 0x7fffffff, const float *__restrict__ pmf1 = nullptr, int nv1 = 0,
                                   int Q1 = 0, int VT1 = 0, float *__restrict__ llr1 = nullptr, int vbase1 = 0)
{
    __shared__ float tile[64 * 33];
    const bool seg1 = (int)blockIdx.x >= nb0;
    const float *__restrict__ pmf = seg1 ? pmf1 : pmf0;
    float *__restrict__ llr = seg1 ? llr1 : llr0;
    const int nv = seg1 ? nv1 : nv0, Q = seg1 ? Q1 : Q0, VT = seg1 ? VT1 : VT0, kind = seg1 ? 1 : kind0, vbase = seg1 ? vbase1 : vbase0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int v0 = ((int)blockIdx.x - (seg1 ? nb0 : 0)) * VT;
    const long b0 = (long)blockIdx.y * 64;
    const int nvv = min(VT, nv - v0), width = nvv * Q;  // floats per codeword in this tile (<= 32)
    // (all threads of the block over the tile's 64 x width floats: every load instruction has 64 active lanes)
    for (int idx = threadIdx.x; idx < 64 * width; idx += blockDim.x) {
        const int c = idx / width, l = idx - c * width;
        if (b0 + c < batch) tile[c * 33 + l] = pmf[((size_t)(b0 + c) * nv + v0) * Q + l];
    }
    __syncthreads();
    if (w >= nvv) return;
    const int v = v0 + w;
    const long b = b0 + lane;
    const int c0 = col_ptr ? col_ptr[vbase + v] : 0, c1 = col_ptr ? col_ptr[vbase + v + 1] : 0;
    if (b >= batch) {  // padding lanes decode a harmless all-equal message
        for (int q = 0; q < Q; q++) llr[((size_t)v * Q + q) * Bp + b] = 0.0f;
        for (int t = c0; t < c1; t++)
            for (int q = 0; q < Q; q++) msg[((size_t)csc_edge[t] * W + q) * Bp + b] = 0.0f;
        return;
    }
    const float *p = tile + lane * 33 + w * Q;
    PmfScan sc;
    for (int q = 0; q < Q; q++) sc.step(p[q]);
    if (sc.bad()) {
        atomicMax(err, QERR_PMF);
        atomicMax(first_bad, ~pmf_err_key((u64)b, kind, (u64)v, sc.have));  // (kept inverted: see scaldpc_qary::d_status)
    }
    float *own = tile + lane * 33 + w * Q;  // (this thread's slots of the tile: probabilities in, LLRs out)
    for (int q = 0; q < Q; q++) {
        const float l = glibc_logf(sc.mx / p[q]);
        llr[((size_t)v * Q + q) * Bp + b] = l;
        own[q] = l;
    }
    for (int t = c0; t < c1; t++) {
        const int e = csc_edge[t];
        const bool rev = edge_h[e] < 0;
        for (int q = 0; q < Q; q++) msg[((size_t)e * W + q) * Bp + b] = own[rev ? Q - 1 - q : q];
    }
}

// The same conversion on rows as they stand: pmf [rows][Q] -> llr [rows][Q] (scaldpc_qary_into_llr).
// bad[0] = smallest row index that fails the sum test (or has no maximum), as k_q_into_llr's key.
__global__ void k_q_into_llr_rows(const float *__restrict__ pmf, long rows, int Q, float *__restrict__ llr,
                                  u64 *__restrict__ first_bad)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float *p = pmf + (size_t)r * Q;
    PmfScan sc;
    for (int q = 0; q < Q; q++) sc.step(p[q]);
    if (sc.bad()) atomicMin(first_bad, pmf_err_key(0, 0, (u64)r, sc.have));
    for (int q = 0; q < Q; q++) llr[(size_t)r * Q + q] = glibc_logf(sc.mx / p[q]);
}

// decoder.rs:567-573: v2c = channel * h.  thread = (edge, codeword).
__global__ void k_q_init(const int *__restrict__ edge_var, const int *__restrict__ edge_h,
                         const int *__restrict__ var_q, const long *__restrict__ var_off,
                         const float *__restrict__ llr, float *__restrict__ msg, int W, long Bp)
{
    const long b = (long)blockIdx.y * blockDim.x + threadIdx.x;
    const int e = blockIdx.x;
    if (b >= Bp) return;
    const int v = edge_var[e], Q = var_q[v];
    const float *ch = llr + var_off[v] * Bp + b;
    const bool rev = edge_h[e] < 0;
    for (int q = 0; q < Q; q++) msg[((size_t)e * W + q) * Bp + b] = ch[(size_t)(rev ? Q - 1 - q : q) * Bp];
}

// Check-node update of Decoder (decoder.rs:585-631), finite-support enumeration
// (FiniteDValueIterator, decoder.rs:281-401), index 0 fastest.
// block = T threads = T codewords of one check; LDS: A[k*Q][T], Bt[k*Q][T] floats, fin[k*Q][T] bytes.
// WORD: the per-lane registers that hold one 8-bit digit per edge of the check (finite-symbol counts, the
// enumeration index, the chosen symbols): u64 for checks of up to 8 edges (every size the reference registers,
// lib.rs:32-75), unsigned __int128 for 9..16 -- Decoder is const-generic in DC (decoder.rs:417-438).
template <typename WORD>
__global__ void k_q_check(const int *__restrict__ row_ptr, float *msg, int Q, int B, long Bp, int batch, int maxdc,
                          int *__restrict__ err)
{
    extern __shared__ unsigned char smem[];
    const int T = blockDim.x, tid = threadIdx.x;
    float *A = (float *)smem;
    float *Bt = A + (size_t)maxdc * Q * T;
    unsigned char *fin = (unsigned char *)(Bt + (size_t)maxdc * Q * T);
    const int c = blockIdx.x;
    const long b = (long)blockIdx.y * T + tid;
    if (b >= batch) return;  // padding lanes: no barrier below, every thread owns its LDS column
    const int e0 = row_ptr[c], k = row_ptr[c + 1] - e0;
    if (k == 0) {
        if (tid == 0) atomicMax(err, QERR_NO_CONFIG);
        return;
    }
    WORD nums = 0;
    bool bad = false;
    for (int j = 0; j < k; j++) {
        int cnt = 0;
        for (int q = 0; q < Q; q++) {
            const float x = msg[((size_t)(e0 + j) * Q + q) * Bp + b];
            A[(size_t)(j * Q + q) * T + tid] = x;
            Bt[(size_t)(j * Q + q) * T + tid] = INFINITY;
            if (finite_f(x)) fin[(size_t)(j * Q + cnt++) * T + tid] = (unsigned char)q;
        }
        nums |= (WORD)cnt << (8 * j);
        bad |= cnt == 0;
    }
    if (bad) {
        atomicMax(err, QERR_NO_FINITE);
    } else {
        WORD idx = 0;
        int nconf = 0;
        for (;;) {
            int dsum = 0;
            float S = 0.0f;
            WORD qs = 0;
            for (int j = 0; j < k - 1; j++) {
                const int ij = (int)(idx >> (8 * j)) & 255;
                const int q = fin[(size_t)(j * Q + ij) * T + tid];
                qs |= (WORD)q << (8 * j);
                dsum += q - B;
                S += A[(size_t)(j * Q + q) * T + tid];
            }
            const int dl = -dsum;
            if (dl >= -B && dl <= B) {
                const int ql = dl + B;
                qs |= (WORD)ql << (8 * (k - 1));
                S += A[(size_t)((k - 1) * Q + ql) * T + tid];
                if (finite_f(S)) {
                    nconf++;
                    for (int j = 0; j < k; j++) {
                        const int q = (int)(qs >> (8 * j)) & 255;
                        const size_t o = (size_t)(j * Q + q) * T + tid;
                        Bt[o] = fminf(S - A[o], Bt[o]);
                    }
                }
            }
            int j = 0;
            for (; j < k - 1; j++) {
                const int ij = (int)(idx >> (8 * j)) & 255, nj = (int)(nums >> (8 * j)) & 255;
                if (ij + 1 < nj) {
                    idx += (WORD)1 << (8 * j);
                    break;
                }
                idx &= ~((WORD)255 << (8 * j));
            }
            if (j >= k - 1) break;
        }
        if (nconf == 0) atomicMax(err, QERR_NO_CONFIG);
    }
    for (int j = 0; j < k; j++)
        for (int q = 0; q < Q; q++)
            msg[((size_t)(e0 + j) * Q + q) * Bp + b] = Bt[(size_t)(j * Q + q) * T + tid];
}


// ---------------------------------------------------------------------------
// Small and medium batches (<= 256; single `min_sum` calls are the reference's usual pattern): lane = codeword
// would leave 63 lanes idle while one walks Q^(DC-1) assignments.  Here a WAVE owns one
// (check, codeword): the lanes split the assignment space (assignment c goes to lane
// c mod 64, stepped through mixed-radix digits), each keeps private running minima in LDS
// ([slot][lane], conflict free), and the 64 partial minima of every slot are combined with
// wave shuffles.  min is exact and every S is summed in the same order as before, so the
// messages are bit-identical to the lane = codeword kernels'.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return v;
}

// The wave kernels' walk through the assignment space: assignment c goes to lane c mod 64.  Digits are 8 bits each, index 0
// fastest, digit j below radix(j).  start: the digits of the lane's first assignment and of the stride 64.
template <typename Radix>
__device__ __forceinline__ void mixed_radix_start(int lane, int nd, Radix radix, u64 &idx, u64 &stp)
{
    idx = 0;
    stp = 0;
    unsigned a = (unsigned)lane, st = 64;  // (both start below 65: 32-bit division, not the 64-bit library routine)
    for (int j = 0; j < nd; j++) {
        const unsigned nj = (unsigned)radix(j);
        idx |= (u64)(a % nj) << (8 * j);
        a /= nj;
        stp |= (u64)(st % nj) << (8 * j);
        st /= nj;
    }
}
// idx + stride (one conditional subtraction per digit)
template <typename Radix>
__device__ __forceinline__ u64 mixed_radix_step(u64 idx, u64 stp, int nd, Radix radix)
{
    int carry = 0;
    u64 nidx = 0;
    for (int j = 0; j < nd; j++) {
        int d = ((int)(idx >> (8 * j)) & 255) + ((int)(stp >> (8 * j)) & 255) + carry;
        carry = d >= radix(j);
        if (carry) d -= radix(j);
        nidx |= (u64)d << (8 * j);
    }
    return nidx;
}

// generic Decoder check (decoder.rs:585-631).  grid (R, batch), block 64.
// LDS: A[k*Q] floats (shared), fin[k*Q] + num[k] bytes (shared), Bt[k*Q][64] floats (per lane).
__global__ __launch_bounds__(64) void k_q_check_wave(const int *__restrict__ row_ptr, float *msg, int Q, int B, long Bp,
                                                     int maxdc, int *__restrict__ err)
{
    extern __shared__ unsigned char smem[];
    const int lane = threadIdx.x;
    float *A = (float *)smem;
    float *Bt = A + maxdc * Q;
    unsigned char *fin = (unsigned char *)(Bt + (size_t)maxdc * Q * 64);
    unsigned char *num = fin + maxdc * Q;
    const int c = blockIdx.x;
    const long b = blockIdx.y;
    const int e0 = row_ptr[c], k = row_ptr[c + 1] - e0;
    if (k == 0) {
        if (lane == 0) atomicMax(err, QERR_NO_CONFIG);
        return;
    }
    for (int i = lane; i < k * Q; i += 64) A[i] = msg[((size_t)(e0 + i / Q) * Q + i % Q) * Bp + b];
    for (int i = 0; i < k * Q; i++) Bt[(size_t)i * 64 + lane] = INFINITY;
    __syncthreads();
    if (lane < k) {
        int cnt = 0;
        for (int q = 0; q < Q; q++)
            if (finite_f(A[lane * Q + q])) fin[lane * Q + cnt++] = (unsigned char)q;
        num[lane] = (unsigned char)cnt;
    }
    __syncthreads();
    bool bad = false;
    unsigned long long total = 1;
    for (int j = 0; j < k; j++) bad |= num[j] == 0;
    for (int j = 0; j < k - 1; j++) total *= num[j];
    if (bad) {
        if (lane == 0) atomicMax(err, QERR_NO_FINITE);
    } else {
        // digits of this lane's first assignment and of the stride 64, index 0 fastest
        const auto radix = [&](int j) { return (int)num[j]; };
        u64 idx, stp;
        mixed_radix_start(lane, k - 1, radix, idx, stp);
        int nconf = 0;
        for (unsigned long long cfg = lane; cfg < total; cfg += 64) {
            int dsum = 0;
            float S = 0.0f;
            u64 qs = 0;
            for (int j = 0; j < k - 1; j++) {
                const int q = fin[j * Q + ((int)(idx >> (8 * j)) & 255)];
                qs |= (u64)q << (8 * j);
                dsum += q - B;
                S += A[j * Q + q];
            }
            const int dl = -dsum;
            if (dl >= -B && dl <= B) {
                const int ql = dl + B;
                qs |= (u64)ql << (8 * (k - 1));
                S += A[(k - 1) * Q + ql];
                if (finite_f(S)) {
                    nconf++;
                    for (int j = 0; j < k; j++) {
                        const int q = (int)(qs >> (8 * j)) & 255;
                        float *bb = &Bt[(size_t)(j * Q + q) * 64 + lane];
                        *bb = fminf(S - A[j * Q + q], *bb);
                    }
                }
            }
            idx = mixed_radix_step(idx, stp, k - 1, radix);
        }
        const u64 any = __ballot(nconf > 0);
        if (!any && lane == 0) atomicMax(err, QERR_NO_CONFIG);
    }
    // minimum over the 64 lanes' partial results, TRANSPOSED (fold_min_rows64): lane L folds whole rows i = L, L + 64, ... of Bt
    // instead of 6 dependent ds_bpermute steps per entry (k * Q entries: 630 of them for a degree-7 check over Q = 15)
    __syncthreads();
    for (int i = lane; i < k * Q; i += 64) {
        msg[((size_t)(e0 + i / Q) * Q + i % Q) * Bp + b] = fold_min_rows64(Bt + (size_t)i * 64, lane);
    }
}

// DecoderSpecial check (decoder_special.rs:506-563), wave per (check, codeword).
// LDS: Ab[nb*QB], As[QS] floats (shared), Bb[nb*QB][64], Bs[QS][64] floats (per lane).
__global__ __launch_bounds__(64) void k_q_special_check_wave(const int *__restrict__ row_ptr, float *msg, int B, int BSUM,
                                                             int W, long Bp, int nbm, int skip_nb)
{
    extern __shared__ unsigned char smem[];
    const int lane = threadIdx.x;
    const int QB = 2 * B + 1, QS = 2 * BSUM + 1;
    float *Ab = (float *)smem;
    float *As = Ab + nbm * QB;
    float *Bb = As + QS;
    float *Bs = Bb + (size_t)nbm * QB * 64;
    const int c = blockIdx.x;
    const long b = blockIdx.y;
    const int e0 = row_ptr[c], k = row_ptr[c + 1] - e0, nb = k - 1;
    if (nb == skip_nb) return;  // rows of this degree belong to k_q_special_check_tree
    for (int i = lane; i < nb * QB; i += 64) Ab[i] = msg[((size_t)(e0 + i / QB) * W + i % QB) * Bp + b];
    for (int i = lane; i < QS; i += 64) As[i] = msg[((size_t)(e0 + nb) * W + i) * Bp + b];
    for (int i = 0; i < nb * QB; i++) Bb[(size_t)i * 64 + lane] = INFINITY;
    for (int i = 0; i < QS; i++) Bs[(size_t)i * 64 + lane] = INFINITY;
    __syncthreads();
    unsigned long long total = 1;
    for (int j = 0; j < nb; j++) total *= QB;
    const auto radix = [=](int) { return QB; };
    u64 dq, stp;
    mixed_radix_start(lane, nb, radix, dq, stp);
    for (unsigned long long cfg = lane; cfg < total; cfg += 64) {
        int dsum = 0;
        float S = 0.0f;
        for (int j = 0; j < nb; j++) {
            const int q = (int)(dq >> (8 * j)) & 255;
            dsum += q - B;
            S += Ab[j * QB + q];
        }
        const int os = -dsum + BSUM;
        S += As[os];
        for (int j = 0; j < nb; j++) {
            const int q = (int)(dq >> (8 * j)) & 255;
            float *bb = &Bb[(size_t)(j * QB + q) * 64 + lane];
            *bb = fminf(*bb, S - Ab[j * QB + q]);
        }
        Bs[(size_t)os * 64 + lane] = fminf(Bs[(size_t)os * 64 + lane], S - As[os]);
        dq = mixed_radix_step(dq, stp, nb, radix);
    }
    // minima over the 64 lanes, transposed (see k_q_check_wave): the row's nb * QB coefficient entries, then its QS sum entries
    __syncthreads();
    for (int i = lane; i < nb * QB + QS; i += 64) {
        const float *row = i < nb * QB ? Bb + (size_t)i * 64 : Bs + (size_t)(i - nb * QB) * 64;
        const float v = fold_min_rows64(row, lane);
        if (i < nb * QB)
            msg[((size_t)(e0 + i / QB) * W + i % QB) * Bp + b] = v;
        else
            msg[((size_t)(e0 + nb) * W + (i - nb * QB)) * Bp + b] = v;
    }
}

// Variable-node update (decoder.rs:634-658 / decoder_special.rs:566-609).
// thread = (variable, codeword); LDS: sum[Qmax][T], tmp[Qmax][T].
// SOFT (the last pass of a soft call, scaldpc_qary_soft.h): the totals go to cost[var_off[v] + q][Bp] (laid out like llr;
// nullptr: not wanted) and the margin of the decision to margin[v][Bp] (likewise), out of the same scan that decides.
template <bool SOFT>
__device__ __forceinline__ void var_body(unsigned char *smem, int v0, const int *__restrict__ col_ptr, const int *__restrict__ csc_edge,
                                         const int *__restrict__ edge_h, const int *__restrict__ var_q,
                                         const long *__restrict__ var_off, const float *__restrict__ llr, float *msg, int W, long Bp,
                                         int batch, int Qmax, int last, signed char *__restrict__ out, float *__restrict__ cost,
                                         float *__restrict__ margin)
{
    const int T = blockDim.x, tid = threadIdx.x;
    float *sum = (float *)smem;
    float *tmp = sum + (size_t)Qmax * T;
    const int v = v0 + blockIdx.x;
    const long b = (long)blockIdx.y * T + tid;
    if (b >= batch) return;
    const int Q = var_q[v], Bv = (Q - 1) / 2;
    const float *ch = llr + var_off[v] * Bp + b;
    for (int q = 0; q < Q; q++) sum[(size_t)q * T + tid] = ch[(size_t)q * Bp];
    const int c0 = col_ptr[v], c1 = col_ptr[v + 1];
    for (int t = c0; t < c1; t++) {
        const int e = csc_edge[t];
        const bool rev = edge_h[e] < 0;
        const float *in = msg + (size_t)e * W * Bp + b;
        for (int q = 0; q < Q; q++) sum[(size_t)q * T + tid] = sum[(size_t)q * T + tid] + in[(size_t)(rev ? Q - 1 - q : q) * Bp];
    }
    for (int t = c0; t < c1; t++) {
        const int e = csc_edge[t];
        const bool rev = edge_h[e] < 0;
        float *io = msg + (size_t)e * W * Bp + b;
        // prim_out = (sum - c2v*h) * h   (qary_sub_with_mult_in_gf then mult_in_gf)
        for (int q = 0; q < Q; q++) {
            const int qi = rev ? Q - 1 - q : q;
            tmp[(size_t)qi * T + tid] = sum[(size_t)q * T + tid] - io[(size_t)qi * Bp];
        }
        float mv = INFINITY;
        int ma = 0;
        for (int q = 0; q < Q; q++) {
            const float x = tmp[(size_t)q * T + tid];
            if (x < mv) {
                mv = x;
                ma = q;
            }
        }
        const float mn = tmp[(size_t)ma * T + tid];
        for (int q = 0; q < Q; q++) io[(size_t)q * Bp] = tmp[(size_t)q * T + tid] - mn;
    }
    if (SOFT) {
        SoftScan sc;
        for (int q = 0; q < Q; q++) {
            const float x = sum[(size_t)q * T + tid];
            if (cost) cost[(size_t)(var_off[v] + q) * Bp + b] = x;
            sc.step(x, q);
        }
        out[(size_t)v * Bp + b] = (signed char)(sc.ma - Bv);
        if (margin) margin[(size_t)v * Bp + b] = sc.m2 - sum[(size_t)sc.ma * T + tid];
    } else if (last) {
        float mv = INFINITY;
        int ma = 0;
        for (int q = 0; q < Q; q++) {
            const float x = sum[(size_t)q * T + tid];
            if (x < mv) {
                mv = x;
                ma = q;
            }
        }
        out[(size_t)v * Bp + b] = (signed char)(ma - Bv);
    }
}

// SOFT = false: cost and margin are not read.  SOFT = true: `last` is not (a soft pass is the last one).
template <bool SOFT>
__global__ void k_q_var(int v0, const int *__restrict__ col_ptr, const int *__restrict__ csc_edge,
                        const int *__restrict__ edge_h, const int *__restrict__ var_q,
                        const long *__restrict__ var_off, const float *__restrict__ llr, float *msg, int W, long Bp,
                        int batch, int Qmax, int last, signed char *__restrict__ out, float *__restrict__ cost,
                        float *__restrict__ margin)
{
    extern __shared__ unsigned char smem[];
    var_body<SOFT>(smem, v0, col_ptr, csc_edge, edge_h, var_q, var_off, llr, msg, W, Bp, batch, Qmax, last, out, cost, margin);
}

// The same update with everything in registers, for the plain decoder with alphabets Q = 3, 5, 7, 15 and columns of at
// most DMAX checks: every incoming message is loaded ONCE (the generic kernel reads each twice, with an LDS round trip
// between global accesses), all of a column's loads are issued before the first add.  Same additions and subtractions in
// the same order, the same first-minimum rule: identical symbols.  llr is [var][Q][Bp] here (one alphabet).
// grid (N, Bp/64), block 64.
//   v: variable (graph index: column of col_ptr, row of `out`);  llr: this variable's Q rows;  W: width of a message row
//   SOFT (the last pass of a soft call): cost / margin point at THIS variable's rows of the staging arrays (nullptr: not wanted)
template <int Q, int DMAX, bool SOFT = false>
__device__ __forceinline__ void var_small_body(int v, const float *__restrict__ llr, const int *__restrict__ col_ptr,
                                               const int *__restrict__ csc_edge, const int *__restrict__ edge_h, float *msg, int W,
                                               long Bp, long b, int last, signed char *__restrict__ out,
                                               float *__restrict__ cost = nullptr, float *__restrict__ margin = nullptr)
{
    const int c0 = col_ptr[v], deg = col_ptr[v + 1] - c0;
    float sum[Q], in[DMAX][Q];
    int ed[DMAX];
    bool rv[DMAX];
#pragma unroll
    for (int q = 0; q < Q; q++) sum[q] = llr[(size_t)q * Bp + b];
#pragma unroll
    for (int t = 0; t < DMAX; t++) {
        ed[t] = 0;
        rv[t] = false;
        if (t < deg) {
            ed[t] = csc_edge[c0 + t];
            rv[t] = edge_h[ed[t]] < 0;
#pragma unroll
            for (int q = 0; q < Q; q++) in[t][q] = msg[((size_t)ed[t] * W + q) * Bp + b];
        }
    }
#pragma unroll
    for (int t = 0; t < DMAX; t++)
        if (t < deg) {
#pragma unroll
            for (int q = 0; q < Q; q++) sum[q] = sum[q] + (rv[t] ? in[t][Q - 1 - q] : in[t][q]);
        }
#pragma unroll
    for (int t = 0; t < DMAX; t++)
        if (t < deg) {
            float tmp[Q];  // tmp[qi] = sum[q] - c2v[qi], qi = q mirrored where h < 0
#pragma unroll
            for (int q = 0; q < Q; q++) tmp[q] = (rv[t] ? sum[Q - 1 - q] : sum[q]) - in[t][q];
            float mv = INFINITY, mn = tmp[0];  // first strict minimum; default index 0 (NaN never selected)
#pragma unroll
            for (int q = 0; q < Q; q++)
                if (tmp[q] < mv) {
                    mv = tmp[q];
                    mn = tmp[q];
                }
#pragma unroll
            for (int q = 0; q < Q; q++) msg[((size_t)ed[t] * W + q) * Bp + b] = tmp[q] - mn;
        }
    if (SOFT) {
        SoftScan sc;
        float m1 = sum[0];  // the total at the decided symbol (index 0 when nothing is selected)
#pragma unroll
        for (int q = 0; q < Q; q++) {
            if (sum[q] < sc.mv) m1 = sum[q];
            sc.step(sum[q], q);
        }
        if (cost) {
#pragma unroll
            for (int q = 0; q < Q; q++) cost[(size_t)q * Bp + b] = sum[q];
        }
        out[(size_t)v * Bp + b] = (signed char)(sc.ma - (Q - 1) / 2);
        if (margin) margin[b] = sc.m2 - m1;
    } else if (last) {
        float mv = INFINITY;
        int ma = 0;
#pragma unroll
        for (int q = 0; q < Q; q++)
            if (sum[q] < mv) {
                mv = sum[q];
                ma = q;
            }
        out[(size_t)v * Bp + b] = (signed char)(ma - (Q - 1) / 2);
    }
}

// (cost / margin: the staging arrays' bases, read only where SOFT)
template <int Q, int DMAX, bool SOFT>
__global__ __launch_bounds__(64) void k_q_var_small(const int *__restrict__ col_ptr, const int *__restrict__ csc_edge,
                                                    const int *__restrict__ edge_h, const float *__restrict__ llr, float *msg,
                                                    long Bp, int batch, int last, signed char *__restrict__ out,
                                                    float *__restrict__ cost, float *__restrict__ margin)
{
    const int v = blockIdx.x;
    const long b = (long)blockIdx.y * 64 + threadIdx.x;
    if (b >= batch) return;
    var_small_body<Q, DMAX, SOFT>(v, llr + (size_t)v * Q * Bp, col_ptr, csc_edge, edge_h, msg, Q, Bp, b, last, out,
                                  SOFT && cost ? cost + (size_t)v * Q * Bp : nullptr, SOFT && margin ? margin + (size_t)v * Bp : nullptr);
}

// DecoderSpecial (decoder_special.rs:566-609): the first BV variables over QA symbols (columns of at most DA checks), the
// row-sum variables behind them over QS symbols, one check each; message rows are W = max(QA, QS) wide.
// grid (N, Bp/64), block 64.
template <int QA, int DA, int QS, bool SOFT>
__global__ __launch_bounds__(64) void k_q_var_small_special(const int *__restrict__ col_ptr, const int *__restrict__ csc_edge,
                                                            const int *__restrict__ edge_h, const float *__restrict__ llr,
                                                            float *msg, int BV, int W, long Bp, int batch, int last,
                                                            signed char *__restrict__ out, float *__restrict__ cost,
                                                            float *__restrict__ margin)
{
    const int v = blockIdx.x;
    const long b = (long)blockIdx.y * 64 + threadIdx.x;
    if (b >= batch) return;
    if constexpr (SOFT) {
        float *mg = margin ? margin + (size_t)v * Bp : nullptr;
        if (v < BV) {
            const size_t row = (size_t)v * QA;
            var_small_body<QA, DA, true>(v, llr + row * Bp, col_ptr, csc_edge, edge_h, msg, W, Bp, b, 1, out, cost ? cost + row * Bp : nullptr, mg);
        } else {
            const size_t row = (size_t)BV * QA + (size_t)(v - BV) * QS;
            var_small_body<QS, 1, true>(v, llr + row * Bp, col_ptr, csc_edge, edge_h, msg, W, Bp, b, 1, out, cost ? cost + row * Bp : nullptr, mg);
        }
    } else if (v < BV)  // (one address expression for both forms compiles to other code: kept apart)
        var_small_body<QA, DA>(v, llr + (size_t)v * QA * Bp, col_ptr, csc_edge, edge_h, msg, W, Bp, b, last, out);
    else
        var_small_body<QS, 1>(v, llr + ((size_t)BV * QA + (size_t)(v - BV) * QS) * Bp, col_ptr, csc_edge, edge_h, msg, W, Bp, b, last, out);
}

// [N][Bp] -> [batch][N]
__global__ void k_q_unpack(const signed char *__restrict__ in, int N, int batch, long Bp, signed char *__restrict__ out)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (v < N && b < batch) out[(size_t)b * N + v] = in[(size_t)v * Bp + b];
}

}  // namespace

// The handle's stream and timing events, released when the handle goes.  scaldpc_qary derives from it, so every buffer
// member has returned its device memory before they are released.
struct QaryStreams {
    int device = 0;  // the device the handle was created on; every entry point runs there
    hipStream_t own_stream = nullptr;
    std::vector<hipEvent_t> tev;
    QaryStreams() = default;
    QaryStreams(const QaryStreams &) = delete;
    QaryStreams &operator=(const QaryStreams &) = delete;
    ~QaryStreams()
    {
        for (auto &e : tev) (void)hipEventDestroy(e);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
};

// Every block the handle owns is a Buf member; d_err and d_first_bad are views into d_status.  The graph's shape (QaryShape:
// special, R, N, E, Q, QS, W, the degrees) is what qary_plan reads.
struct scaldpc_qary : QaryStreams, QaryShape {
    int B = 0, BSUM = 0, iterations = 0;
    long llr_rows = 0;  // total alphabet rows over all variables
    Buf<int> d_row_ptr, d_col_ptr, d_csc_edge, d_edge_var, d_edge_h, d_var_q;
    Buf<long> d_var_off;
    std::vector<int> h_var_q;
    std::vector<long> h_var_off;
    long cap_bp = 0;  // codeword columns d_msg, d_llr and d_hard are sized for
    Buf<float> d_msg, d_llr, d_pmf, d_pmf2;
    Buf<signed char> d_hard, d_out;
    // soft calls only (allocated by the first soft call that asks for the output they stage; a handle that only sees plain
    // calls owns none of them): the last pass's totals [llr_rows][Bp] and margins [N][Bp] as the variable kernels write them,
    // their [batch][...] forms for host callers, and the unmet-check counts
    Buf<float> d_cost, d_margin, d_cost_out, d_margin_out;
    Buf<int> d_unmet;
    // Monte-Carlo calls only (scaldpc_mc_qary_run; allocated by the first one): the drawn levels [N][Bp], the level tables (their pmf
    // rows, then their LLR rows), and for host callers the per-trial results (errs, wrong, success) and the levels as [batch][N]
    Buf<unsigned char> d_mc_lvl, d_mc_lvl_out;
    Buf<float> d_mc_tab;
    Buf<int> d_mc_res;
    std::vector<float> mc_tab;  // host side of d_mc_tab's pmf rows and of d_mc_res: alive until the call has drained its stream
    std::vector<int> mc_res;
    bool mc_tab_ok = false;  // d_mc_tab holds the LLR rows of mc_tab (a finished call put them there): a sweep converts its tables once
    // scaldpc_mc_qary_run_secret only (allocated by the first such call): the secret values [N][Bp] and, for host callers, as
    // [batch][N]; the law's device form (pack_secret_law) with its host side, kept like the tables
    Buf<signed char> d_mc_sec, d_mc_sec_out;
    Buf<unsigned> d_mc_law;
    Buf<long long> d_trial_ids;  // the _at entries: the device copy of the call's trial list, [batch]
    std::vector<unsigned> mc_law;
    bool mc_law_ok = false;
    // one 16-byte status block per handle, zeroed by ONE fill and read back by ONE copy per call: [0] = the bitwise complement of
    // the smallest (codeword, variable) key whose pmf row fails the sum test (0: none; kept inverted so that "none" is zero
    // and the kernels lower the key with atomicMax), [1] = the call's error code (low word).  A third word behind the block is
    // k_q_into_llr_rows's key in a Monte-Carlo call (never read: the level tables are tested on the host)
    Buf<u64> d_status;
    int *d_err = nullptr;        // = (int *)(d_status + 1)
    u64 *d_first_bad = nullptr;  // = d_status
    QaryKnobs kn;  // (set by scaldpc_qary_configure; the environment is read once, at creation)
    float stat_ms_check = 0.f, stat_ms_var = 0.f, stat_ms_call = 0.f;
    int stat_iters = 0, stat_kernel = -1, stat_batch = 0;
    std::mutex mu;
};

namespace {

int qary_build(int R, int N, int B, int BSUM, bool special, const int8_t *H, int iterations, scaldpc_qary **out)
{
    if (!out) return fail(SCALDPC_EINVAL, "out is NULL");
    *out = nullptr;
    if (R <= 0 || N <= 0 || B < 1 || !H || iterations < 0)
        return fail(SCALDPC_EINVAL, "bad q-ary decoder arguments (R=%d N=%d B=%d)", R, N, B);
    if (B > 127) return fail(SCALDPC_EDEGREE, "B=%d: hard decisions are int8 (decoder.rs i8)", B);
    if (special) {
        if (BSUM < 1 || BSUM % B != 0)
            return fail(SCALDPC_EINVAL, "BSUM (%d) must be multiple of B (%d)", BSUM, B);  // decoder_special.rs:388-392
        if (N <= R) return fail(SCALDPC_EINVAL, "special decoder needs N > R");
        if (BSUM > 127) return fail(SCALDPC_EDEGREE, "BSUM=%d: hard decisions are int8", BSUM);
    }
    const int BV = special ? N - R : N;
    std::vector<int> row_ptr(R + 1, 0), col_cnt(N, 0), edge_var, edge_h;
    for (int r = 0; r < R; r++) {
        for (int c = 0; c < N; c++) {
            const int h = H[(size_t)r * N + c];
            if (!h) continue;
            if (h != 1 && h != -1) return fail(SCALDPC_EINVAL, "H[%d][%d] = %d: entries must be in {-1,0,1}", r, c, h);
            edge_var.push_back(c);
            edge_h.push_back(h);
            col_cnt[c]++;
        }
        row_ptr[r + 1] = (int)edge_var.size();
    }
    const int E = (int)edge_var.size();
    int maxdc = 0;
    for (int r = 0; r < R; r++) maxdc = std::max(maxdc, row_ptr[r + 1] - row_ptr[r]);
    // one 8-bit digit per edge of a check in a register word: 64 bits for degree <= 8 (all kernels), 128 bits for 9..16
    // (the lane-per-codeword kernel only: Decoder is const-generic in DC, decoder.rs:417-438; the reference registers 4 and 7)
    // DecoderSpecial beyond 8: the any-length min-plus recursion (k_q_special_check_dp_any), where the plan takes the shape
    if (special && maxdc > 8) {
        QaryShape g;
        g.special = true;
        g.R = R; g.N = N; g.E = E; g.Q = 2 * B + 1; g.QS = 2 * BSUM + 1; g.W = g.QS; g.maxdc = g.mindc = maxdc;
        QaryPlan p;
        if (qary_plan(g, QaryKnobs(), 1, &p))
            return fail(SCALDPC_EDEGREE, "check degree %d > 8 is not supported by the enumeration kernels, and the min-plus recursion "
                        "for rows of any length takes B = 1, 2, 3 with 2*B*(degree-1)+1 <= 85 table entries (here B = %d, %d entries)",
                        maxdc, B, 2 * B * (maxdc - 1) + 1);
    } else if (maxdc > (special ? 8 : 16))
        return fail(SCALDPC_EDEGREE, "check degree %d > %d is not supported by the enumeration kernels", maxdc, special ? 8 : 16);
    if (special) {
        for (int r = 0; r < R; r++) {
            const int k = row_ptr[r + 1] - row_ptr[r];
            if (k < 1) return fail(SCALDPC_EINVAL, "special decoder: check %d is empty", r);
            for (int j = 0; j < k - 1; j++)
                if (edge_var[row_ptr[r] + j] >= BV)
                    return fail(SCALDPC_EINVAL, "special decoder: H is not of the form [H' | I] (row %d)", r);
            if (edge_var[row_ptr[r] + k - 1] < BV)
                return fail(SCALDPC_EINVAL, "special decoder: row %d has no row-sum variable (H != [H' | I])", r);
            if ((k - 1) * B > BSUM)
                return fail(SCALDPC_EINVAL, "special decoder: (degree-1)*B = %d exceeds BSUM = %d in row %d", (k - 1) * B,
                            BSUM, r);
        }
        for (int v = BV; v < N; v++)
            if (col_cnt[v] != 1) return fail(SCALDPC_EINVAL, "special decoder: row-sum variable %d has degree %d", v, col_cnt[v]);
    }
    std::vector<int> col_ptr(N + 1, 0), csc_edge(E), fill(N, 0);
    for (int v = 0; v < N; v++) col_ptr[v + 1] = col_ptr[v] + col_cnt[v];
    for (int e = 0; e < E; e++) csc_edge[col_ptr[edge_var[e]] + fill[edge_var[e]]++] = e;

    scaldpc_qary *h = new (std::nothrow) scaldpc_qary();
    if (!h) return fail(SCALDPC_ENOMEM, "out of host memory");
    h->special = special;
    h->R = R; h->N = N; h->B = B; h->BSUM = BSUM;
    h->Q = 2 * B + 1;
    h->QS = special ? 2 * BSUM + 1 : h->Q;
    h->W = std::max(h->Q, h->QS);
    h->iterations = iterations;
    h->E = E;
    h->maxdc = maxdc;
    h->mindc = maxdc;
    for (int v = 0; v < N; v++) h->maxdv = std::max(h->maxdv, col_cnt[v]);
    for (int r = 0; r < R; r++) h->mindc = std::min(h->mindc, row_ptr[r + 1] - row_ptr[r]);
    h->h_var_q.resize(N);
    h->h_var_off.resize(N);
    long off = 0;
    for (int v = 0; v < N; v++) {
        h->h_var_q[v] = v < BV ? h->Q : h->QS;
        h->h_var_off[v] = off;
        off += h->h_var_q[v];
    }
    h->llr_rows = off;
    if (const char *e = getenv("SCALDPC_QARY_WAVE")) h->kn.wave = atoi(e) != 0;  // the environment is read once per handle
    if (getenv("SCALDPC_QARY_NO_UNROLL")) h->kn.unroll = 0;
    if (getenv("SCALDPC_QARY_NO_TREE")) h->kn.tree = 0;
    auto device_side = [&]() -> int {
        auto up = [](auto &d, const auto *src, size_t cnt) -> int {
            SC_TRY(d.ensure(cnt));
            if (cnt) SC_HIP(hipMemcpy(d, src, cnt * sizeof(*src), hipMemcpyHostToDevice));
            return 0;
        };
        SC_TRY(up(h->d_row_ptr, row_ptr.data(), R + 1));
        SC_TRY(up(h->d_col_ptr, col_ptr.data(), N + 1));
        SC_TRY(up(h->d_csc_edge, csc_edge.data(), E));
        SC_TRY(up(h->d_edge_var, edge_var.data(), E));
        SC_TRY(up(h->d_edge_h, edge_h.data(), E));
        SC_TRY(up(h->d_var_q, h->h_var_q.data(), N));
        SC_TRY(up(h->d_var_off, h->h_var_off.data(), N));
        SC_TRY(h->d_status.ensure(3));
        h->d_first_bad = h->d_status;
        h->d_err = (int *)(h->d_status + 1);
        if (hipGetDevice(&h->device) != hipSuccess) return fail(SCALDPC_EHIP, "hipGetDevice failed");
        if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess)
            return fail(SCALDPC_EHIP, "hipStreamCreate failed");
        return 0;
    };
    if (const int rc = device_side()) {
        scaldpc_qary_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

// The optional outputs of a soft call (each may be NULL; all NULL: the plain call).  cost_s: DecoderSpecial's row-sum rows.
struct SoftOut {
    float *cost_b = nullptr, *cost_s = nullptr, *margin = nullptr;
    int32_t *unmet = nullptr;
};

// One call on its way through qary_run's steps.
struct QaryCall {
    hipStream_t s = nullptr;
    int batch = 0, BV = 0, iters = 1;  // BV: coefficient variables; the loop body runs at least once (decoder.rs:578-579)
    long Bp = 0;                       // batch rounded up to whole waves
    bool dev_io = false;
    QaryPlan plan;
    SoftOut so;
    const float *dp_b = nullptr, *dp_s = nullptr;  // the probabilities on the device
    signed char *dout = nullptr;                   // the symbols [batch][N] on the device
    bool want_cost() const { return so.cost_b != nullptr; }
    bool want_margin() const { return so.margin != nullptr; }
    size_t n_pmf_b(const scaldpc_qary *h) const { return (size_t)batch * BV * h->Q; }  // floats of the coefficient rows' input (and cost table)
    size_t n_pmf_s(const scaldpc_qary *h) const { return h->special ? (size_t)batch * h->R * h->QS : 0; }
};

// Everything the call will touch, before anything is queued.
int ensure_buffers(scaldpc_qary *h, const QaryCall &c)
{
    if (c.Bp > h->cap_bp) {
        h->d_msg.reset(); h->d_llr.reset(); h->d_hard.reset();
        h->cap_bp = 0;
        SC_TRY(h->d_msg.ensure((size_t)std::max(h->E, 1) * h->W * c.Bp));
        SC_TRY(h->d_llr.ensure((size_t)h->llr_rows * c.Bp));
        SC_TRY(h->d_hard.ensure((size_t)h->N * c.Bp));
        h->cap_bp = c.Bp;
    }
    if (c.want_cost()) {
        SC_TRY(h->d_cost.ensure((size_t)h->llr_rows * c.Bp));
        if (!c.dev_io) SC_TRY(h->d_cost_out.ensure((size_t)c.batch * h->llr_rows));
    }
    if (c.want_margin()) {
        SC_TRY(h->d_margin.ensure((size_t)h->N * c.Bp));
        if (!c.dev_io) SC_TRY(h->d_margin_out.ensure((size_t)c.batch * h->N));
    }
    if (c.dev_io) return 0;
    if (c.so.unmet) SC_TRY(h->d_unmet.ensure(c.batch));
    SC_TRY(h->d_pmf.ensure(c.n_pmf_b(h)));
    if (h->special) SC_TRY(h->d_pmf2.ensure(c.n_pmf_s(h)));
    return h->d_out.ensure((size_t)c.batch * h->N);
}

// One alphabet's rows of a conversion: nv variables of Q symbols from graph variable vbase on (kind 0: coefficient rows, 1: row-sum rows).
struct LlrSeg {
    const float *pmf;
    int nv, Q, kind, vbase;
    float *llr;
};

// k_q_into_llr_tiled over one alphabet or both (b != nullptr); fused: it writes the first messages too.
void launch_llr_tiled(scaldpc_qary *h, const QaryCall &c, const LlrSeg &a, const LlrSeg *b, bool fused)
{
    const int VT0 = std::max(1, 32 / a.Q), nb0 = (a.nv + VT0 - 1) / VT0;
    const int VT1 = b ? std::max(1, 32 / b->Q) : 0, nb1 = b ? (b->nv + VT1 - 1) / VT1 : 0;
    hipLaunchKernelGGL(k_q_into_llr_tiled, dim3(nb0 + nb1, c.Bp / 64), dim3(64 * std::max(VT0, VT1)), 0, c.s, a.pmf, a.nv, a.Q, VT0,
                       c.batch, c.Bp, a.llr, h->d_err, h->d_first_bad, a.kind, fused ? h->d_col_ptr.get() : nullptr,
                       (const int *)h->d_csc_edge, (const int *)h->d_edge_h, h->d_msg, h->W, a.vbase, b ? nb0 : 0x7fffffff,
                       b ? b->pmf : nullptr, b ? b->nv : 0, b ? b->Q : 0, VT1, b ? b->llr : nullptr, b ? b->vbase : 0);
}

// Host inputs are staged as they are ([batch][var][Q] floats); probabilities -> LLRs and the first messages on the device.
int stage_and_convert(scaldpc_qary *h, QaryCall &c, const float *pmf_b, const float *pmf_s)
{
    c.dp_b = pmf_b;
    c.dp_s = pmf_s;
    if (!c.dev_io) {
        SC_HIP(hipMemcpyAsync(h->d_pmf, pmf_b, c.n_pmf_b(h) * sizeof(float), hipMemcpyHostToDevice, c.s));
        c.dp_b = h->d_pmf;
        if (h->special) {
            SC_HIP(hipMemcpyAsync(h->d_pmf2, pmf_s, c.n_pmf_s(h) * sizeof(float), hipMemcpyHostToDevice, c.s));
            c.dp_s = h->d_pmf2;
        }
    }
    const LlrSeg seg[2] = {{c.dp_b, c.BV, h->Q, 0, 0, h->d_llr}, {c.dp_s, h->R, h->QS, 1, c.BV, h->d_llr + (size_t)c.BV * h->Q * c.Bp}};
    if (c.plan.llr == QLlr::FUSED_BOTH) {
        launch_llr_tiled(h, c, seg[0], &seg[1], true);
        SC_HIP(hipGetLastError());
    } else
        for (int i = 0; i < (h->special ? 2 : 1); i++) {
            if (c.plan.llr == QLlr::FUSED_EACH || (i ? c.plan.llr_tiled_s : c.plan.llr_tiled_b))
                launch_llr_tiled(h, c, seg[i], nullptr, c.plan.llr == QLlr::FUSED_EACH);
            else
                hipLaunchKernelGGL(k_q_into_llr, dim3(seg[i].nv, c.Bp / 64), dim3(64), 0, c.s, seg[i].pmf, seg[i].nv, seg[i].Q, c.batch,
                                   c.Bp, seg[i].llr, h->d_err, h->d_first_bad, seg[i].kind);
            SC_HIP(hipGetLastError());
        }
    if (c.plan.init) {
        hipLaunchKernelGGL(k_q_init, dim3(h->E, c.Bp / 64), dim3(64), 0, c.s, h->d_edge_var, h->d_edge_h, h->d_var_q, h->d_var_off,
                           h->d_llr, h->d_msg, h->W, c.Bp);
        SC_HIP(hipGetLastError());
    }
    return 0;
}

void launch_check(scaldpc_qary *h, const QaryCall &c)
{
    const QaryPlan &p = c.plan;
    const hipStream_t s = c.s;
    // kernels of more than one instantiation: one launch site per signature
    const auto rows = [&](auto kernel) {  // lane = codeword, registers only
        hipLaunchKernelGGL(kernel, dim3(h->R, c.Bp / 64), dim3(64), 0, s, h->d_row_ptr, h->d_msg, c.Bp, c.batch, h->d_err);
    };
    const auto special_dp = [&](auto kernel, int parts) {
        hipLaunchKernelGGL(kernel, dim3(h->R, c.Bp / 64), dim3(64 * parts), 0, s, h->d_row_ptr, h->d_msg, h->BSUM, h->W, c.Bp, c.batch);
    };
    const auto lane = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(h->R, c.Bp / p.T), dim3(p.T), p.check_lds, s, h->d_row_ptr, h->d_msg, h->Q, h->B, c.Bp, c.batch,
                           h->maxdc, h->d_err);
    };
    const auto special_any = [&](auto kernel) {  // lane = codeword, tables in LDS
        hipLaunchKernelGGL(kernel, dim3(h->R, c.Bp / 64), dim3(64), p.dp_any_lds, s, h->d_row_ptr, h->d_msg, h->BSUM, h->W, c.Bp, c.batch,
                           (int)(p.dp_any_lds / (3 * 64 * 4)));
    };
    // the special decoder's wave kernel: the form itself, or behind the tree walk / the min-plus recursion for the rows they leave
    bool special_wave = p.wave_fallback_nb >= 0;
    switch (p.check) {
        case QCheck::NONE: return;
        case QCheck::DP_3_7: rows(k_q_check_dp<3, 7>); break;
        case QCheck::UNROLLED_3_7: rows(k_q_check_unrolled<3, 7>); break;
        case QCheck::UNROLLED_5_5: rows(k_q_check_unrolled<5, 5>); break;
        case QCheck::SPECIAL_DP:
            // (a few dozen codewords: four waves per (check, 64 codewords); a few hundred: two)
            if (p.check_parts == 4) special_dp(k_q_special_check_dp<5, 6, 4>, 4);
            else if (p.check_parts == 2) special_dp(k_q_special_check_dp<5, 6, 2>, 2);
            else special_dp(k_q_special_check_dp<5, 6, 1>, 1);
            break;
        case QCheck::SPECIAL_DP_ANY:
            if (h->Q == 3) special_any(k_q_special_check_dp_any<3>);
            else if (h->Q == 5) special_any(k_q_special_check_dp_any<5>);
            else special_any(k_q_special_check_dp_any<7>);
            break;
        case QCheck::SPECIAL_TREE:
            hipLaunchKernelGGL((k_q_special_check_tree<5, 6>), dim3(h->R, c.batch), dim3(64), p.tree_lds, s, h->d_row_ptr, h->d_msg,
                               h->BSUM, h->W, c.Bp);
            break;
        case QCheck::SPECIAL_WAVE: special_wave = true; break;
        case QCheck::WAVE:
            hipLaunchKernelGGL(k_q_check_wave, dim3(h->R, c.batch), dim3(64), p.wave_lds, s, h->d_row_ptr, h->d_msg, h->Q, h->B, c.Bp,
                               h->maxdc, h->d_err);
            break;
        case QCheck::SPECIAL_LANE:
            hipLaunchKernelGGL(k_q_special_check, dim3(h->R, c.Bp / p.T), dim3(p.T), p.check_lds, s, h->d_row_ptr, h->d_msg, h->B, h->BSUM,
                               h->W, c.Bp, c.batch, h->maxdc - 1);
            break;
        case QCheck::LANE:
            if (p.check_words128) lane(k_q_check<unsigned __int128>);
            else lane(k_q_check<u64>);
            break;
    }
    if (special_wave)  // (skip_nb -1, the form itself: no row is skipped)
        hipLaunchKernelGGL(k_q_special_check_wave, dim3(h->R, c.batch), dim3(64), p.wave_lds, s, h->d_row_ptr, h->d_msg, h->B, h->BSUM,
                           h->W, c.Bp, h->maxdc - 1, p.wave_fallback_nb);
}

// SOFT: the soft form of whichever kernel the plain call runs -- totals (dc) and margins (dm) staged next to the symbols.
template <bool SOFT>
void launch_var(scaldpc_qary *h, const QaryCall &c, int last, float *dc = nullptr, float *dm = nullptr)
{
    const auto small = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(h->N, c.Bp / 64), dim3(64), 0, c.s, h->d_col_ptr, h->d_csc_edge, h->d_edge_h, h->d_llr, h->d_msg,
                           c.Bp, c.batch, last, h->d_hard, dc, dm);
    };
    switch (c.plan.var) {
        case QVar::SMALL:
            if (h->Q == 3) small(k_q_var_small<3, 4, SOFT>);
            else if (h->Q == 5) small(k_q_var_small<5, 4, SOFT>);
            else if (h->Q == 7) small(k_q_var_small<7, 4, SOFT>);
            else small(k_q_var_small<15, 4, SOFT>);
            break;
        case QVar::SMALL_SPECIAL:
            hipLaunchKernelGGL((k_q_var_small_special<5, 4, 25, SOFT>), dim3(h->N, c.Bp / 64), dim3(64), 0, c.s, h->d_col_ptr,
                               h->d_csc_edge, h->d_edge_h, h->d_llr, h->d_msg, c.BV, h->W, c.Bp, c.batch, last, h->d_hard, dc, dm);
            break;
        case QVar::GENERIC:
            hipLaunchKernelGGL(k_q_var<SOFT>, dim3(h->N, c.Bp / c.plan.var_T), dim3(c.plan.var_T), c.plan.var_lds, c.s, 0, h->d_col_ptr,
                               h->d_csc_edge, h->d_edge_h, h->d_var_q, h->d_var_off, h->d_llr, h->d_msg, h->W, c.Bp, c.batch, h->W, last,
                               h->d_hard, dc, dm);
            break;
    }
}

// The iterations: check pass, variable pass.  With the timing knob every launch is bracketed by events:
// tev[2 it], tev[2 it + 1]: before iteration it's check / variable pass;  tev[2 iters]: the end;  tev[2 iters + 1]: the start.
int iterate(scaldpc_qary *h, const QaryCall &c)
{
    const int iters = c.iters;
    const bool timing = h->kn.timing != 0;
    if (timing) {
        while (h->tev.size() < (size_t)2 * iters + 2) {
            hipEvent_t e;
            SC_HIP(hipEventCreate(&e));
            h->tev.push_back(e);
        }
        SC_HIP(hipEventRecord(h->tev[2 * iters + 1], c.s));  // start of the call's device work is behind us: into_llr + init
    }
    for (int it = 1; it <= iters; it++) {
        if (timing) SC_HIP(hipEventRecord(h->tev[2 * (it - 1)], c.s));
        if (c.plan.check != QCheck::NONE) {
            launch_check(h, c);
            SC_HIP(hipGetLastError());
        }
        if (timing) SC_HIP(hipEventRecord(h->tev[2 * (it - 1) + 1], c.s));
        if (it == iters && (c.want_cost() || c.want_margin()))
            launch_var<true>(h, c, 1, c.want_cost() ? h->d_cost.get() : nullptr, c.want_margin() ? h->d_margin.get() : nullptr);
        else
            launch_var<false>(h, c, it == iters ? 1 : 0);
        SC_HIP(hipGetLastError());
    }
    if (timing) SC_HIP(hipEventRecord(h->tev[2 * iters], c.s));
    return 0;
}

// Symbols and soft outputs into the caller's layout and memory, with the status block; returns with the stream drained.
int emit(scaldpc_qary *h, QaryCall &c, int8_t *out, u64 (&status)[2])
{
    const hipStream_t s = c.s;
    const int batch = c.batch;
    const long Bp = c.Bp;
    const size_t nb = c.n_pmf_b(h), n_cost = (size_t)batch * h->llr_rows, n_margin = (size_t)batch * h->N;
    c.dout = c.dev_io ? (signed char *)out : h->d_out.get();
    hipLaunchKernelGGL(k_q_unpack, dim3((h->N + 255) / 256, batch), dim3(256), 0, s, h->d_hard, h->N, batch, Bp, c.dout);
    SC_HIP(hipGetLastError());
    if (c.want_cost() || c.want_margin()) {
        // staging [row][Bp] -> [batch][rows]: the cost table (two row ranges for DecoderSpecial) and the margins, one launch
        float *oc = c.dev_io ? c.so.cost_b : h->d_cost_out.get(), *ocs = c.dev_io ? c.so.cost_s : h->d_cost_out.get() + nb;
        SoftSegs sg = {};
        if (c.want_cost()) {
            sg.src[0] = h->d_cost; sg.dst[0] = oc; sg.rows[0] = c.BV * h->Q;
            if (h->special) { sg.src[1] = h->d_cost + (size_t)c.BV * h->Q * Bp; sg.dst[1] = ocs; sg.rows[1] = h->R * h->QS; }
        }
        if (c.want_margin()) { sg.src[2] = h->d_margin; sg.dst[2] = c.dev_io ? c.so.margin : h->d_margin_out.get(); sg.rows[2] = h->N; }
        for (int i = 0; i < 3; i++) sg.tile0[i + 1] = sg.tile0[i] + (sg.rows[i] + 63) / 64;
        hipLaunchKernelGGL(k_q_soft_transpose, dim3(sg.tile0[3], Bp / 64), dim3(256), 0, s, sg, batch, Bp);
        SC_HIP(hipGetLastError());
    }
    if (c.so.unmet) {
        int *du = c.dev_io ? c.so.unmet : h->d_unmet.get();
        SC_HIP(hipMemsetAsync(du, 0, (size_t)batch * sizeof(int), s));
        hipLaunchKernelGGL((k_q_unmet<8>), dim3((h->R + 7) / 8, Bp / 64), dim3(64), 0, s, h->d_row_ptr, h->d_edge_var, h->d_edge_h,
                           h->d_hard, h->R, batch, Bp, du);
        SC_HIP(hipGetLastError());
    }
    SC_HIP(hipMemcpyAsync(status, h->d_status, sizeof(status), hipMemcpyDeviceToHost, s));
    if (!c.dev_io) {
        SC_HIP(hipMemcpyAsync(out, c.dout, (size_t)batch * h->N, hipMemcpyDeviceToHost, s));
        if (c.want_cost()) {
            SC_HIP(hipMemcpyAsync(c.so.cost_b, h->d_cost_out, nb * sizeof(float), hipMemcpyDeviceToHost, s));
            if (h->special) SC_HIP(hipMemcpyAsync(c.so.cost_s, h->d_cost_out + nb, (n_cost - nb) * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        if (c.want_margin()) SC_HIP(hipMemcpyAsync(c.so.margin, h->d_margin_out, n_margin * sizeof(float), hipMemcpyDeviceToHost, s));
        if (c.so.unmet) SC_HIP(hipMemcpyAsync(c.so.unmet, h->d_unmet, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    SC_HIP(hipStreamSynchronize(s));
    return 0;
}

// The timing sums (with the knob) and the call's verdict out of the status block.
int report(scaldpc_qary *h, const QaryCall &c, const u64 (&status)[2])
{
    if (h->kn.timing) {
        h->stat_ms_check = h->stat_ms_var = 0.f;
        for (int it = 0; it < c.iters; it++) {
            float a = 0.f, b = 0.f;
            SC_HIP(hipEventElapsedTime(&a, h->tev[2 * it], h->tev[2 * it + 1]));
            SC_HIP(hipEventElapsedTime(&b, h->tev[2 * it + 1], h->tev[2 * it + 2]));
            h->stat_ms_check += a;
            h->stat_ms_var += b;
        }
        SC_HIP(hipEventElapsedTime(&h->stat_ms_call, h->tev[2 * c.iters + 1], h->tev[2 * c.iters]));
        h->stat_iters = c.iters;
        h->stat_kernel = (int)c.plan.check;
        h->stat_batch = c.batch;
    }
    const int err = (int)(unsigned)status[1];
    const u64 bad = ~status[0];
    if (err == QERR_PMF) {
        const int bb = (int)(bad >> 32), vv = (int)((bad & 0x7fffffffull) >> 1) + (((bad >> 31) & 1) ? c.BV : 0);
        if (bad & 1) return fail(SCALDPC_EPMF, "No maximum probability found (codeword %d, variable %d)", bb, vv);
        return fail(SCALDPC_EPMF, "channel output of codeword %d, variable %d does not sum to 1 +- 1e-3 (decoder.rs:683-684)",
                    bb, vv);
    }
    if (err == QERR_NO_CONFIG)
        return fail(SCALDPC_ENOCONF, "a check node admits no finite configuration (decoder.rs:618)");
    if (err == QERR_NO_FINITE)
        return fail(SCALDPC_ENOCONF, "a message has no finite entry (the reference would not terminate, decoder.rs:368-375)");
    return 0;
}

// One call from the handle's lock to its verdict.  `prepare` makes sure of every block the call will touch (nothing is queued
// yet), `first` queues what leaves the LLRs and the first messages in the workspaces, `last` delivers the outputs and returns
// with the stream drained and the status block read.  The plan, the iterations and the verdict are the same for every entry.
template <typename Prepare, typename First, typename Last>
int qary_steps(scaldpc_qary *h, int batch, uint32_t flags, void *stream, const SoftOut &so, Prepare prepare, First first, Last last)
{
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard dg(h->device);
    QaryCall c;
    c.s = stream ? (hipStream_t)stream : h->own_stream;
    c.batch = batch;
    c.Bp = ((long)batch + 63) / 64 * 64;
    c.BV = h->special ? h->N - h->R : h->N;
    c.iters = std::max(1, h->iterations);
    c.dev_io = flags & SCALDPC_F_DEVICE_IO;
    c.so = so;
    const int refused = qary_plan(*h, h->kn, batch, &c.plan);  // (nothing is queued yet)
    if (refused == 2)
        return fail(SCALDPC_EDEGREE, "check degree %d > 8 runs on the min-plus recursion for rows of any length only, which the "
                    "dp_any knob has switched off", h->maxdc);
    if (refused)
        return fail(SCALDPC_EDEGREE, "alphabet/degree too large for the LDS-staged enumeration (%zu B per codeword)",
                    c.plan.check_lds / c.plan.T);
    SC_TRY(prepare(c));
    SC_HIP(hipMemsetAsync(h->d_status, 0, 2 * sizeof(u64), c.s));
    SC_TRY(first(c));
    SC_TRY(iterate(h, c));
    u64 status[2] = {0, 0};
    SC_TRY(last(c, status));
    return report(h, c, status);
}

int qary_run(scaldpc_qary *h, const float *pmf_b, const float *pmf_s, int batch, uint32_t flags, void *stream,
             int8_t *out, const SoftOut &so = SoftOut())
{
    if (!h || !pmf_b || !out || (h->special && !pmf_s)) return fail(SCALDPC_EINVAL, "NULL argument");
    if (batch <= 0) return fail(SCALDPC_EINVAL, "batch must be positive");
    return qary_steps(
        h, batch, flags, stream, so, [&](QaryCall &c) { return ensure_buffers(h, c); },
        [&](QaryCall &c) { return stage_and_convert(h, c, pmf_b, pmf_s); },
        [&](QaryCall &c, u64(&status)[2]) { return emit(h, c, out, status); });
}

// ---------------------------------------------------------------------------------------------- scaldpc_mc_qary_run
// The level tables of a call (0: coefficient variables, 1: DecoderSpecial's row-sum variables) and its outputs.
struct McTables {
    const float *levels[2] = {nullptr, nullptr};
    const double *weights[2] = {nullptr, nullptr};
    int K[2] = {0, 0}, Q[2] = {0, 0};
    int floats() const { return K[0] * Q[0] + K[1] * Q[1]; }
};
struct McOut {
    uint8_t *success;
    int32_t *errs, *wrong;
    uint8_t *levels;
    int8_t *symbols;
};

// Everything that can be refused about the tables, and their thresholds (mc_cumulative_thresholds, scaldpc_mc_law.h: the rule the
// binary scaldpc_mc_hqc_run_soft draws its outcomes by); nothing is queued, no handle state is touched.
int mc_law(const McTables &t, int ntab, McLaw *law)
{
    static const char *const name[2] = {"levels_b", "levels_s"};
    *law = McLaw();
    for (int i = 0; i < ntab; i++) {
        const int K = t.K[i];
        if (K < 1 || K > MC_MAX_LEVELS) return fail(SCALDPC_EINVAL, "%s: %d levels, 1 .. %d are taken", name[i], K, MC_MAX_LEVELS);
        char why[160];
        if (mc_cumulative_thresholds(name[i], t.weights[i], K, law->t[i], why, sizeof why)) return fail(SCALDPC_EINVAL, "%s", why);
        law->K[i] = K;
    }
    for (int i = 0; i < ntab; i++)
        for (int k = 0; k < t.K[i]; k++) {
            PmfScan sc;
            for (int q = 0; q < t.Q[i]; q++) sc.step(t.levels[i][(size_t)k * t.Q[i] + q]);
            if (sc.bad())
                return fail(SCALDPC_EPMF, sc.have ? "%s: level %d does not sum to 1 +- 1e-3 (decoder.rs:683-684)"
                                                  : "%s: level %d: No maximum probability found", name[i], k);
        }
    return 0;
}

// The workspaces of a device-pointer call (the pmf staging of a host call is not needed: there is no input), then the blocks of this entry.
int mc_ensure(scaldpc_qary *h, const QaryCall &c, const McTables &t, const McOut &o)
{
    QaryCall work = c;
    work.dev_io = true;
    SC_TRY(ensure_buffers(h, work));
    SC_TRY(h->d_mc_lvl.ensure((size_t)h->N * c.Bp));
    if (h->d_mc_tab.cap() < (size_t)2 * t.floats()) h->mc_tab_ok = false;
    SC_TRY(h->d_mc_tab.ensure((size_t)2 * t.floats()));
    if (c.dev_io) return 0;
    SC_TRY(h->d_mc_res.ensure((size_t)2 * c.batch + ((size_t)c.batch + 3) / 4));
    if (o.levels) SC_TRY(h->d_mc_lvl_out.ensure((size_t)c.batch * h->N));
    if (o.symbols) SC_TRY(h->d_out.ensure((size_t)c.batch * h->N));
    return 0;
}

// The tables' rows -> LLR rows (k_q_into_llr_rows: the plain call's glibc_logf(max / p); skipped when the tables are those of
// the handle's last finished call).  Returns the LLR rows on the device, [K[0]][Q[0]] then [K[1]][Q[1]].
int mc_rows(scaldpc_qary *h, const QaryCall &c, const McTables &t, float **rows)
{
    const int nt = t.floats(), nb = t.K[0] * t.Q[0];
    float *d_rows = h->d_mc_tab + nt;
    // the tables of the last finished call, bit for bit (the chunks of a sweep): their LLR rows are still there -- no copy, no conversion
    const bool kept = h->mc_tab_ok && h->mc_tab.size() == (size_t)nt && !memcmp(h->mc_tab.data(), t.levels[0], (size_t)nb * sizeof(float)) &&
                      (nt == nb || !memcmp(h->mc_tab.data() + nb, t.levels[1], (size_t)(nt - nb) * sizeof(float)));
    if (!kept) {
        h->mc_tab_ok = false;
        h->mc_tab.assign(t.levels[0], t.levels[0] + nb);
        if (t.K[1]) h->mc_tab.insert(h->mc_tab.end(), t.levels[1], t.levels[1] + (nt - nb));
        SC_HIP(hipMemcpyAsync(h->d_mc_tab, h->mc_tab.data(), (size_t)nt * sizeof(float), hipMemcpyHostToDevice, c.s));
        for (int i = 0, off = 0; i < 2 && t.K[i]; off += t.K[i] * t.Q[i], i++) {
            hipLaunchKernelGGL(k_q_into_llr_rows, dim3(1), dim3(256), 0, c.s, h->d_mc_tab + off, (long)t.K[i], t.Q[i], d_rows + off,
                               h->d_status + 2);
            SC_HIP(hipGetLastError());
        }
    }
    *rows = d_rows;
    return 0;
}

// The first step of a Monte-Carlo call: the tables' LLR rows (mc_rows), then
// k_q_mc_draw leaves in d_llr and d_msg what stage_and_convert leaves there for the materialised input (fused or not: k_q_init
// copies the same numbers), and the drawn levels in d_mc_lvl.
int mc_draw(scaldpc_qary *h, const QaryCall &c, const McTables &t, const McLaw &law, const TrialSrc &ts, uint64_t seed)
{
    float *d_rows = nullptr;
    SC_TRY(mc_rows(h, c, t, &d_rows));
    DeviceTrials tr;  // (scaldpc_trials.h)
    SC_TRY(stage_trials(h->d_trial_ids, ts, c.batch, c.s, &tr));
    const long long *const ids = tr.ids;
    const dim3 grid((h->N + 3) / 4, c.Bp / 64);
    const size_t lds = (size_t)t.floats() * sizeof(float);
    if (ids)
        hipLaunchKernelGGL(k_q_mc_draw_at, grid, dim3(256), lds, c.s, law, d_rows, t.Q[0], t.Q[1], c.BV, h->N, c.batch, c.Bp, ids,
                           (unsigned)seed, (unsigned)(seed >> 32), h->d_col_ptr, h->d_csc_edge, h->d_edge_h, h->d_llr, h->d_msg, h->W,
                           h->d_mc_lvl);
    else
        hipLaunchKernelGGL(k_q_mc_draw, grid, dim3(256), lds, c.s, law, d_rows, t.Q[0], t.Q[1], c.BV, h->N, c.batch, c.Bp, tr.first,
                           (unsigned)seed, (unsigned)(seed >> 32), h->d_col_ptr, h->d_csc_edge, h->d_edge_h, h->d_llr, h->d_msg, h->W,
                           h->d_mc_lvl);
    SC_HIP(hipGetLastError());
    return 0;
}

// The last step: the per-trial results out of the staged symbols and levels; the optional [batch][N] arrays through k_q_unpack.
// Host callers get errs, wrong and success through ONE block and one copy.  Returns with the stream drained.
int mc_emit(scaldpc_qary *h, const QaryCall &c, const McLaw &law, const McOut &o, u64 (&status)[2])
{
    const hipStream_t s = c.s;
    const int batch = c.batch;
    const size_t n_sym = (size_t)batch * h->N;
    int *d_errs = c.dev_io ? o.errs : h->d_mc_res.get(), *d_wrong = c.dev_io ? o.wrong : h->d_mc_res.get() + batch;
    unsigned char *d_success = c.dev_io ? o.success : (unsigned char *)(h->d_mc_res.get() + 2 * (size_t)batch);
    unsigned char *d_levels = c.dev_io ? o.levels : h->d_mc_lvl_out.get();
    signed char *d_symbols = c.dev_io ? (signed char *)o.symbols : h->d_out.get();
    hipLaunchKernelGGL(k_q_mc_result, dim3(c.Bp / 64), dim3(1024), 0, s, h->d_hard, h->d_mc_lvl, h->N, c.BV, law.K[0] - 1, law.K[1] - 1,
                       batch, c.Bp, d_success, d_errs, d_wrong);
    SC_HIP(hipGetLastError());
    const dim3 ug((h->N + 255) / 256, batch);
    if (o.levels) {
        hipLaunchKernelGGL(k_q_unpack, ug, dim3(256), 0, s, (const signed char *)h->d_mc_lvl.get(), h->N, batch, c.Bp, (signed char *)d_levels);
        SC_HIP(hipGetLastError());
    }
    if (o.symbols) {
        hipLaunchKernelGGL(k_q_unpack, ug, dim3(256), 0, s, h->d_hard, h->N, batch, c.Bp, d_symbols);
        SC_HIP(hipGetLastError());
    }
    SC_HIP(hipMemcpyAsync(status, h->d_status, sizeof(status), hipMemcpyDeviceToHost, s));
    const size_t n_res = (size_t)2 * batch + ((size_t)batch + 3) / 4;
    if (!c.dev_io) {
        h->mc_res.resize(n_res);
        SC_HIP(hipMemcpyAsync(h->mc_res.data(), h->d_mc_res, n_res * sizeof(int), hipMemcpyDeviceToHost, s));
        if (o.levels) SC_HIP(hipMemcpyAsync(o.levels, d_levels, n_sym, hipMemcpyDeviceToHost, s));
        if (o.symbols) SC_HIP(hipMemcpyAsync(o.symbols, d_symbols, n_sym, hipMemcpyDeviceToHost, s));
    }
    SC_HIP(hipStreamSynchronize(s));
    h->mc_tab_ok = true;
    if (!c.dev_io) {
        const int *res = h->mc_res.data();
        if (o.errs) memcpy(o.errs, res, (size_t)batch * sizeof(int));
        if (o.wrong) memcpy(o.wrong, res + batch, (size_t)batch * sizeof(int));
        memcpy(o.success, res + 2 * (size_t)batch, batch);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------- scaldpc_mc_qary_run_secret
struct McSecretOut {
    uint8_t *success;
    int32_t *wrong, *chan;
    int8_t *secret;
    uint8_t *levels;
    int8_t *symbols;
};

// The law as the kernels of scaldpc_qary_secret.h read it, in 32-bit words: the prior's Q[0] thresholds (64 bits each), then per
// table thr [K][Q] and cnt [Q] (SecretTab), then the best values, 32 bytes per table.
struct SecretLawAt {
    size_t tab[2], best, words;
};
SecretLawAt pack_secret_law(const McSecretLaw &law, std::vector<unsigned> *out)
{
    SecretLawAt at;
    size_t n = (size_t)2 * law.Q[0];
    for (int i = 0; i < 2; i++) {
        at.tab[i] = n;
        n += (size_t)law.K[i] * law.Q[i] + law.Q[i];
    }
    at.best = n;
    at.words = n + 16;
    out->assign(at.words, 0u);
    memcpy(out->data(), law.prior.data(), (size_t)law.Q[0] * sizeof(u64));
    for (int i = 0; i < 2; i++) {
        const int K = law.K[i], Q = law.Q[i];
        unsigned *thr = out->data() + at.tab[i], *cnt = thr + (size_t)K * Q;
        for (int s = 0; s < Q; s++)
            for (int k = 0; k < K; k++) {
                const u64 t = law.t[i][(size_t)s * K + k];
                thr[(size_t)k * Q + s] = t < (1ull << 32) ? (unsigned)t : 0xFFFFFFFFu;
                cnt[s] += t < (1ull << 32);
            }
        memcpy((signed char *)(out->data() + at.best) + 32 * i, law.best[i].data(), K);
    }
    return at;
}

int secret_ensure(scaldpc_qary *h, const QaryCall &c, const McTables &t, const McSecretOut &o, size_t law_words)
{
    QaryCall work = c;
    work.dev_io = true;
    SC_TRY(ensure_buffers(h, work));
    SC_TRY(h->d_mc_lvl.ensure((size_t)h->N * c.Bp));
    SC_TRY(h->d_mc_sec.ensure((size_t)h->N * c.Bp));
    if (h->d_mc_tab.cap() < (size_t)2 * t.floats()) h->mc_tab_ok = false;
    SC_TRY(h->d_mc_tab.ensure((size_t)2 * t.floats()));
    if (h->d_mc_law.cap() < law_words) h->mc_law_ok = false;
    SC_TRY(h->d_mc_law.ensure(law_words));
    if (c.dev_io) return 0;
    SC_TRY(h->d_mc_res.ensure((size_t)4 * c.batch + ((size_t)c.batch + 3) / 4));
    if (o.secret) SC_TRY(h->d_mc_sec_out.ensure((size_t)c.batch * h->N));
    if (o.levels) SC_TRY(h->d_mc_lvl_out.ensure((size_t)c.batch * h->N));
    if (o.symbols) SC_TRY(h->d_out.ensure((size_t)c.batch * h->N));
    return 0;
}

// The first step: the tables' LLR rows (mc_rows) and the law (copied unless it is the last finished call's, word for word), then
// the secret and the outcomes of the coefficient variables, then the row sums and theirs.
int secret_draw(scaldpc_qary *h, const QaryCall &c, const McTables &t, const std::vector<unsigned> &law, const SecretLawAt &at,
                const TrialSrc &ts, uint64_t seed)
{
    float *d_rows = nullptr;
    SC_TRY(mc_rows(h, c, t, &d_rows));
    DeviceTrials tr;
    SC_TRY(stage_trials(h->d_trial_ids, ts, c.batch, c.s, &tr));
    const long long *const ids = tr.ids;
    const long first_trial = tr.first;
    if (!(h->mc_law_ok && h->mc_law == law)) {
        h->mc_law_ok = false;
        h->mc_law = law;
        SC_HIP(hipMemcpyAsync(h->d_mc_law, h->mc_law.data(), at.words * sizeof(unsigned), hipMemcpyHostToDevice, c.s));
    }
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    if (ids) {
        hipLaunchKernelGGL(k_q_mc_secret_draw_at, dim3((c.BV + 3) / 4, c.Bp / 64), dim3(256), mc_secret_lds_bytes(t.K[0], t.Q[0]), c.s,
                           (const u64 *)h->d_mc_law.get(), h->d_mc_law + at.tab[0], d_rows, t.K[0], t.Q[0], c.BV, c.batch, c.Bp, ids, k0,
                           k1, h->d_col_ptr, h->d_csc_edge, h->d_edge_h, h->d_llr, h->d_msg, h->W, h->d_mc_lvl, h->d_mc_sec);
        SC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_q_mc_secret_sums_at, dim3((h->R + 3) / 4, c.Bp / 64), dim3(256), mc_secret_lds_bytes(t.K[1], t.Q[1]), c.s,
                           h->d_mc_law + at.tab[1], d_rows + t.K[0] * t.Q[0], t.K[1], t.Q[1], t.Q[0], c.BV, h->R, c.batch, c.Bp, ids, k0,
                           k1, h->d_row_ptr, h->d_edge_var, h->d_edge_h, h->d_llr, h->d_msg, h->W, h->d_mc_lvl, h->d_mc_sec);
        SC_HIP(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(k_q_mc_secret_draw, dim3((c.BV + 3) / 4, c.Bp / 64), dim3(256), mc_secret_lds_bytes(t.K[0], t.Q[0]), c.s,
                       (const u64 *)h->d_mc_law.get(), h->d_mc_law + at.tab[0], d_rows, t.K[0], t.Q[0], c.BV, c.batch, c.Bp, first_trial, k0,
                       k1, h->d_col_ptr, h->d_csc_edge, h->d_edge_h, h->d_llr, h->d_msg, h->W, h->d_mc_lvl, h->d_mc_sec);
    SC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_q_mc_secret_sums, dim3((h->R + 3) / 4, c.Bp / 64), dim3(256), mc_secret_lds_bytes(t.K[1], t.Q[1]), c.s,
                       h->d_mc_law + at.tab[1], d_rows + t.K[0] * t.Q[0], t.K[1], t.Q[1], t.Q[0], c.BV, h->R, c.batch, c.Bp, first_trial, k0,
                       k1, h->d_row_ptr, h->d_edge_var, h->d_edge_h, h->d_llr, h->d_msg, h->W, h->d_mc_lvl, h->d_mc_sec);
    SC_HIP(hipGetLastError());
    return 0;
}

// The last step: the per-trial results; the optional [batch][N] arrays through k_q_unpack.  Host callers get wrong, channel_wrong
// and success through ONE block and one copy, as mc_emit's.  Returns with the stream drained.
int secret_emit(scaldpc_qary *h, const QaryCall &c, const SecretLawAt &at, const McSecretOut &o, u64 (&status)[2])
{
    const hipStream_t s = c.s;
    const int batch = c.batch;
    const size_t n_sym = (size_t)batch * h->N;
    int *d_wrong = c.dev_io ? o.wrong : h->d_mc_res.get(), *d_chan = c.dev_io ? o.chan : h->d_mc_res.get() + 2 * (size_t)batch;
    unsigned char *d_success = c.dev_io ? o.success : (unsigned char *)(h->d_mc_res.get() + 4 * (size_t)batch);
    signed char *d_secret = c.dev_io ? (signed char *)o.secret : h->d_mc_sec_out.get();
    unsigned char *d_levels = c.dev_io ? o.levels : h->d_mc_lvl_out.get();
    signed char *d_symbols = c.dev_io ? (signed char *)o.symbols : h->d_out.get();
    hipLaunchKernelGGL(k_q_mc_secret_result, dim3(c.Bp / 64), dim3(1024), 0, s, h->d_hard, h->d_mc_lvl, h->d_mc_sec,
                       (const signed char *)(h->d_mc_law + at.best), h->N, c.BV, batch, c.Bp, d_success, d_wrong, d_chan);
    SC_HIP(hipGetLastError());
    const dim3 ug((h->N + 255) / 256, batch);
    const auto unpack = [&](const void *plane, void *out) {
        hipLaunchKernelGGL(k_q_unpack, ug, dim3(256), 0, s, (const signed char *)plane, h->N, batch, c.Bp, (signed char *)out);
    };
    if (o.secret) {
        unpack(h->d_mc_sec.get(), d_secret);
        SC_HIP(hipGetLastError());
    }
    if (o.levels) {
        unpack(h->d_mc_lvl.get(), d_levels);
        SC_HIP(hipGetLastError());
    }
    if (o.symbols) {
        unpack(h->d_hard.get(), d_symbols);
        SC_HIP(hipGetLastError());
    }
    SC_HIP(hipMemcpyAsync(status, h->d_status, sizeof(status), hipMemcpyDeviceToHost, s));
    const size_t n_res = (size_t)4 * batch + ((size_t)batch + 3) / 4;
    if (!c.dev_io) {
        h->mc_res.resize(n_res);
        SC_HIP(hipMemcpyAsync(h->mc_res.data(), h->d_mc_res, n_res * sizeof(int), hipMemcpyDeviceToHost, s));
        if (o.secret) SC_HIP(hipMemcpyAsync(o.secret, d_secret, n_sym, hipMemcpyDeviceToHost, s));
        if (o.levels) SC_HIP(hipMemcpyAsync(o.levels, d_levels, n_sym, hipMemcpyDeviceToHost, s));
        if (o.symbols) SC_HIP(hipMemcpyAsync(o.symbols, d_symbols, n_sym, hipMemcpyDeviceToHost, s));
    }
    SC_HIP(hipStreamSynchronize(s));
    h->mc_tab_ok = true;
    h->mc_law_ok = true;
    if (!c.dev_io) {
        const int *res = h->mc_res.data();
        if (o.wrong) memcpy(o.wrong, res, (size_t)2 * batch * sizeof(int));
        if (o.chan) memcpy(o.chan, res + 2 * (size_t)batch, (size_t)2 * batch * sizeof(int));
        memcpy(o.success, res + 4 * (size_t)batch, batch);
    }
    return 0;
}

}  // namespace

extern "C" {

int scaldpc_qary_create(int32_t R, int32_t N, int32_t B, const int8_t *H, int32_t iterations, scaldpc_qary **out)
{
    return qary_build(R, N, B, 0, false, H, iterations, out);
}

int scaldpc_qary_special_create(int32_t R, int32_t N, int32_t B, int32_t BSUM, const int8_t *H, int32_t iterations,
                                scaldpc_qary **out)
{
    return qary_build(R, N, B, BSUM, true, H, iterations, out);
}

int scaldpc_qary_into_llr(const float *pmf, int64_t rows, int32_t Q, uint32_t flags, void *stream, float *llr)
{
    if (!pmf || !llr) return fail(SCALDPC_EINVAL, "NULL argument");
    if (rows <= 0 || Q <= 0) return fail(SCALDPC_EINVAL, "rows and Q must be positive");
    const bool dev_io = flags & SCALDPC_F_DEVICE_IO;
    hipStream_t s = (hipStream_t)stream;  // NULL: the default stream (this call owns no handle)
    const size_t cnt = (size_t)rows * Q;
    Buf<float> d_l, d_p;  // (declared in reverse: released in the order d_bad, d_p, d_l, after the synchronise below)
    Buf<u64> d_bad;
    SC_TRY(d_bad.ensure(1));
    if (!dev_io) {
        SC_TRY(d_p.ensure(cnt));
        SC_TRY(d_l.ensure(cnt));
    }
    u64 bad = ~0ull;
    hipError_t e = hipMemsetAsync(d_bad, 0xFF, sizeof(u64), s);
    if (e == hipSuccess && !dev_io) e = hipMemcpyAsync(d_p, pmf, cnt * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_q_into_llr_rows, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, dev_io ? pmf : d_p, (long)rows, Q,
                           dev_io ? llr : d_l, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess && !dev_io) e = hipMemcpyAsync(llr, d_l, cnt * sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(u64), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(SCALDPC_EHIP, "into_llr failed: %s", hipGetErrorString(e));
    if (bad != ~0ull) {
        if (bad & 1) return fail(SCALDPC_EPMF, "No maximum probability found (row %lld)", (long long)(bad >> 1));
        return fail(SCALDPC_EPMF, "channel output row %lld does not sum to 1 +- 1e-3 (decoder.rs:683-684)", (long long)(bad >> 1));
    }
    return 0;
}

int scaldpc_qary_configure(scaldpc_qary *h, const char *key, const char *value)
{
    if (!h || !key || !value) return fail(SCALDPC_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (!set_knob(h->kn, key, value)) return fail(SCALDPC_EINVAL, "unknown knob %s", key);
    return 0;
}

int scaldpc_qary_last_timing(scaldpc_qary *h, float *ms, int32_t *info)
{
    if (!h || !ms || !info) return fail(SCALDPC_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->stat_kernel < -1 || h->stat_iters == 0) return fail(SCALDPC_EINVAL, "no timed call yet: configure(\"timing\", \"1\") first");
    ms[0] = h->stat_ms_check;
    ms[1] = h->stat_ms_var;
    ms[2] = h->stat_ms_call;
    info[0] = h->stat_iters;
    info[1] = h->stat_kernel;
    info[2] = h->stat_batch;
    info[3] = h->maxdc;
    return 0;
}

int scaldpc_qary_min_sum_batch(scaldpc_qary *h, const float *pmf, int32_t batch, uint32_t flags, void *stream,
                               int8_t *out)
{
    if (h && h->special) return fail(SCALDPC_EINVAL, "this handle is a special decoder: use scaldpc_qary_special_min_sum_batch");
    return qary_run(h, pmf, nullptr, batch, flags, stream, out);
}

int scaldpc_qary_special_min_sum_batch(scaldpc_qary *h, const float *pmf_b, const float *pmf_sum, int32_t batch,
                                       uint32_t flags, void *stream, int8_t *out)
{
    if (h && !h->special) return fail(SCALDPC_EINVAL, "this handle is not a special decoder");
    return qary_run(h, pmf_b, pmf_sum, batch, flags, stream, out);
}

int scaldpc_qary_min_sum_batch_soft(scaldpc_qary *h, const float *pmf, int32_t batch, uint32_t flags, void *stream, int8_t *out,
                                    float *out_cost, float *out_margin, int32_t *out_unmet)
{
    if (h && h->special) return fail(SCALDPC_EINVAL, "this handle is a special decoder: use scaldpc_qary_special_min_sum_batch_soft");
    if (flags & SCALDPC_F_ASYNC) return fail(SCALDPC_EINVAL, "SCALDPC_F_ASYNC: a q-ary soft call is synchronous");
    return qary_run(h, pmf, nullptr, batch, flags, stream, out, SoftOut{out_cost, nullptr, out_margin, out_unmet});
}

int scaldpc_qary_special_min_sum_batch_soft(scaldpc_qary *h, const float *pmf_b, const float *pmf_sum, int32_t batch,
                                            uint32_t flags, void *stream, int8_t *out, float *out_cost_b, float *out_cost_sum,
                                            float *out_margin, int32_t *out_unmet)
{
    if (h && !h->special) return fail(SCALDPC_EINVAL, "this handle is not a special decoder");
    if (flags & SCALDPC_F_ASYNC) return fail(SCALDPC_EINVAL, "SCALDPC_F_ASYNC: a q-ary soft call is synchronous");
    if ((out_cost_b == nullptr) != (out_cost_sum == nullptr))
        return fail(SCALDPC_EINVAL, "out_cost_b and out_cost_sum: pass both or neither");
    return qary_run(h, pmf_b, pmf_sum, batch, flags, stream, out, SoftOut{out_cost_b, out_cost_sum, out_margin, out_unmet});
}

// scaldpc_mc_qary_run and scaldpc_mc_qary_run_at: one body, the trials from either source
static int mc_qary_run_body(scaldpc_qary *h, const float *levels_b, const double *weights_b, int32_t k_b, const float *levels_s,
                            const double *weights_s, int32_t k_s, const TrialSrc &ts, int32_t batch, uint64_t seed, uint32_t flags,
                            void *stream, uint8_t *out_success, int32_t *out_errs, int32_t *out_wrong, uint8_t *out_levels,
                            int8_t *out_symbols)
{
    if (!h || !levels_b || !weights_b || !out_success) return fail(SCALDPC_EINVAL, "NULL argument");
    if (h->special && (!levels_s || !weights_s)) return fail(SCALDPC_EINVAL, "a special decoder needs levels_s and weights_s");
    if (!h->special && (levels_s || weights_s || k_s)) return fail(SCALDPC_EINVAL, "levels_s / weights_s / k_s: this handle is not a special decoder");
    if (batch <= 0) return fail(SCALDPC_EINVAL, "batch must be positive");
    char why[96];
    if (!trials_ok(ts, batch, why, sizeof why)) return fail(SCALDPC_EINVAL, "%s", why);
    if (flags & SCALDPC_F_ASYNC) return fail(SCALDPC_EINVAL, "SCALDPC_F_ASYNC: a q-ary Monte-Carlo call is synchronous");
    McTables t;
    t.levels[0] = levels_b; t.weights[0] = weights_b; t.K[0] = k_b; t.Q[0] = h->Q;
    if (h->special) { t.levels[1] = levels_s; t.weights[1] = weights_s; t.K[1] = k_s; t.Q[1] = h->QS; }
    McLaw law;
    SC_TRY(mc_law(t, h->special ? 2 : 1, &law));
    const McOut o = {out_success, out_errs, out_wrong, out_levels, out_symbols};
    return qary_steps(
        h, batch, flags, stream, SoftOut(), [&](QaryCall &c) { return mc_ensure(h, c, t, o); },
        [&](QaryCall &c) { return mc_draw(h, c, t, law, ts, seed); },
        [&](QaryCall &c, u64(&status)[2]) { return mc_emit(h, c, law, o, status); });
}

int scaldpc_mc_qary_run(scaldpc_qary *h, const float *levels_b, const double *weights_b, int32_t k_b, const float *levels_s,
                        const double *weights_s, int32_t k_s, int64_t first_trial, int32_t batch, uint64_t seed, uint32_t flags,
                        void *stream, uint8_t *out_success, int32_t *out_errs, int32_t *out_wrong, uint8_t *out_levels,
                        int8_t *out_symbols)
{
    return mc_qary_run_body(h, levels_b, weights_b, k_b, levels_s, weights_s, k_s, TrialSrc::range(first_trial), batch, seed, flags, stream,
                            out_success, out_errs, out_wrong, out_levels, out_symbols);
}

int scaldpc_mc_qary_run_at(scaldpc_qary *h, const float *levels_b, const double *weights_b, int32_t k_b, const float *levels_s,
                           const double *weights_s, int32_t k_s, const int64_t *trial_ids, int32_t batch, uint64_t seed, uint32_t flags,
                           void *stream, uint8_t *out_success, int32_t *out_errs, int32_t *out_wrong, uint8_t *out_levels,
                           int8_t *out_symbols)
{
    return mc_qary_run_body(h, levels_b, weights_b, k_b, levels_s, weights_s, k_s, TrialSrc::list(trial_ids), batch, seed, flags, stream,
                            out_success, out_errs, out_wrong, out_levels, out_symbols);
}

// scaldpc_mc_qary_run_secret and scaldpc_mc_qary_run_secret_at: one body, the trials from either source
static int mc_qary_run_secret_body(scaldpc_qary *h, const double *prior_b, const float *levels_b, const double *weights_b, int32_t k_b,
                                   const float *levels_s, const double *weights_s, int32_t k_s, const TrialSrc &ts, int32_t batch,
                                   uint64_t seed, uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_wrong,
                                   int32_t *out_channel_wrong, int8_t *out_secret, uint8_t *out_levels, int8_t *out_symbols)
{
    if (!h || !out_success) return fail(SCALDPC_EINVAL, "NULL argument");
    if (!h->special)
        return fail(SCALDPC_EINVAL, "this handle is not a special decoder: without row-sum variables a drawn secret is no code word");
    McTables t;
    t.levels[0] = levels_b; t.weights[0] = weights_b; t.K[0] = k_b; t.Q[0] = h->Q;
    t.levels[1] = levels_s; t.weights[1] = weights_s; t.K[1] = k_s; t.Q[1] = h->QS;
    McSecretLaw law;
    char why[200];
    // (a list's own refusals come first: mc_qary_secret_law knows a first index only, and is given a legal one)
    if (ts.listed && !trials_ok(ts, batch, why, sizeof why)) return fail(SCALDPC_EINVAL, "%s", why);
    if (const int kind = mc_qary_secret_law(prior_b, t.levels, t.weights, t.K, t.Q, (long long)ts.first, batch, (flags & SCALDPC_F_ASYNC) != 0,
                                            &law, why, sizeof why))
        return fail(kind == MC_SECRET_EPMF ? SCALDPC_EPMF : kind == MC_SECRET_EDEGREE ? SCALDPC_EDEGREE : SCALDPC_EINVAL, "%s", why);
    std::vector<unsigned> words;
    const SecretLawAt at = pack_secret_law(law, &words);
    const McSecretOut o = {out_success, out_wrong, out_channel_wrong, out_secret, out_levels, out_symbols};
    return qary_steps(
        h, batch, flags, stream, SoftOut(), [&](QaryCall &c) { return secret_ensure(h, c, t, o, at.words); },
        [&](QaryCall &c) { return secret_draw(h, c, t, words, at, ts, seed); },
        [&](QaryCall &c, u64(&status)[2]) { return secret_emit(h, c, at, o, status); });
}

int scaldpc_mc_qary_run_secret(scaldpc_qary *h, const double *prior_b, const float *levels_b, const double *weights_b, int32_t k_b,
                               const float *levels_s, const double *weights_s, int32_t k_s, int64_t first_trial, int32_t batch,
                               uint64_t seed, uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_wrong,
                               int32_t *out_channel_wrong, int8_t *out_secret, uint8_t *out_levels, int8_t *out_symbols)
{
    return mc_qary_run_secret_body(h, prior_b, levels_b, weights_b, k_b, levels_s, weights_s, k_s, TrialSrc::range(first_trial), batch, seed,
                                   flags, stream, out_success, out_wrong, out_channel_wrong, out_secret, out_levels, out_symbols);
}

int scaldpc_mc_qary_run_secret_at(scaldpc_qary *h, const double *prior_b, const float *levels_b, const double *weights_b, int32_t k_b,
                                  const float *levels_s, const double *weights_s, int32_t k_s, const int64_t *trial_ids, int32_t batch,
                                  uint64_t seed, uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_wrong,
                                  int32_t *out_channel_wrong, int8_t *out_secret, uint8_t *out_levels, int8_t *out_symbols)
{
    return mc_qary_run_secret_body(h, prior_b, levels_b, weights_b, k_b, levels_s, weights_s, k_s, TrialSrc::list(trial_ids), batch, seed,
                                   flags, stream, out_success, out_wrong, out_channel_wrong, out_secret, out_levels, out_symbols);
}

void scaldpc_qary_destroy(scaldpc_qary *h)
{
    if (!h) return;
    DeviceGuard dg(h->device);
    delete h;  // the buffers, then the stream and events (QaryStreams)
}

}  // extern "C"
