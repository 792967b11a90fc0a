// Device code of the binary BP path (included by scaldpc_bp.hip, which holds the handle,
// the scheduling and the C ABI).  Everything lives in an anonymous namespace of that one
// translation unit; the split is for reading, not for linking.
#pragma once
#include "scaldpc_logf.h"  // glibc's logf on the device (k_soft_convert)
#include "scaldpc_mc_law.h"  // McHqcLaw: the outcome table k_mc_hqc_outcome takes by value
#include "scaldpc_philox.h"
#include "scaldpc_mc_draw.h"  // the bodies of the K6 generators, over the source of the trial index
#include "scaldpc_rec_pack.h"  // row words of the record form's variable pass
#include "scaldpc_rec_trim.h"  // rows of the record form's check pass that end in a constant edge
#include <type_traits>

// v_writelane_b32 as an instruction the COMPILER emits: ROCm 7.2's clang has no __builtin_amdgcn_writelane, but the LLVM
// intrinsic is reachable through an asm label.  Unlike an `asm("v_writelane_b32 ...")` statement the hazard recogniser
// sees its SGPR operand, so the 2 wait states gfx950 needs between a VALU write of an SGPR (v_cmp, v_readlane -- e.g. a
// spill reload the register allocator put there) and this VALU read of it are padded (profiles/isa_lint.py
// checks the built code object).
extern "C" __device__ int scaldpc_llvm_writelane(int src, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

namespace {

__device__ __forceinline__ unsigned writelane(unsigned src, int lane, unsigned old)
{
    return (unsigned)scaldpc_llvm_writelane((int)src, lane, (int)old);
}

constexpr int TW = 64;       // codewords per tile = one wavefront of lanes
constexpr int MAXB = 8;      // degree buckets per node kind
constexpr int ROW_CAP = 64;  // largest register-resident row degree (also the sign-mask width)
#ifndef REC_CHUNK
#define REC_CHUNK 8
#endif

__device__ __forceinline__ int rfl(int x) { return __builtin_amdgcn_readfirstlane(x); }

// Where a kernel takes the prior LLR of column v for codeword `lane` of tile `tl` from.  Every kernel that consumes a
// prior is ONE __global__ template whose last parameter P is the source: SharedPrior (the handle's one prior per column,
// a wave-uniform read) or SoftPrior (scaldpc_bp_decode_batch_soft).  The kernel takes a `typename P::Arg` and builds
// P{arg} in its body: for SharedPrior the argument is the bare __restrict__ pointer -- a struct passed by value would lose
// the noalias, and with it the proof that the uniform prior loads behind a message store are unclobbered (one VGPR more
// and another instruction stream in the first check passes).
struct SharedPrior {
    typedef const float *__restrict__ Arg;
    const float *prior;  // [n]
    __device__ __forceinline__ float operator()(int v, int, int) const { return prior[v]; }
};
// Per-codeword priors for the columns [first_col, first_col + cols): plane = float [tile][cols][64] of LLRs, one coalesced
// 256-B row per (tile, column) like every message access; the columns below keep the shared prior.  The address is
// selected, then ONE load issued: straight-line code in the exact-degree kernels, and no read of the plane for a column it
// does not hold.  (Measured against two other forms on the first check pass of the HQC-128 graph, 51-edge rows: a branch
// per edge, and both loads followed by a select, need 151 / 133 VGPRs and up to 1414 SGPR spills against this form's 126
// and none; profiles/soft_priors/README.md.)
// (tl counts from the first tile of the launch: the host passes the plane of that tile.)
struct SoftPrior {
    typedef SoftPrior Arg;
    const float *prior;  // [n]
    const float *plane;  // [tile][cols][64]
    int first_col, cols;
    __device__ __forceinline__ float operator()(int v, int tl, int lane) const
    {
        const float *src = v >= first_col ? plane + ((size_t)tl * cols + (v - first_col)) * 64 + lane : prior + v;
        return *src;
    }
};

// Straight-line code for a node's EXACT degree, dispatched wave-uniformly: calls f(std::integral_constant<int, D>) for
// D == deg, 1 <= D <= CAP (CAP bounds what is compiled in; any other degree does nothing).
template <int CAP, class F>
__device__ __forceinline__ void for_exact_degree(int deg, F &&f)
{
#define XD(D)                                                        \
    case D:                                                          \
        if constexpr (D <= CAP) f(std::integral_constant<int, D>{}); \
        break;
#define XD8(D) XD(D) XD(D + 1) XD(D + 2) XD(D + 3) XD(D + 4) XD(D + 5) XD(D + 6) XD(D + 7)
    switch (deg) {
        XD(1) XD(2) XD(3) XD(4) XD(5) XD(6) XD(7)
        XD8(8) XD8(16) XD8(24) XD8(32) XD8(40) XD8(48) XD8(56)
        XD(64)
        default: break;
    }
#undef XD8
#undef XD
}

// ---------------------------------------------------------------------------
// input / output reshaping
// ---------------------------------------------------------------------------
// uint8 [batch][len] (one row per codeword, as decode() receives them) -> planes [tile][x].
// wave = (tile, 16 consecutive x): lane c owns one 16-byte stretch of codeword c and fetches it WIDE.  A row starts at any
// alignment (len is odd on the HQC graphs, the caller's pointer is any), so the lane reads the five aligned dwords that
// cover its stretch, all in flight together, and shifts its 16 bytes out of them: a byte load per x (16 dependent-free
// but separate wave loads, each touching 64 cache lines for one byte apiece) made this kernel eight times slower than
// its mirror image k_unpack_bits.  A lane whose five dwords are not wholly inside [in, in + batch * len) -- the first
// stretch behind an unaligned `in`, the last 20 bytes of the array -- reads its bytes one by one: nothing outside the
// array is ever read.  Padding lanes (codeword >= batch) read nothing and ballot 0.  Lane j keeps the word of x0 + j, so
// the wave stores its words with one coalesced store.
// grid (ceil(len/64), T), block 256.
__global__ __launch_bounds__(256) void k_pack_bits(const uint8_t *__restrict__ in, int len, int batch,
                                                   u64 *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int x0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const int t = blockIdx.y;
    if (x0 >= len) return;
    const long b = (long)t * TW + lane;
    const int nx = min(16, len - x0);
    unsigned w[4] = {0u, 0u, 0u, 0u};  // the lane's bytes x0 ... x0 + 15, little endian (bytes from nx on: whatever, unused)
    if (b < batch) {
        const uint8_t *p = in + (size_t)b * len + x0;
        const size_t lo = (size_t)in, hi = lo + (size_t)batch * len, pa = (size_t)p;
        const unsigned mis = (unsigned)(pa & 3u);
        const size_t a = pa - mis;
        if (a >= lo && a + 20 <= hi) {
            const unsigned *q = (const unsigned *)a;
            unsigned d[5];
#pragma unroll
            for (int i = 0; i < 5; i++) d[i] = q[i];
#pragma unroll
            for (int i = 0; i < 4; i++) w[i] = (unsigned)(((((u64)d[i + 1]) << 32) | d[i]) >> (8u * mis));
        } else {
            for (int j = 0; j < nx; j++) w[j >> 2] |= (unsigned)p[j] << (8 * (j & 3));
        }
    }
    u64 mine = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (j >= nx) break;  // (wave-uniform)
        const u64 word = __ballot((w[j >> 2] >> (8 * (j & 3))) & 1u);
        if (lane == j) mine = word;
    }
    if (lane < nx) out[(size_t)t * len + x0 + lane] = mine;
}

// hard decision planes (XOR received planes) -> uint8 [batch][n].
// grid (ceil(n/256), T), block 256: a thread owns one variable of one tile.
__global__ __launch_bounds__(256) void k_unpack_bits(const u64 *__restrict__ hard, const u64 *__restrict__ recv,
                                                     int n, int batch, uint8_t *__restrict__ out)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int t = blockIdx.y;
    if (v >= n) return;
    u64 w = hard[(size_t)t * n + v];
    if (recv) w ^= recv[(size_t)t * n + v];
    const int nb = min(TW, batch - t * TW);
    for (int c = 0; c < nb; c++) out[(size_t)(t * TW + c) * n + v] = (uint8_t)((w >> c) & 1);
}

// posterior [tile][var][64] -> float [batch][n] via an LDS transpose of 64 vars x 64 codewords.
// grid (ceil(n/64), T), block 256.
__global__ __launch_bounds__(256) void k_unpack_llr(const float *__restrict__ post, int n, int batch,
                                                    float *__restrict__ out)
{
    __shared__ float tile[64][65];
    const int t = blockIdx.y, v0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = w; j < 64; j += 4)
        if (v0 + j < n) tile[j][lane] = post[((size_t)t * n + v0 + j) * TW + lane];
    __syncthreads();
    for (int c = w; c < 64; c += 4) {
        const long b = (long)t * TW + c;
        if (b < batch && v0 + lane < n) out[(size_t)b * n + v0 + lane] = tile[lane][c];
    }
}

// Per-codeword channel probabilities float [batch][cols] (one row per codeword, as scaldpc_bp_decode_batch_soft receives
// them) -> the LLR plane float [tile][cols][64] SoftPrior reads: k_unpack_llr's 64 x 64 LDS transpose in the other
// direction, both sides coalesced.  llr = logf((1 - p) / p) in f32 with glibc's logf and the correctly rounded division:
// value for value what prior_llrs computes on the host (p = 0 / p = 1 -> +-inf).  The lanes of a ragged last tile get
// LLR 0.  A value that is no probability (outside [0, 1], NaN) leaves the smallest such index b * cols + j in *bad
// (preset to ~0) and an LLR of 0 in the plane.
// grid (ceil(cols/64), T), block 256.
__global__ __launch_bounds__(256) void k_soft_convert(const float *__restrict__ probs, int cols, int batch,
                                                      float *__restrict__ plane, u64 *__restrict__ bad)
{
    __shared__ float tile[64][65];
    const int t = blockIdx.y, j0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < 64; c += 4) {
        const long b = (long)t * TW + c;
        float l = 0.0f;
        if (b < batch && j0 + lane < cols) {
            const size_t i = (size_t)b * cols + j0 + lane;
            const float p = probs[i];
            if (p >= 0.0f && p <= 1.0f)
                l = scaldpc::glibc_logf((1.0f - p) / p);
            else
                atomicMin(bad, (u64)i);
        }
        tile[c][lane] = l;
    }
    __syncthreads();
    for (int j = w; j < 64; j += 4)
        if (j0 + j < cols) plane[((size_t)t * cols + j0 + j) * TW + lane] = tile[lane][j];
}

// conv planes + iteration counters -> int32 iters[batch], uint8 conv[batch].  grid T, block 64.
__global__ __launch_bounds__(64) void k_unpack_state(const u64 *__restrict__ conv_bits, const int *__restrict__ iters,
                                                     int batch, int *__restrict__ out_iters,
                                                     uint8_t *__restrict__ out_conv)
{
    const int t = blockIdx.x, c = threadIdx.x;
    const long b = (long)t * TW + c;
    if (b >= batch) return;
    if (out_iters) out_iters[b] = iters[b];
    if (out_conv) out_conv[b] = (uint8_t)((conv_bits[t] >> c) & 1);
}

// ---------------------------------------------------------------------------
// A call of a handful of codewords from host buffers (the attack loop's single decode(), hqc.py:708) is
// bound by the NUMBER of launches, copies and memsets around its few iterations, so the reshaping steps
// are fused for it: one kernel in front (pack the input bytes into planes + reset the per-tile state +
// zero the hard-decision planes and the early-exit counters), one behind (decisions, posteriors,
// iteration counts and flags of every codeword into ONE buffer that travels back in one copy).
// ---------------------------------------------------------------------------
// grid ceil(max(len, n) / 64), block 256: wave = 16 consecutive positions of the one tile.
__global__ __launch_bounds__(256) void k_small_prepare(const uint8_t *__restrict__ in, int len, int batch,
                                                       u64 *__restrict__ planes, int n, u64 *__restrict__ hard,
                                                       int max_iter, u64 *__restrict__ done, u64 *__restrict__ conv,
                                                       int *__restrict__ iters, int *__restrict__ remaining, int nrem,
                                                       int *__restrict__ el_unsat, int nun)
{
    const int lane = threadIdx.x & 63;
    const int x0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const uint8_t *p = in + (size_t)(lane < batch ? lane : 0) * len;
    for (int j = 0; j < 16; j++) {
        const int x = x0 + j;
        if (x < len) {
            const u64 w = __ballot(lane < batch && (p[x] & 1));
            if (lane == 0) planes[x] = w;
        }
        if (x < n && lane == 0) hard[x] = 0;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < 64) {
            iters[threadIdx.x] = max_iter;
            const u64 pad = __ballot((int)threadIdx.x >= batch);  // padding codewords are born "done"
            if (threadIdx.x == 0) {
                done[0] = pad;
                conv[0] = 0;
            }
        }
        for (int i = threadIdx.x; i < nrem; i += 256) remaining[i] = 0;
        for (int i = threadIdx.x; i < nun; i += 256) el_unsat[i] = 0;
    }
}

// out = [bits: batch x n bytes][pad to 4][llr: batch x n floats, if post][iters: batch ints][conv: batch bytes]
// grid ceil(n / 256), block 256: thread = variable.  One tile, batch <= 8.
__global__ __launch_bounds__(256) void k_small_unpack(const u64 *__restrict__ hard, const u64 *__restrict__ recv,
                                                      const float *__restrict__ post, const u64 *__restrict__ conv_bits,
                                                      const int *__restrict__ iters, int n, int batch,
                                                      uint8_t *__restrict__ out)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const size_t bits_bytes = ((size_t)batch * n + 3) / 4 * 4;
    float *llr = (float *)(out + bits_bytes);
    int *oit = (int *)(out + bits_bytes + (post ? sizeof(float) * (size_t)batch * n : 0));
    uint8_t *ocv = (uint8_t *)(oit + batch);
    if (v < n) {
        u64 w = hard[v];
        if (recv) w ^= recv[v];
        for (int c = 0; c < batch; c++) {
            out[(size_t)c * n + v] = (uint8_t)((w >> c) & 1);
            if (post) llr[(size_t)c * n + v] = post[(size_t)v * TW + c];
        }
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < batch) {
        oit[threadIdx.x] = iters[threadIdx.x];
        ocv[threadIdx.x] = (uint8_t)((conv_bits[0] >> threadIdx.x) & 1);
    }
}

// ---------------------------------------------------------------------------
// parity of bit planes along the rows of H.
//   CHECK = false: synd[t][r] = XOR_v bits[t][v]          (received-vector mode: s = H v)
//   CHECK = true : unsat[t][w] = OR_r (synd[t][r] ^ XOR_v bits) over wave w's rows (convergence test H e == s)
// A wave takes ROWS_PER_WAVE consecutive rows of one tile, all in flight at once, its lanes
// over a row's edges: the column indices of a row are one coalesced read, the 8-byte
// plane words are gathered from L2 (n x 8 B per tile: 173 KB at HQC-128), the row parity is
// an XOR butterfly over the wave.  Every wave stores its OR of mismatches in its own slot
// (k_finalize folds the slots): no atomics, so the launch can be as wide as the row count
// allows.  (History: a row per THREAD -- 51 dependent, uncoalesced index reads -- 27.7 us per
// launch on the bench graph; 16 rows per wave one after the other with one atomicOr per wave,
// 19 us, latency-bound at one wave per SIMD; this form: see DESIGN.md.)
// grid (ceil(m / (4*ROWS_PER_WAVE)), T), block 256.
// ---------------------------------------------------------------------------
constexpr int ROWS_PER_WAVE = 4;

template <bool CHECK>
__global__ __launch_bounds__(256) void k_parity(const int *__restrict__ row_ptr, const int *__restrict__ col_idx,
                                                const u64 *__restrict__ bits, int m, int n, u64 *__restrict__ synd,
                                                u64 *__restrict__ unsat, const u64 *__restrict__ done)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.y;
    if (CHECK && done[t] == ~0ull) return;  // whole tile frozen
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave index inside the tile
    const int r0 = wv * ROWS_PER_WAVE;
    const u64 *bt = bits + (size_t)t * n;
    u64 bad = 0;
    // IL rows in flight: their index loads and plane gathers are independent, only the xor
    // butterflies are not
    constexpr int IL = 4;
    const int rend = min(r0 + ROWS_PER_WAVE, m);
    for (int rb = r0; rb < rend; rb += IL) {
        u64 a[IL];
        int ea[IL], eb[IL];
#pragma unroll
        for (int i = 0; i < IL; i++) {
            const int r = min(rb + i, rend - 1);
            ea[i] = rfl(row_ptr[r]) + lane;
            eb[i] = rb + i < rend ? rfl(row_ptr[r + 1]) : 0;
        }
#pragma unroll
        for (int i = 0; i < IL; i++) a[i] = ea[i] < eb[i] ? bt[col_idx[ea[i]]] : 0ull;  // first 64 edges of each row
#pragma unroll
        for (int i = 0; i < IL; i++)
            for (int e = ea[i] + 64; e < eb[i]; e += 64) a[i] ^= bt[col_idx[e]];  // rows wider than a wave
#pragma unroll
        for (int i = 0; i < IL; i++) {
            const int r = rb + i;
            if (r >= rend) break;
            u64 x = a[i];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) x ^= __shfl_xor(x, off);
            if (CHECK)
                bad |= x ^ synd[(size_t)t * m + r];
            else if (lane == 0)
                synd[(size_t)t * m + r] = x;
        }
    }
    if (CHECK && lane == 0) unsat[(size_t)t * (gridDim.x * 4) + wv] = bad;
}

// per-tile state reset.  grid T, block 64.
__global__ __launch_bounds__(64) void k_init_state(int batch, int max_iter, u64 *__restrict__ done,
                                                   u64 *__restrict__ conv, int *__restrict__ iters)
{
    const int t = blockIdx.x, c = threadIdx.x;
    const long b = (long)t * TW + c;
    iters[b] = max_iter;
    const u64 pad = __ballot(b >= batch);  // padding codewords are born "done"
    if (c == 0) {
        done[t] = pad;
        conv[t] = 0;
    }
}

// Latch convergence after the parity test of iteration `it`.  grid G, block 64.
//   latch = 1 (early exit): a codeword that satisfies H e == s for the first time is
//           frozen: done bit set, iters = it, its outputs are no longer overwritten.
//   latch = 0 (fixed iterations): only record whether the FINAL decision satisfies.
// *remaining += number of codewords still running.
// unsat: the `pw` per-wave words k_parity<true> just wrote for each tile (a tile it skipped
// is all done: whatever its stale words say, nothing is latched).
__global__ __launch_bounds__(64) void k_finalize(int it, int latch, u64 *__restrict__ done, u64 *__restrict__ conv,
                                                 const u64 *__restrict__ unsat, int pw, int *__restrict__ iters,
                                                 int *__restrict__ remaining)
{
    const int t = blockIdx.x, c = threadIdx.x;
    const u64 dw = done[t];
    u64 uw = 0;
    if (dw != ~0ull) {
        for (int i = c; i < pw; i += 64) uw |= unsat[(size_t)t * pw + i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) uw |= __shfl_xor(uw, off);
    }
    const u64 newly = ~dw & ~uw;
    if (latch) {
        if ((newly >> c) & 1) iters[(long)t * TW + c] = it;
        if (c == 0) {
            done[t] = dw | newly;
            conv[t] |= newly;
            const int rem = __popcll(~(dw | newly));
            if (rem) atomicAdd(remaining, rem);
        }
    } else if (c == 0) {
        conv[t] = newly;  // dw = padding here
    }
}

// k_parity<true> and k_finalize in ONE launch (the 64-codeword-tile early-exit loop: four launches per
// iteration and lane become three; the finalize kernel -- a wave per tile -- was 8.5 % of the GPU time of the
// config-5 sweep, nearly all of it waiting for a slot and for three dependent memory round trips on a chip
// the other lane keeps saturated).  Every block ORs its rows' mismatches into the tile's accumulator word
// with ONE device-scope atomic, then takes a ticket from the tile's block counter; the block that draws the
// last ticket knows every other block's OR has been performed (each waited for its own before it took its
// ticket) and latches the tile exactly as k_finalize does, then puts both words back to zero for the next
// launch.  Only atomics carry data between blocks -- performed at the device's coherence point, whatever
// XCD the blocks run on -- so no cache write-back or invalidate is involved.
//   unsat: [tile][pw] words, pw >= 4; word 0 = accumulator, word 1 = block counter; zero on entry and exit.
// grid (ceil(m / (4*ROWS_PER_WAVE)), G), block 256.
__global__ __launch_bounds__(256) void k_parity_fin(const int *__restrict__ row_ptr, const int *__restrict__ col_idx,
                                                    const u64 *__restrict__ bits, int m, int n,
                                                    const u64 *__restrict__ synd, u64 *unsat, int pw, int it, int latch,
                                                    u64 *done, u64 *conv, int *__restrict__ iters,
                                                    int *__restrict__ remaining)
{
    __shared__ u64 sbad[4];
    __shared__ int s_last;
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.y;
    const u64 dw = done[t];
    if (dw == ~0ull) return;  // whole tile frozen (uniform over the launch row: no ticket is drawn for it)
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int r0 = wv * ROWS_PER_WAVE;
    const u64 *bt = bits + (size_t)t * n;
    u64 bad = 0;
    constexpr int IL = 4;
    const int rend = min(r0 + ROWS_PER_WAVE, m);
    for (int rb = r0; rb < rend; rb += IL) {
        u64 a[IL];
        int ea[IL], eb[IL];
#pragma unroll
        for (int i = 0; i < IL; i++) {
            const int r = min(rb + i, rend - 1);
            ea[i] = rfl(row_ptr[r]) + lane;
            eb[i] = rb + i < rend ? rfl(row_ptr[r + 1]) : 0;
        }
#pragma unroll
        for (int i = 0; i < IL; i++) a[i] = ea[i] < eb[i] ? bt[col_idx[ea[i]]] : 0ull;
#pragma unroll
        for (int i = 0; i < IL; i++)
            for (int e = ea[i] + 64; e < eb[i]; e += 64) a[i] ^= bt[col_idx[e]];
#pragma unroll
        for (int i = 0; i < IL; i++) {
            const int r = rb + i;
            if (r >= rend) break;
            u64 x = a[i];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) x ^= __shfl_xor(x, off);
            bad |= x ^ synd[(size_t)t * m + r];
        }
    }
    if (lane == 0) sbad[threadIdx.x >> 6] = bad;
    __syncthreads();
    u64 *acc = unsat + (size_t)t * pw;
    if (threadIdx.x == 0) {
        const u64 b = sbad[0] | sbad[1] | sbad[2] | sbad[3];
        if (b) {
            const u64 old = atomicOr(acc, b);
            asm volatile("s_waitcnt vmcnt(0)" ::"v"((unsigned)old) : "memory");  // the OR is performed before the ticket is drawn
        }
        const unsigned tk = atomicAdd((unsigned *)(acc + 1), 1u);
        s_last = tk == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last || threadIdx.x >= 64) return;
    // the tile's last block: latch (k_finalize), and leave the two words zero for the next launch
    const int c = threadIdx.x;
    unsigned lo = 0, hi = 0;
    if (c == 0) {
        const u64 uw0 = atomicExch(acc, 0ull);
        (void)atomicExch((unsigned *)(acc + 1), 0u);
        lo = (unsigned)uw0;
        hi = (unsigned)(uw0 >> 32);
    }
    const u64 uw = ((u64)(unsigned)rfl((int)hi) << 32) | (unsigned)rfl((int)lo);
    const u64 newly = ~dw & ~uw;
    if (latch) {
        if ((newly >> c) & 1) iters[(long)t * TW + c] = it;
        if (c == 0) {
            done[t] = dw | newly;
            conv[t] |= newly;
            const int rem = __popcll(~(dw | newly));
            if (rem) atomicAdd(remaining, rem);
        }
    } else if (c == 0) {
        conv[t] = newly;  // dw = padding here
    }
}

// The convergence test of iteration it - 1 RIDING ON the check pass of iteration it (early-exit tile loop).  The test
// reads only the decisions the last variable pass wrote, the check pass only the messages: a check-pass wave has its
// row in hand anyway, so it XORs the row's decision planes (lanes over the row's edges: one coalesced index load, one
// gather, a butterfly), the block ORs its four rows' mismatches into the tile's accumulator and draws a ticket, the
// block that draws the last ticket latches the tile -- k_parity_fin's protocol word for word, minus the launch and
// minus its own pass over row_ptr.  The variable pass that follows is the first reader of the `done` mask that
// matters, and it starts after this kernel.  Iterations at which the host polls (or stops a group) keep the
// stand-alone k_parity_fin: there the verdict is needed before the next check pass would be launched.
struct FusedTest {
    const u64 *hard;  // [tile][n] decisions of iteration it_prev (the launch's first tile)
    u64 *unsat;       // [tile][pw]: word 0 accumulator, word 1 block counter; zero on entry and exit
    u64 *done, *conv; // [tile]
    int *iters;       // [tile][64]
    int *remaining;   // += codewords still running after the latch
    int n, pw, it_prev;
    int latch;        // 1 = early exit (freeze newly converged codewords), 0 = fixed iterations (record the final verdict only)
};

// Two halves, so that the atomics' round trips sit behind the wave's own row update instead of in front of it:
// fused_row_parity at the top of the kernel (its index load and gather are in flight beside the row's message
// loads), fused_commit at the bottom -- called by EVERY thread of EVERY block of the tile's launch row, rows or not.
__device__ __forceinline__ u64 fused_row_parity(const FusedTest &ft, int tl, int r, int e0, int deg,
                                                const int *__restrict__ col_idx, const u64 *__restrict__ synd, int m)
{
    if (r < 0) return 0;  // this wave has no row
    const int lane = threadIdx.x & 63;
    const u64 *bt = ft.hard + (size_t)tl * ft.n;
    u64 x = 0;
    for (int e = e0 + lane; e < e0 + deg; e += 64) x ^= bt[col_idx[e]];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x ^= __shfl_xor(x, off);
    return x ^ synd[(size_t)tl * m + r];
}

// A check launch has four times k_parity_fin's blocks per tile (1000 on the HQC-128 graph), and 1000 ORs plus 1000
// tickets on ONE address each are ~12 us of serialised atomics per tile and iteration: accumulators and counters are
// therefore SHARDED 16 ways by block index.  unsat words of a tile: [0] [1] k_parity_fin's pair (untouched here),
// [2] top counter, [4 .. 19] shard accumulators, [20 .. 35] shard counters; all zero on entry and exit.
constexpr int FT_SHARDS = 16, FT_WORDS = 36;

__device__ __forceinline__ void fused_commit(const FusedTest &ft, int tl, u64 bad, u64 dw)
{
    __shared__ u64 sbad[4];
    __shared__ int s_last;
    const int lane = threadIdx.x & 63;
    if (lane == 0) sbad[threadIdx.x >> 6] = bad;
    __syncthreads();
    u64 *w = ft.unsat + (size_t)tl * ft.pw;
    if (threadIdx.x == 0) {
        const unsigned sh = blockIdx.x & (FT_SHARDS - 1);
        const unsigned in_shard = (gridDim.x - sh + FT_SHARDS - 1) / FT_SHARDS;  // blocks of this launch row with this shard
        const unsigned shards = gridDim.x < (unsigned)FT_SHARDS ? gridDim.x : (unsigned)FT_SHARDS;
        const u64 b = sbad[0] | sbad[1] | sbad[2] | sbad[3];
        if (b) {
            const u64 old = atomicOr(w + 4 + sh, b);
            asm volatile("s_waitcnt vmcnt(0)" ::"v"((unsigned)old) : "memory");  // the OR is performed before the ticket is drawn
        }
        int last = 0;
        if (atomicAdd((unsigned *)(w + 20 + sh), 1u) == in_shard - 1)  // the shard is complete: its OR holds every block's word
            last = atomicAdd((unsigned *)(w + 2), 1u) == shards - 1;
        s_last = last;
    }
    __syncthreads();
    if (!s_last || threadIdx.x >= 64) return;
    // the tile's last block: gather the shards, latch (k_finalize), leave every word zero for the next launch
    const int c = threadIdx.x;
    u64 uw = 0;
    if (c < FT_SHARDS) {
        uw = atomicExch(w + 4 + c, 0ull);
        (void)atomicExch((unsigned *)(w + 20 + c), 0u);
    }
    if (c == 0) (void)atomicExch((unsigned *)(w + 2), 0u);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) uw |= __shfl_xor(uw, off);
    const u64 newly = ~dw & ~uw;
    if (ft.latch) {
        if ((newly >> c) & 1) ft.iters[(long)tl * TW + c] = ft.it_prev;
        if (c == 0) {
            ft.done[tl] = dw | newly;
            ft.conv[tl] |= newly;
            const int rem = __popcll(~(dw | newly));
            if (rem) atomicAdd(ft.remaining, rem);
        }
    } else if (c == 0) {
        ft.conv[tl] = newly;  // dw = padding here
    }
}

// k_parity_fin with the sharded accumulators / counters of fused_commit (tiles with at least FT_WORDS unsat words):
// the stand-alone test's own 250 ORs + 250 tickets per tile on one address pair are ~6 us of its 15.
// grid (ceil(m / (4*ROWS_PER_WAVE)), G), block 256; ft.it_prev = the iteration being tested.
__global__ __launch_bounds__(256) void k_parity_fin_sharded(const int *__restrict__ row_ptr, const int *__restrict__ col_idx,
                                                            int m, const u64 *__restrict__ synd, FusedTest ft)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.y;
    const u64 dw = ft.done[t];
    if (dw == ~0ull) return;  // whole tile frozen (uniform over the launch row: no ticket is drawn for it)
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int r0 = wv * ROWS_PER_WAVE;
    const u64 *bt = ft.hard + (size_t)t * ft.n;
    u64 bad = 0;
    constexpr int IL = 4;
    const int rend = min(r0 + ROWS_PER_WAVE, m);
    for (int rb = r0; rb < rend; rb += IL) {
        u64 a[IL];
        int ea[IL], eb[IL];
#pragma unroll
        for (int i = 0; i < IL; i++) {
            const int r = min(rb + i, rend - 1);
            ea[i] = rfl(row_ptr[r]) + lane;
            eb[i] = rb + i < rend ? rfl(row_ptr[r + 1]) : 0;
        }
#pragma unroll
        for (int i = 0; i < IL; i++) a[i] = ea[i] < eb[i] ? bt[col_idx[ea[i]]] : 0ull;
#pragma unroll
        for (int i = 0; i < IL; i++)
            for (int e = ea[i] + 64; e < eb[i]; e += 64) a[i] ^= bt[col_idx[e]];
#pragma unroll
        for (int i = 0; i < IL; i++) {
            const int r = rb + i;
            if (r >= rend) break;
            u64 x = a[i];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) x ^= __shfl_xor(x, off);
            bad |= x ^ synd[(size_t)t * m + r];
        }
    }
    fused_commit(ft, t, bad, dw);
}

// ---------------------------------------------------------------------------
// K1  initial bit-to-check messages: msg[tile][e][:] = LLR prior of the edge's column.
// grid (ceil(E/4), G), block 256 = 4 waves, wave = one 256 B edge row.
// ---------------------------------------------------------------------------
// (The body stays a function of its own, here and in check_minsum_body / bp_small_body / el_var_body: written straight
// into the entry point the same work comes out as other instructions -- profiles/bp_prior_entry/README.md.)
template <class P>
__device__ __forceinline__ void init_msg_body(const int *__restrict__ col_idx, P pr, float *__restrict__ msg, long E)
{
    const int lane = threadIdx.x & 63;
    const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    msg[((size_t)blockIdx.y * E + e) * TW + lane] = pr(col_idx[e], blockIdx.y, lane);
}
template <class P>
__global__ __launch_bounds__(256) void k_init_msg(const int *__restrict__ col_idx, float *__restrict__ msg, long E,
                                                  typename P::Arg prior_arg)
{
    init_msg_body(col_idx, P{prior_arg}, msg, E);
}

// ---------------------------------------------------------------------------
// K3  min-sum check-node update, in place.
//   c2v_k = alpha * (-1)^(s + #{k' != k : v2c_k' <= 0}) * min_{k' != k} |v2c_k'|
// The reference package obtains the exclusive minimum by a forward and a backward
// running min; min is exact, so (min1, min2, first argmin) gives the identical
// value with ONE pass over the inputs.  This LOOP form serves graphs with a row wider
// than 64 (the register-resident forms below take everything else): the second sweep
// re-reads the inputs for their signs (reading edge k before overwriting edge k keeps
// that legal in place).
// wave = (row, tile), lane = codeword.  grid (ceil(m/4), G), block 256 = 4 rows.
// ---------------------------------------------------------------------------
// FIRST: iteration 1 takes its inputs straight from the priors (v2c = prior of the edge's
// column by definition), so the message array needs no initialisation pass and is not read.
// (a soft call reads its per-codeword priors in a FIRST pass only: P = SoftPrior is instantiated for FIRST = true alone,
// here and in the other check kernels)
template <bool FIRST, class P>
__device__ __forceinline__ void check_minsum_body(const int *__restrict__ row_ptr, float *msg,
                                                  const u64 *__restrict__ synd, const u64 *__restrict__ done,
                                                  int skip_done, int m, long E, float alpha,
                                                  const int *__restrict__ col_idx, P prior)
{
    const int lane = threadIdx.x & 63;
    const int r = rfl((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));  // uniform: row_ptr / synd / done go through scalar loads
    if (r >= m) return;
    const int tl = blockIdx.y;
    if (skip_done && done[tl] == ~0ull) return;
    const int e0 = row_ptr[r];
    const int deg = row_ptr[r + 1] - e0;
    float *p = msg + ((size_t)tl * E + e0) * TW + lane;
    unsigned par = (unsigned)(synd[(size_t)tl * m + r] >> lane) & 1u;
    float m1 = FLT_MAX, m2 = FLT_MAX;
    int ix = 0;
#pragma unroll 16
    for (int k = 0; k < deg; k++) {
        const float x = FIRST ? prior(rfl(col_idx[e0 + k]), tl, lane) : p[(size_t)k * TW];
        const float a = fabsf(x);
        const unsigned n_ = x <= 0.0f;
        par ^= n_;
        const bool lt = a < m1;
        m2 = lt ? m1 : ((a < m2) ? a : m2);
        ix = lt ? k : ix;
        m1 = lt ? a : m1;
    }
    const float nalpha = -alpha;
#pragma unroll 8
    for (int k = 0; k < deg; k++) {
        const unsigned b = (unsigned)((FIRST ? prior(rfl(col_idx[e0 + k]), tl, lane) : p[(size_t)k * TW]) <= 0.0f);
        p[(size_t)k * TW] = ((k == ix) ? m2 : m1) * ((par ^ b) ? nalpha : alpha);
    }
}
template <bool FIRST, class P>
__global__ __launch_bounds__(256) void k_check_minsum(const int *__restrict__ row_ptr, float *msg,
                                                      const u64 *__restrict__ synd, const u64 *__restrict__ done,
                                                      int skip_done, int m, long E, float alpha,
                                                      const int *__restrict__ col_idx, typename P::Arg prior_arg)
{
    check_minsum_body<FIRST>(row_ptr, msg, synd, done, skip_done, m, E, alpha, col_idx, P{prior_arg});
}

// Register-resident form for rows of degree <= 64: straight-line code instantiated for the
// row's EXACT degree (dispatched wave-uniformly, as in k_check_tanh below): all of the row's
// loads are issued before the first compare, the recurrences are the loop kernel's own, so the
// results are identical.  One descriptor per wave of the launch {row or -1, first edge,
// degree, bound} through scalar loads.  (The loop kernel keeps 8-16 loads in flight: 61.2 us
// per 4-tile launch against this form's -- see DESIGN.md.)
template <int DEG, bool FIRST, class P>
__device__ __forceinline__ void check_minsum_row(float *p, unsigned par, float alpha, P prior, const int *__restrict__ cidx,
                                                 int tl, int lane)
{
    float x[DEG];
#pragma unroll
    for (int k = 0; k < DEG; k++) x[k] = FIRST ? prior(rfl(cidx[k]), tl, lane) : p[(size_t)k * TW];
    float m1 = FLT_MAX, m2 = FLT_MAX;
    int ix = 0;
#pragma unroll
    for (int k = 0; k < DEG; k++) {
        const float a = fabsf(x[k]);
        par ^= (unsigned)(x[k] <= 0.0f);
        const bool lt = a < m1;
        m2 = lt ? m1 : ((a < m2) ? a : m2);
        ix = lt ? k : ix;
        m1 = lt ? a : m1;
    }
    const float nalpha = -alpha;
#pragma unroll
    for (int k = 0; k < DEG; k++)
        p[(size_t)k * TW] = ((k == ix) ? m2 : m1) * ((par ^ (unsigned)(x[k] <= 0.0f)) ? nalpha : alpha);
}

// PAR: the convergence test of the previous iteration rides on this pass (fused_test; early-exit runs, never FIRST).
template <int CAP, bool FIRST, bool PAR, class P>
__global__ __launch_bounds__(256) void k_check_minsum_x(const int *__restrict__ list, float *msg,
                                                        const u64 *__restrict__ synd, const u64 *done,
                                                        int skip_done, int m, long E, float alpha,
                                                        const int *__restrict__ col_idx, typename P::Arg prior_arg,
                                                        FusedTest ft)
{
    const P prior{prior_arg};
    const int lane = threadIdx.x & 63;
    const int tl = blockIdx.y;
    const int *md = list + (size_t)rfl((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 4;  // uniform address: scalar loads
    u64 dw = 0;
    if constexpr (PAR) {
        dw = done[tl];
        if (skip_done && dw == ~0ull) return;  // (uniform over the tile's blocks: no ticket is drawn for a frozen tile)
    } else {
        if (skip_done && done[tl] == ~0ull) return;
    }
    const int r = md[0];
    u64 bad = 0;
    if constexpr (PAR) bad = fused_row_parity(ft, tl, r, md[1], md[2], col_idx, synd, m);
    if (!PAR && r < 0) return;
    if (r >= 0) {
        const int e0 = md[1];
        const int deg = md[2];
        float *p = msg + ((size_t)tl * E + e0) * TW + lane;
        const unsigned sbit = (unsigned)(synd[(size_t)tl * m + r] >> lane) & 1u;
        for_exact_degree<CAP>(deg, [&](auto d) { check_minsum_row<d, FIRST>(p, sbit, alpha, prior, col_idx + e0, tl, lane); });
    }
    if constexpr (PAR) fused_commit(ft, tl, bad, dw);
}

// ---------------------------------------------------------------------------
// RECORD form of the min-sum check update (rows of degree <= 64).  A min-sum check sends only TWO magnitudes -- the
// smallest incoming |x| to every edge but the arg-min, the second smallest to that one -- and a sign per edge.  Instead
// of 4 B per edge and codeword (which the variable pass reads back as a gather), this pass leaves the message array
// alone and writes, per (row, tile), NOTHING per edge:
//     rec  [tile][2][row][64]  float : m1 * alpha | m2 * alpha, each with the row's PARITY in its sign bit: negative
//                                      where the syndrome bit XOR the XOR over the row's edges of (x <= 0) is 1.  The
//                                      magnitudes are never negative (and never NaN: clamped to FLT_MAX), so the bit
//                                      is free.  8 B per row and codeword; two dense planes per tile.  (One float2
//                                      per row and codeword -- 512-B rows, either a 4-byte gather at an 8-byte stride
//                                      or both floats in one 8-byte gather -- measured 7 % slower per step:
//                                      profiles/minsum_signed_records/README.md)
//     arg  [tile][row][64]     u8    : index IN THE ROW of the codeword's arg-min edge -- the FIRST edge whose |x|
//                                      equals m1; REC_NO_ARG where no edge attains it (all inputs NaN or infinite)
// (arg is a third plane of a tile's block of d_rec: rec_tile_floats(), scaldpc_rec_pack.h.)  The sign a check sends on
// edge e is parity XOR (x_e <= 0), and x_e is the message the VARIABLE pass itself stored on that edge one pass earlier,
// so that pass keeps the second factor, per column and contiguously:
//     sgn  [tile][position]    u64   : lane mask "the v2c message at this position of the variable pass's edge order
//                                      is <= 0" (a float compare: +-0 count, NaN does not), written by k_var_rec from
//                                      the very floats it stores
// and rebuilds every message: c2v bits = (arg-min ? rec[1] : rec[0]) bits XOR (own sgn bit << 31).  Negation is a flip of
// the sign bit (of zeros and of FLT_MAX too) and m * (-alpha) == -(m * alpha) in IEEE arithmetic, so that is the float
// k_check_minsum_x would have stored, bit for bit; the sums that follow run in the same order, so nothing about parity
// changes -- only the bytes: the check pass reads 4 B per edge and writes next to nothing, and the 2.3 MB of records
// and arg-min bytes per tile (HQC-128) are L2-sized.
// The FIRST record-form check pass of a group (BOOT) has no sgn from a k_var_rec before it -- its inputs were written
// by k_var_first or k_var -- so it also writes sgn[pos[k]] = ballot(x_k <= 0) itself, scattered by position.
// Measured before it was built: profiles/microbench/minsum_records.hip.
// ---------------------------------------------------------------------------
// The row update is written for VALU issue, which is what bounds the record-form kernels once the bytes are gone (a
// wave64 instruction holds its SIMD for 4 cycles).  Per-lane state is the two minima and the arg-min index; the parity
// is one bit per codeword and lives in a 64-bit SCALAR lane mask:
//   sweep 1, per edge: negative? -> v_cmp into a mask, parity ^= mask (scalar); |x| clamped to FLT_MAX (v_min: a NaN
//            or infinite input never wins a strict compare against minima that start at FLT_MAX, so the clamp changes
//            nothing the loop form computes), m2 = med3(a, m1, m2), m1 = min(m1, a)  -- the compare-select recurrences
//            of k_check_minsum_x, value for value (a < m1: m2 takes the old m1; m1 <= a < m2: m2 takes a; else nothing);
//   sweep 2, per edge, LAST edge first: idx = (|x_k| == m1) ? k : idx, so the first edge that attains m1 wins, as
//            `ix` did.  A compare and a select: 6 VALU instructions per edge in all.
//   BOOT only, per edge: negative? again (the inputs are still in registers) -> lane k of two registers with v_writelane.
constexpr unsigned REC_NO_ARG = 255;  // (no row has an edge 255: rows of the record form have at most 64)
static_assert(REC_TW == TW, "the record layout of scaldpc_rec_pack.h is laid out for the kernels' tile width");

// SETTLED codewords (fixed-iteration calls).  After check pass t the whole message state of a codeword is
// (rec, arg, sgn).  Test t asks: did check pass t store the records and arg-min bytes it overwrote, and did variable pass
// t - 1 store the sign masks it overwrote, bit for bit?  Then the check-to-variable messages of t are those of t - 1, the
// iteration is a deterministic map of the state, and every later pass repeats: the codeword is settled at t.  A tile all
// of whose real codewords are settled at t is FROZEN at t, and every pass but the decode's last returns at once for it.
//   words [tile][SETTLE_WORDS] u32, zero at the start of a level: a wave that sees a difference in test t stores t into
//         word (block & (SETTLE_SHARDS - 1)) of its tile -- every writer of a test writes the same value, so plain stores
//         do; the shards keep a launch's few thousand stores off one address.  The words never decrease, so their maximum
//         is the last test in which something of the tile changed; a tile has a 128-B line of its own.
//   done  the latest test completed before this launch on its stream (0 = none): the tile is frozen when its maximum is
//         below it.  (A wave of check pass t may read a word another wave of the same pass has just set to t: that tile
//         changed in test t, so it was not frozen at t - 1 either and its maximum was t - 1 = done already.)
//   mark  the test this launch is a half of (0 = it is not tracked: a BOOT pass, or a pass at which alpha still moves)
// words == nullptr: all of it off.  A wave-uniform branch on a kernel argument, no instantiation of its own.
// The SPARSE gate (knob settle_sparse; the rule in full: tests/settle_sparse_ref.py, which restates it, and DESIGN.md 4).
// Long before a tile freezes most of its rows and columns have stopped changing, so a tracked pass also says WHICH nodes
// changed, and the next pass returns for the nodes none of whose inputs did:
//   rowf  [tile][m] {stamp, -, dirty lo, dirty hi}: a row that runs in tracked check pass t stores stamp = t and the mask of
//         its edges (by index in the row) whose check-to-variable message may differ from the one before in a real codeword:
//         all ones if a first record differs bit for bit (its sign bit is the row's parity), else bit(old arg) | bit(new arg)
//         over the codewords whose second record or arg-min byte differs
//   colf  [tile][n] u32: a column of degree > 1 that runs in tracked variable pass t stores t << 1 | (a sign mask it stored
//         differs from the one it overwrote in a real codeword)
//   gate  this pass returns for a row none of whose columns is stamped with the pass before (colf >> 1 == mark - 1), for a
//         column none of whose edges has its bit in a row flag stamped with this pass (stamp == mark - 1: variable pass t
//         carries mark t + 1) and whose own colf is not (t - 1) << 1 | 1.  Which passes gate: settle_sparse_*_gate.
// Plain stores, one writer per word and pass, visible at the kernel boundary on the lane's stream like the words.  A stale
// or missing stamp can only make a node run; running is always right.  rowf == nullptr: off.
constexpr int SETTLE_WORDS = 32, SETTLE_SHARDS = 8;
struct Settle {
    unsigned *words = nullptr;  // of the launch's first tile
    int done = 0, mark = 0;
    uint4 *rowf = nullptr;      // of the launch's first tile, like words
    unsigned *colf = nullptr;
    int ncol = 0, gate = 0;     // columns of the graph (colf's tile stride)
};
__device__ __forceinline__ bool settle_frozen(const unsigned *__restrict__ w, int done)
{
    unsigned mx = 0;
#pragma unroll
    for (int i = 0; i < SETTLE_SHARDS; i++) mx = w[i] > mx ? w[i] : mx;  // (uniform address: scalar loads, issued with the wave's first)
    return (int)mx < done;
}

// mark_word (steady passes only; null = not tracked): where the wave stores `mark` if a REAL codeword's records or arg-min
// byte differ from the ones it overwrites (real = lane mask of the tile's codewords that are not padding)
template <int DEG, bool BOOT>
__device__ __forceinline__ void check_minsum_row_rec(const float *p, u64 synd_mask, float alpha, float *__restrict__ rec,
                                                     float *__restrict__ rec2, unsigned char *__restrict__ arg,
                                                     u64 *__restrict__ sgn, int lane, const int *__restrict__ pos,
                                                     bool const_last = false, float x_last = 0.0f,
                                                     unsigned *mark_word = nullptr, unsigned mark = 0, u64 real = 0,
                                                     uint4 *row_flag = nullptr)
{
    // BOOT: the sign masks are laid out in the variable pass's order (position of the edge in the re-laid edge list: a
    // column's masks are contiguous there); lane k fetches edge k's position up front
    int mp = 0;
    if constexpr (BOOT)
        if (lane < DEG) mp = pos[lane];
    float x[DEG];
#pragma unroll
    for (int k = 0; k < DEG - 1; k++) x[k] = p[(size_t)k * TW];  // (plain loads: non-temporal ones cost 5-9 % and save no byte, profiles/r04/ab_rec_nontemporal.log)
    // const_last (wave-uniform: REC_CONST_LAST in the row's descriptor, shared priors): the row's LAST edge goes into a
    // column of degree 1, whose message is its prior in every pass -- iteration 1 stored prior + 0.0f there and nothing
    // has written the edge since.  x_last is that prior from a scalar load; the 256-B row of 64 equal floats stays
    // unread.  (The pass uses x through x <= 0, |x| and |x| == m1 alone: a zero's sign cannot matter.)  One uniform
    // branch, after the other edges' loads have been issued; every compare still comes behind every load.
    if (const_last)
        x[DEG - 1] = x_last;
    else
        x[DEG - 1] = p[(size_t)(DEG - 1) * TW];
    // A tracked pass (mark_word, wave-uniform) fetches the records and the arg-min byte it is about to overwrite.  Rows of up
    // to 32 edges (EARLY) issue the three loads here, with the row's own, so that their latency hides behind both sweeps:
    // those builds have registers to spare.  Longer rows fetch them late (below).
    constexpr bool EARLY = DEG <= 32;
    bool tracked = false;
    if constexpr (!BOOT) tracked = mark_word != nullptr;
    unsigned o1 = 0, o2 = 0, oa = 0;
    if constexpr (!BOOT && EARLY)
        if (tracked) {
            o1 = __float_as_uint(rec[lane]);
            o2 = __float_as_uint(rec2[lane]);
            oa = arg[lane];
        }
    float m1 = FLT_MAX, m2 = FLT_MAX;
    const float fmax = FLT_MAX;
    u64 par = ((u64)(unsigned)rfl((int)(synd_mask >> 32)) << 32) | (unsigned)rfl((int)synd_mask);  // (uniform by construction: keep it on the scalar side)
#pragma unroll
    for (int k = 0; k < DEG; k++) {
        // the sweep runs in chunks of REC_CHUNK edges: the parity is pinned down after a chunk and the next chunk's inputs
        // pass through an empty asm behind that point, so at most a chunk's sign masks are live in SGPRs.  Left alone
        // the scheduler runs the compares of the whole row ahead of the XORs (nothing wants the parity before the row's
        // end): 354 static SGPR spills in the 64-edge build, every one a v_writelane / v_readlane pair on the VALU this
        // kernel is bound by.
        if (k % REC_CHUNK == 0 && k > 0) {
            asm volatile("" : "+s"(par));
#pragma unroll
            for (int j = k; j < DEG && j < k + REC_CHUNK; j++) asm volatile("" : "+v"(x[j]));
        }
        par ^= __ballot(x[k] <= 0.0f);
        float a;
        asm("v_min_f32 %0, |%1|, %2" : "=v"(a) : "v"(x[k]), "v"(fmax));
        asm("v_med3_f32 %0, %1, %2, %0" : "+v"(m2) : "v"(a), "v"(m1));
        asm("v_min_f32 %0, %0, %1" : "+v"(m1) : "v"(a));
    }
    float s1, s2;
    {
        // the row's parity goes into the records' sign bit: one select with a negated source each, on the scalar mask
        const bool odd = __builtin_amdgcn_inverse_ballot_w64(par);
        const float r1 = m1 * alpha, r2 = m2 * alpha;
        s1 = odd ? -r1 : r1;
        s2 = odd ? -r2 : r2;
    }
    // A tracked pass over a row of more than 32 edges fetches the records it overwrites and stores the new ones eight edges
    // into sweep 2 instead of in front of it: every edge of that sweep frees a register, and in front of it the 64-edge
    // build has none to spare (its occupancy hangs on 72).  The loads are tied behind the sweep's steps so far through an
    // empty asm on their lane offset; the old arg-min byte and the compare come behind the sweep.
    if (!tracked || EARLY) {
        rec[lane] = s1;
        rec2[lane] = s2;
    }
    constexpr int AT = DEG - 8;
    unsigned idx = REC_NO_ARG;
#pragma unroll
    for (int k = DEG - 1; k >= 0; k--) {
        // (edge k's compare waits for edge k + 1's select, through an empty asm: compare and select pair up through VCC
        // instead of a run of compares ahead of the selects with a live SGPR pair each)
        asm("" : "+v"(x[k]) : "v"(idx));
        idx = (fabsf(x[k]) == m1) ? (unsigned)k : idx;
        if constexpr (!BOOT && !EARLY)
            if (k == AT && tracked) {
                int lo = lane;
                asm volatile("" : "+v"(lo) : "v"(idx));
                o1 = __float_as_uint(rec[lo]);
                o2 = __float_as_uint(rec2[lo]);
                rec[lo] = s1;
                rec2[lo] = s2;
            }
    }
    if constexpr (!BOOT) {
        if (tracked) {
            if constexpr (!EARLY) oa = arg[lane];
            arg[lane] = (unsigned char)idx;
            const u64 c1 = __ballot(o1 != __float_as_uint(s1)) & real;
            const u64 c2 = __ballot(o2 != __float_as_uint(s2) || oa != idx) & real;
            if ((c1 | c2) != 0 && lane == 0) *mark_word = mark;
            // the sparse gate's row flag (Settle): which of the row's edges may carry another message than before.  The OR of
            // the arg-min bits is built on the scalar side, one step per distinct arg value among the changed codewords, and
            // only under "no first record changed, something else did".
            if (row_flag) {
                u64 dirty = 0;
                if (c1 != 0)
                    dirty = ~0ull;
                else if (c2 != 0) {
#pragma unroll 1
                    for (int half = 0; half < 2; half++) {
                        const unsigned av = half ? idx : oa;
                        u64 rem = c2;
#pragma unroll 1
                        while (rem != 0) {
                            const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)av, rfl(__builtin_ctzll(rem)));
                            if (a < 64u) dirty |= 1ull << a;
                            rem &= ~__ballot(av == a);
                        }
                    }
                }
                if (lane == 0) *row_flag = make_uint4(mark, 0u, (unsigned)dirty, (unsigned)(dirty >> 32));
            }
        } else
            arg[lane] = (unsigned char)idx;
    } else
        arg[lane] = (unsigned char)idx;
    if constexpr (BOOT) {
        unsigned nlo = 0, nhi = 0;  // lane k keeps edge k's mask
        // The v_writelanes below are the compiler's own instructions (writelane(), top of this file): a v_writelane reading
        // an SGPR that a VALU instruction -- a v_cmp, or a v_readlane reloading a spilled mask -- wrote fewer than 2 wait
        // states earlier gets the OLD value on gfx950, and inside an `asm` statement nobody pads (round 3 measured it on
        // edge 0 of degree-1 rows: VERDICT r03 #1).
#pragma unroll
        for (int k = 0; k < DEG; k++) {
            // the sweep runs in chunks of REC_CHUNK edges: a chunk's compares wait (through an empty asm on their inputs)
            // for the previous chunk's v_writelanes, so at most a chunk's masks are live in SGPRs.  Left alone the
            // scheduler keeps sweep 1's sign masks of the whole row for reuse: SGPR spills in the 64-edge build, every
            // one a v_writelane / v_readlane pair.
            if (k % REC_CHUNK == 0) {
                asm volatile("" ::"v"(nlo), "v"(nhi));
#pragma unroll
                for (int j = k; j < DEG && j < k + REC_CHUNK; j++) asm volatile("" : "+v"(x[j]));
            }
            const u64 ng = __ballot(x[k] <= 0.0f);
            nlo = writelane((unsigned)ng, k, nlo);
            nhi = writelane((unsigned)(ng >> 32), k, nhi);
        }
        if (lane < DEG) sgn[mp] = ((u64)nhi << 32) | nlo;
    }
}

// (Iteration 1 never comes here: it runs without a check pass -- k_var_first -- or, with first_fused off, in the message
// form, whose check kernel reads the priors.)
// BOOT is the SECOND template parameter: a profile's per-kernel averages tell the one bootstrap launch of a group from
// the steady-state ones by the instantiation's name.
template <int CAP, bool BOOT, bool PAR = false>
__global__ __launch_bounds__(256) void k_check_minsum_rec(const int *__restrict__ list, const float *msg,
                                                          const u64 *__restrict__ synd, const u64 *done,
                                                          int skip_done, int m, long E, float alpha,
                                                          const int *__restrict__ col_idx,
                                                          float *__restrict__ rec, u64 *__restrict__ sgn,
                                                          const int *__restrict__ csr_pos,
                                                          const float *__restrict__ const_prior, FusedTest ft = FusedTest{},
                                                          Settle st = Settle{})
{
    const int lane = threadIdx.x & 63;
    const int tl = blockIdx.y;
    const int *md = list + (size_t)rfl((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 4;  // uniform address: scalar loads
    u64 dw = 0;
    unsigned *mark_word = nullptr;  // (settled codewords: fixed-iteration calls, which never come with PAR)
    bool sparse = false;
    if constexpr (PAR) {
        dw = done[tl];
        if (skip_done && dw == ~0ull) return;
    } else {
        if (skip_done && done[tl] == ~0ull) return;
        if (st.words) {
            unsigned *w = st.words + (size_t)tl * SETTLE_WORDS;
            if (settle_frozen(w, st.done)) return;  // the tile is frozen: this pass would store what is there
            if (!BOOT && st.mark) {
                mark_word = w + (blockIdx.x & (SETTLE_SHARDS - 1));
                dw = done[tl];  // (fixed iterations: the padding lanes)
                sparse = st.rowf != nullptr;
            }
        }
    }
    const int r = md[0];
    u64 bad = 0;
    if constexpr (PAR) bad = fused_row_parity(ft, tl, r, md[1], md[2], col_idx, synd, m);
    if (!PAR && r < 0) return;
    if (r >= 0) {
        const int e0 = md[1];
        const int deg = md[2];
        uint4 *rf = nullptr;
        if constexpr (!BOOT && !PAR)
            if (sparse) {
                // the sparse gate (Settle): lane k looks at the column of edge k; no column stamped by the variable pass
                // before = no input of the row changed, and the row would store what is there
                if (st.gate) {
                    unsigned cf = 0;
                    if (lane < deg) cf = st.colf[(size_t)tl * st.ncol + col_idx[e0 + lane]];
                    if (__ballot(lane < deg && (cf >> 1) == (unsigned)(st.mark - 1)) == 0) return;
                }
                rf = st.rowf + (size_t)tl * m + r;
            }
        const float *p = msg + ((size_t)tl * E + e0) * TW + lane;
        float *rt = rec + (size_t)tl * rec_tile_floats(m);  // the tile's block: [m1 | m2][row][64], arg
        float *rc = rt + rec_row_off(r), *rc2 = rc + rec_m2_off(m);
        unsigned char *ar = (unsigned char *)(rt + rec_arg_off(m)) + (size_t)r * TW;
        u64 *sg = sgn + (size_t)tl * E;  // (masks by position: the tile's base)
        const int *ps = csr_pos + e0;
        const u64 sw = synd[(size_t)tl * m + r];  // (uniform: a scalar load; the row's syndrome bits ARE a lane mask)
        // the constant last edge (check_minsum_row_rec): const_prior = the handle's shared priors, null in a soft call,
        // whose columns of degree 1 may carry a prior per codeword -- its rows run with all their loads
        const bool cl = const_prior != nullptr && (md[3] & REC_CONST_LAST) != 0;
        float xl = 0.0f;
        if (cl) xl = const_prior[rec_desc_col(md[3])];
        // (the ladder for_exact_degree spells, kept as a macro here and in k_var_rec: through the helper's lambda the
        // record-form kernels come out with other registers and an instruction more or less)
#define MR(D)                                                                                                   \
    case D:                                                                                                     \
        if constexpr (D <= CAP)                                                                                 \
            check_minsum_row_rec<D, BOOT>(p, sw, alpha, rc, rc2, ar, sg, lane, ps, cl, xl, mark_word, (unsigned)st.mark, ~dw, rf); \
        break;
#define MR8(D) MR(D) MR(D + 1) MR(D + 2) MR(D + 3) MR(D + 4) MR(D + 5) MR(D + 6) MR(D + 7)
        switch (deg) {
            MR(1) MR(2) MR(3) MR(4) MR(5) MR(6) MR(7)
            MR8(8) MR8(16) MR8(24) MR8(32) MR8(40) MR8(48) MR8(56)
            MR(64)
            default: break;
        }
#undef MR8
#undef MR
    }
    if constexpr (PAR) fused_commit(ft, tl, bad, dw);
}

// ---------------------------------------------------------------------------
// K2  tanh-rule (sum-product) check-node update, LLR domain, fp32, COMPLEMENT form, in place.
//   c2v_k = (-1)^(s + #{k' != k : x_k' < 0}) * 2 atanh( prod_{k' != k} tanh(|x_k'|/2) )
// computed without the 1-x cancellation that saturates the textbook form at |L|~17
// in fp32:   u_k = 1 - tanh(|x_k|/2) = 2 / (exp|x_k| + 1)
//            U   = 1 - prod(1 - u)   via  U' = U + u (1 - U)     (forward and backward)
//            |c2v_k| = log(2 / U_excl - 1),  U_excl = Upre + Usuf (1 - Upre)
// Exact for |L| up to ~88 (then u underflows to 0 and L = +inf, which is also what
// p = 0 priors feed in).  Same exclusive forward/backward sweep as the reference
// package; the CPU oracle's method 3 is this sequence op for op.
// Row values live in registers: straight-line code instantiated for the row's EXACT degree
// (1..64, dispatched wave-uniformly), sign parity carried in the float sign bits.
// ---------------------------------------------------------------------------
// Device math for the tanh rule: the hardware transcendental units (v_exp_f32,
// v_rcp_f32, v_log_f32; ~1 ulp each) instead of the ~100-instruction-per-edge
// correctly rounded expf / logf / IEEE division, which made this kernel ALU-bound once
// the messages were cache resident.  The complement form does not amplify these
// errors (|dL| stays ~1e-6 relative, tests/helpers.compare states the tolerance).
// Measured per message against the float64 closed form (tests/test_message_probes_gpu.py, rows of 2 ... 200 edges,
// |x| from 2e-3 to 85): at most 10 u, u = 2^-24 * max(1, |L|), i.e. 6e-7 * max(1, |L|); the float32 oracle with glibc's
// expf / logf and IEEE division reaches 8.4 u on the same inputs (profiles/message_probes/message_error_mi355x.txt).
__device__ __forceinline__ float tanh_compl(float a)  // 1 - tanh(a/2) = 2 / (e^a + 1), a >= 0
{
    // raw v_exp_f32: e^a >= 1 here, so the denormal fix-ups of __expf are dead weight
    return 2.0f * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(a * 1.44269504088896340736f) + 1.0f);
}
__device__ __forceinline__ float llr_from_compl(float U)  // 2 atanh(1 - U) = log(2/U - 1), U in [0, 1]
{
    // 2/U - 1 >= 1: raw v_log_f32 needs no denormal handling either
    return __builtin_amdgcn_logf(fmaf(2.0f, __builtin_amdgcn_rcpf(U), -1.0f)) * 0.69314718055994530942f;
}
// U' = U + u (1 - U), one rounding (the oracle's method 3 uses fmaf in the same places)
__device__ __forceinline__ float compl_step(float U, float u) { return fmaf(u, 1.0f - U, U); }

// FIRST: iteration 1 takes its inputs from the priors of the row's columns (cidx = the row's
// slice of col_idx), so the message array needs no initialisation pass and is not read.
template <int DEG, bool FIRST, class P>
__device__ __forceinline__ void check_tanh_row(float *p, unsigned sbit, P prior, const int *__restrict__ cidx, int tl, int lane)
{
    // EXACT degree: straight-line code, no per-edge branches (a predicated `k < deg` unroll
    // makes every edge its own basic block, and the compiler then waits for all memory
    // traffic at each block entry).
    // uu[k]: first the input x_k, then u_k >= 0 carrying the SIGN BIT of x_k (a -0.0 input
    // counts as negative here; it forces every other output of the row to +-0, so only
    // the sign of exact zeros can differ from the `x < 0` convention), finally the output.
    float uu[DEG], pre[DEG];
#pragma unroll
    for (int k = 0; k < DEG; k++) uu[k] = FIRST ? prior(rfl(cidx[k]), tl, lane) : p[(size_t)k * TW];
    unsigned acc = sbit << 31;  // running XOR of sign bits, syndrome folded in
    float U = 0.0f;
#pragma unroll
    for (int k = 0; k < DEG; k++) {
        const unsigned xb = __float_as_uint(uu[k]);
        acc ^= xb;
        const float u = tanh_compl(fabsf(uu[k]));
        uu[k] = __uint_as_float(__float_as_uint(u) | (xb & 0x80000000u));
        pre[k] = U;
        U = compl_step(U, u);
    }
    U = 0.0f;
#pragma unroll
    for (int k = DEG - 1; k >= 0; k--) {
        const float Ut = compl_step(pre[k], U);  // pre + U (1 - pre)
        const float Lm = llr_from_compl(Ut);
        const unsigned sg = (acc ^ __float_as_uint(uu[k])) & 0x80000000u;  // parity of the OTHER inputs
        U = compl_step(U, fabsf(uu[k]));
        p[(size_t)k * TW] = __uint_as_float(__float_as_uint(Lm) ^ sg);
    }
}

// Any-degree fallback: the forward sweep parks Upre in a scratch array (the reference
// package parks its prefix products in the message slot), the backward sweep re-reads
// the inputs and recomputes u before overwriting them.
__device__ __forceinline__ void check_tanh_row_generic(float *p, float *sc, int deg, unsigned sbit)
{
    float U = 0.0f;
    unsigned par = sbit;
    for (int k = 0; k < deg; k++) {
        const float x = p[(size_t)k * TW];
        sc[(size_t)k * TW] = U;
        par ^= (unsigned)(x < 0.0f);
        const float u = tanh_compl(fabsf(x));
        U = compl_step(U, u);
    }
    U = 0.0f;
    for (int k = deg - 1; k >= 0; k--) {
        const float x = p[(size_t)k * TW];
        const float pk = sc[(size_t)k * TW];
        const float Ut = compl_step(pk, U);
        const float Lm = llr_from_compl(Ut);
        p[(size_t)k * TW] = ((par ^ (unsigned)(x < 0.0f)) & 1u) ? -Lm : Lm;
        const float u = tanh_compl(fabsf(x));
        U = compl_step(U, u);
    }
}

// One fused launch over all rows (the bucket table only separates the register-resident
// rows, degree <= 64, from the any-degree fallback; its lists are sorted by degree so that
// neighbouring waves run the same instantiation).  wave = (row, tile).
// CAP = largest degree compiled in (the register budget follows the widest instantiation,
// so graphs with narrow rows get the high-occupancy build).
// grid (row descriptors / 4, G), block 256 = 4 rows of one bucket.
// PAR: the convergence test of the previous iteration rides on this pass (fused_test; early-exit runs, never FIRST).
template <int CAP, bool FIRST, bool PAR, class P>
__global__ __launch_bounds__(256) void k_check_tanh(const int *__restrict__ list, float *msg, float *scratch,
                                                    const u64 *__restrict__ synd, const u64 *done,
                                                    int skip_done, int m, long E, const int *__restrict__ col_idx,
                                                    typename P::Arg prior_arg, FusedTest ft)
{
    const P prior{prior_arg};
    const int lane = threadIdx.x & 63;
    const int tl = blockIdx.y;
    // one descriptor per WAVE of the launch: {row or -1 (padding), first edge, degree, 0 = any-degree
    // fallback}: a single load instead of bucket table -> row list -> row_ptr
    const int *md = list + (size_t)rfl((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 4;  // uniform address: scalar loads
    u64 dw = 0;
    if constexpr (PAR) {
        dw = done[tl];
        if (skip_done && dw == ~0ull) return;  // (uniform over the tile's blocks: no ticket is drawn for a frozen tile)
    } else {
        if (skip_done && done[tl] == ~0ull) return;
    }
    const int r = md[0];
    u64 bad = 0;
    if constexpr (PAR) bad = fused_row_parity(ft, tl, r, md[1], md[2], col_idx, synd, m);
    if (!PAR && r < 0) return;
    if (r >= 0) {
        const int e0 = md[1];
        const int deg = md[2];
        const size_t base = ((size_t)tl * E + e0) * TW + lane;
        float *p = msg + base;
        const unsigned sbit = (unsigned)(synd[(size_t)tl * m + r] >> lane) & 1u;
        // dispatch on the row's exact degree (wave-uniform); CAP bounds what is compiled in
        if (md[3] == 0)
            check_tanh_row_generic(p, scratch + base, deg, sbit);
        else
            for_exact_degree<CAP>(deg, [&](auto d) { check_tanh_row<d, FIRST>(p, sbit, prior, col_idx + e0, tl, lane); });
    }
    if constexpr (PAR) fused_commit(ft, tl, bad, dw);
}

// ---------------------------------------------------------------------------
// LDS-resident decoder for small graphs (the reference's own FER commands: n = 13 ... 1500,
// E <= 4500, main.py:189-276).  When a codeword's whole message state fits one CU's LDS
// (2 E floats + n + m bytes), ONE launch decodes the batch: workgroup = codeword, the
// messages never leave LDS, all iterations and the H e == s early exit run inside the
// kernel (no per-iteration launches, no host polling, no HBM/cache traffic at all).
// Threads take rows in the check phase and columns in the variable phase and sweep their
// edges sequentially in the reference package's order, so every value is bit-identical
// to the streaming kernels' (same operations, same order, same device math).
//   LDS: msg[E] (in place v2c <-> c2v), scr[E] (prefix sums / prefix products),
//        hard[n], synd[m], recv[n] (received-vector mode), flag.
// grid = batch, block = 256.
// ---------------------------------------------------------------------------
// PLANES = false: byte I/O as decode() hands it over (in: [batch][m or n], out_bits [batch][n]).
// PLANES = true : bit-plane I/O for the Monte-Carlo entry points (in = syndrome planes
//                 u64 [tile][m]; out_bits = hard planes u64 [tile][n], zeroed by the caller;
//                 out_conv = conv planes u64 [tile]; out_llr = posterior [tile][var][64]).
// Per-codeword priors (P = SoftPrior) come with either: byte I/O for scaldpc_bp_decode_batch_soft, plane I/O for
// scaldpc_mc_hqc_run_soft, whose plane the trial generator filled (a workgroup reads lane b & 63 of tile b >> 6 of it).
template <int METHOD, bool PLANES, class P>  // METHOD: SCALDPC_BP_PRODUCT_SUM / SCALDPC_BP_MIN_SUM
__device__ __forceinline__ void bp_small_body(const int *__restrict__ row_ptr, const int *__restrict__ col_idx,
                                              const int *__restrict__ col_ptr, const int *__restrict__ csc_edge,
                                              P prior, int m, int n, int E,
                                              const void *__restrict__ in_, int kind, int max_iter, float alpha0,
                                              int early, void *__restrict__ out_bits_,
                                              float *__restrict__ out_llr, int *__restrict__ out_iters,
                                              void *__restrict__ out_conv_)
{
    const uint8_t *in = (const uint8_t *)in_;
    uint8_t *out_bits = (uint8_t *)out_bits_;
    uint8_t *out_conv = (uint8_t *)out_conv_;
    const u64 *in_planes = (const u64 *)in_;
    u64 *hard_planes = (u64 *)out_bits_;
    u64 *conv_planes = (u64 *)out_conv_;
    extern __shared__ float sm[];
    float *msg = sm, *scr = sm + E;
    uint8_t *hard = (uint8_t *)(scr + E);
    uint8_t *synd = hard + n;
    uint8_t *recv = synd + m;  // n bytes, received-vector mode only
    __shared__ int flag;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int pt = b >> 6, pc = b & 63;  // tile / bit of this codeword in plane I/O

    if (PLANES) {
        for (int r = tid; r < m; r += nt) synd[r] = (uint8_t)((in_planes[(size_t)pt * m + r] >> pc) & 1);
    } else if (kind == SCALDPC_IN_SYNDROME) {
        for (int r = tid; r < m; r += nt) synd[r] = in[(size_t)b * m + r] & 1;
    } else {
        for (int v = tid; v < n; v += nt) recv[v] = in[(size_t)b * n + v] & 1;
        __syncthreads();
        for (int r = tid; r < m; r += nt) {
            uint8_t p = 0;
            for (int e = row_ptr[r]; e < row_ptr[r + 1]; e++) p ^= recv[col_idx[e]];
            synd[r] = p;
        }
    }
    for (int e = tid; e < E; e += nt) msg[e] = prior(col_idx[e], pt, pc);  // (a workgroup is a codeword: its lane of its tile)
    for (int v = tid; v < n; v += nt) hard[v] = 0;
    __syncthreads();

    int it_done = max_iter, conv = 0;
    for (int it = 1; it <= max_iter; it++) {
        const bool last = it == max_iter;
        // ---- check nodes ----
        if (METHOD == SCALDPC_BP_MIN_SUM) {
            const float alpha = alpha0 == 0.0f ? (float)(1.0 - exp2(-(double)it)) : alpha0;
            const float nalpha = -alpha;
            for (int r = tid; r < m; r += nt) {
                const int e0 = row_ptr[r], e1 = row_ptr[r + 1];
                float m1 = FLT_MAX, m2 = FLT_MAX;
                int ix = e0;
                unsigned par = synd[r];
                for (int e = e0; e < e1; e++) {
                    const float x = msg[e];
                    const float a = fabsf(x);
                    par ^= (unsigned)(x <= 0.0f);
                    const bool lt = a < m1;
                    m2 = lt ? m1 : ((a < m2) ? a : m2);
                    ix = lt ? e : ix;
                    m1 = lt ? a : m1;
                }
                for (int e = e0; e < e1; e++) {
                    const unsigned nb = msg[e] <= 0.0f;
                    msg[e] = ((e == ix) ? m2 : m1) * ((par ^ nb) ? nalpha : alpha);
                }
            }
        } else {
            for (int r = tid; r < m; r += nt) {
                const int e0 = row_ptr[r], e1 = row_ptr[r + 1];
                float U = 0.0f;
                unsigned par = synd[r];
                for (int e = e0; e < e1; e++) {
                    const float x = msg[e];
                    scr[e] = U;
                    par ^= (unsigned)(x < 0.0f);
                    const float u = tanh_compl(fabsf(x));
                    U = compl_step(U, u);
                }
                U = 0.0f;
                for (int e = e1 - 1; e >= e0; e--) {
                    const float x = msg[e];
                    const float pk = scr[e];
                    const float Ut = compl_step(pk, U);
                    const float Lm = llr_from_compl(Ut);
                    msg[e] = ((par ^ (unsigned)(x < 0.0f)) & 1u) ? -Lm : Lm;
                    const float u = tanh_compl(fabsf(x));
                    U = compl_step(U, u);
                }
            }
        }
        __syncthreads();
        // ---- variable nodes ----
        const bool outs = early || last;
        for (int v = tid; v < n; v += nt) {
            const int c0 = col_ptr[v], c1 = col_ptr[v + 1];
            float temp = prior(v, pt, pc);
            for (int t = c0; t < c1; t++) {
                const int e = csc_edge[t];
                scr[e] = temp;
                temp += msg[e];
            }
            float suf = 0.0f;
            for (int t = c1 - 1; t >= c0; t--) {
                const int e = csc_edge[t];
                const float mk = msg[e];
                msg[e] = scr[e] + suf;
                suf += mk;
            }
            if (outs) {
                hard[v] = temp <= 0.0f;
                if (out_llr) out_llr[PLANES ? ((size_t)pt * n + v) * TW + pc : (size_t)b * n + v] = temp;
            }
        }
        if (tid == 0) flag = 0;
        __syncthreads();
        // ---- H e == s ? ----
        if (outs) {
            for (int r = tid; r < m; r += nt) {
                uint8_t p = synd[r];
                for (int e = row_ptr[r]; e < row_ptr[r + 1]; e++) p ^= hard[col_idx[e]];
                if (p) flag = 1;
            }
            __syncthreads();
            conv = !flag;
            if (conv && early) {
                it_done = it;
                break;
            }
        }
    }
    if (PLANES) {
        for (int v = tid; v < n; v += nt)
            if (hard[v]) atomicOr(hard_planes + (size_t)pt * n + v, 1ull << pc);
        if (tid == 0) {
            out_iters[b] = it_done;
            if (conv) atomicOr(conv_planes + pt, 1ull << pc);
        }
        return;
    }
    for (int v = tid; v < n; v += nt)
        out_bits[(size_t)b * n + v] = hard[v] ^ (kind == SCALDPC_IN_RECEIVED ? recv[v] : (uint8_t)0);
    if (tid == 0) {
        if (out_iters) out_iters[b] = it_done;
        if (out_conv) out_conv[b] = (uint8_t)conv;
    }
}
template <int METHOD, bool PLANES, class P>
__global__ __launch_bounds__(256) void k_bp_small(const int *__restrict__ row_ptr, const int *__restrict__ col_idx,
                                                  const int *__restrict__ col_ptr, const int *__restrict__ csc_edge,
                                                  typename P::Arg prior_arg, int m, int n, int E,
                                                  const void *__restrict__ in_, int kind, int max_iter, float alpha0,
                                                  int early, void *__restrict__ out_bits_,
                                                  float *__restrict__ out_llr, int *__restrict__ out_iters,
                                                  void *__restrict__ out_conv_)
{
    bp_small_body<METHOD, PLANES>(row_ptr, col_idx, col_ptr, csc_edge, P{prior_arg}, m, n, E, in_, kind, max_iter, alpha0, early,
                                  out_bits_, out_llr, out_iters, out_conv_);
}

// ---------------------------------------------------------------------------
// K4  variable-node update + posterior + hard decision, in place.
//   prefix : v2c_k = prior + sum_{k'<k} c2v_k'      (ascending row)
//   total  : L = prior + sum_k c2v_k ; e = [L <= 0]
//   suffix : v2c_k += sum_{k'>k} c2v_k'             (accumulated from the last edge)
// Column values live in registers (unrolled to MAXD, predicated on the uniform degree: for this
// gather kernel the lower register count of the bucketed form (70 VGPRs, 7 waves/SIMD) beats
// exact-degree straight-line code (131 VGPRs): 68.6 vs 74.9 us).
// Returns the posterior L.
// ---------------------------------------------------------------------------
// A wave's column record (VAR_REC ints, one scalar load): {column or -1, start of the column's
// edge list in the re-laid list, degree, unroll bound, first VAR_INLINE edge ids}.
constexpr int VAR_INLINE = 16, VAR_REC = 4 + VAR_INLINE;

// The column update with the edge ids fetched FIRST, all of them, as wide scalar loads (the record's
// inline ids, then the column's list), so that the gathers issue back to back: with one id fetched per
// edge the compiler puts an `s_load_dword` + `s_waitcnt lgkmcnt(0)` right in front of each
// gather (the branch on `k < d` keeps it from hoisting them), i.e. the gathers of a degree-11 column
// leave the wave a scalar-cache round trip apart (round 2: 65.0 -> 63.5 us, profiles/r02/ab_*.json).  The message row of edge e is addressed as
// (uniform base + e * 256) + lane * 4: the edge enters on the scalar side (SGPR base of the
// global_load), the lane offset is the one VGPR.  Same operations, same order: identical results.
template <int MAXD>
__device__ __forceinline__ float var_col_s(float *tile_base, unsigned lane, const int4 *__restrict__ rec4,
                                           const int *__restrict__ ce1, int d, float pr)
{
    int eid[MAXD];
    {
        const int4 a = rec4[1], b = rec4[2], c = rec4[3], e = rec4[4];  // uniform address: scalar loads
        const int in16[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, e.x, e.y, e.z, e.w};
#pragma unroll
        for (int k = 0; k < MAXD && k < VAR_INLINE; k++) eid[k] = in16[k];
#pragma unroll
        for (int k = VAR_INLINE; k < MAXD; k++) eid[k] = ce1[k];  // (the list is padded: reads past a column stay inside it)
    }
    float mm[MAXD], pp[MAXD];
#pragma unroll
    for (int k = 0; k < MAXD; k++)
        if (k < d) mm[k] = (tile_base + (size_t)rfl(eid[k]) * TW)[lane];
    float temp = pr;
#pragma unroll
    for (int k = 0; k < MAXD; k++)
        if (k < d) {
            pp[k] = temp;
            temp += mm[k];
        }
    float suf = 0.0f;
#pragma unroll
    for (int k = MAXD - 1; k >= 0; k--)
        if (k < d) {
            (tile_base + (size_t)rfl(eid[k]) * TW)[lane] = pp[k] + suf;
            suf += mm[k];
        }
    return temp;
}

// A wave-uniform pointer pinned to an SGPR pair: the access `sbase(p)[lane]` then takes the scalar-base form
// (global_load/store v, v_lane_offset, s[base]) instead of a 64-bit VGPR address the compiler re-derives per edge with
// a v_lshl_add_u64 -- one VALU instruction per access in a pass that is bound by VALU issue.
typedef __attribute__((address_space(1))) float gfloat;  // (a pointer that went through an asm is no longer known to be global)
__device__ __forceinline__ gfloat *sbase(const float *p)
{
    gfloat *g = (gfloat *)p;
    asm("" : "+s"(g));
    return g;
}

// ITERATION 1 without its check pass.  The first check-to-variable message of an edge depends on the codeword only
// through the SYNDROME BIT of the edge's row: its magnitude is a function of the row's priors, its sign the parity of
// the priors' signs XOR that bit.  So the host keeps, per edge, the message of a codeword with an all-zero syndrome
// (`first_tab`: computed once per prior set by the row-parallel check kernel, whose values are the tile kernels' own,
// bit for bit) next to the edge's row, and the first variable pass takes c2v = first ^ (syndrome bit << 31) from scalar
// loads instead of gathering 256-B message rows a check pass would have had to write first: one launch and
// 8 E bytes per codeword less, same sums in the same order, identical results.
//   ft: the column's slice of first_tab (laid out like the re-laid edge list), {message bits, row}
//   f, wv: lane j's table entry of the column's j-th edge and that edge's syndrome word (fetched by the kernel, for
//          BOTH columns a wave handles, before either is processed)
template <int MAXD>
__device__ __forceinline__ float var_col_first(float *tile_base, unsigned lane, const int4 *__restrict__ rec4,
                                               const int *__restrict__ ce1, int2 f, u64 wv, int d, float pr)
{
    int eid[MAXD];
    {
        const int4 a = rec4[1], b = rec4[2], c = rec4[3], e = rec4[4];
        const int in16[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, e.x, e.y, e.z, e.w};
#pragma unroll
        for (int k = 0; k < MAXD && k < VAR_INLINE; k++) eid[k] = in16[k];
#pragma unroll
        for (int k = VAR_INLINE; k < MAXD; k++) eid[k] = ce1[k];
    }
    float mm[MAXD], pp[MAXD];
    // Lane j fetches the table entry of the column's j-th edge and then that edge's syndrome word: TWO vector round
    // trips for the whole column, whatever its degree; edge k's pair then reaches every lane through v_readlane.
    // (Through scalar loads the compiler makes every edge its own dependent `s_load; s_waitcnt; s_load; s_waitcnt`
    // chain -- 22 round trips in a row for a degree-11 column -- or, with the loads hoisted out of the `k < d`
    // predicate, still one `s_load; s_waitcnt` per syndrome word for want of SGPRs.)
    const int wlo = (int)(unsigned)wv, whi = (int)(unsigned)(wv >> 32);
#pragma unroll
    for (int k = 0; k < MAXD; k++)
        if (k < d) {
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane(wlo, k), hi = (unsigned)__builtin_amdgcn_readlane(whi, k);
            const u64 w = ((u64)hi << 32) | lo;
            mm[k] = __uint_as_float((unsigned)__builtin_amdgcn_readlane(f.x, k) ^ (((unsigned)(w >> lane) & 1u) << 31));
        }
    float temp = pr;
#pragma unroll
    for (int k = 0; k < MAXD; k++)
        if (k < d) {
            pp[k] = temp;
            temp += mm[k];
        }
    float suf = 0.0f;
#pragma unroll
    for (int k = MAXD - 1; k >= 0; k--)
        if (k < d) {
            (tile_base + (size_t)rfl(eid[k]) * TW)[lane] = pp[k] + suf;
            suf += mm[k];
        }
    return temp;
}

// first_tab[pos] = {first message of edge list[pos] (zero-syndrome codeword), its row}: one thread per list position.
// The row of an edge = the last r with row_ptr[r] <= e (binary search).  grid ceil(E/256).
__global__ __launch_bounds__(256) void k_first_tab(const int *__restrict__ list, const float *__restrict__ first_msg,
                                                   const int *__restrict__ row_ptr, int m, long E, int2 *__restrict__ tab)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= E) return;
    const int e = list[p];
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (row_ptr[mid] <= e) lo = mid; else hi = mid - 1;
    }
    tab[p] = make_int2(__float_as_int(first_msg[e]), lo);
}

// Any-degree fallback: prefix parked in the scratch array, second sweep re-reads c2v
// just before overwriting it.
__device__ __forceinline__ float var_col_generic(float *mt, float *st, const int *__restrict__ ce, int d, float pr)
{
    float temp = pr;
    for (int k = 0; k < d; k++) {
        const size_t o = (size_t)ce[k] * TW;
        st[o] = temp;
        temp += mt[o];
    }
    float suf = 0.0f;
    for (int k = d - 1; k >= 0; k--) {
        const size_t o = (size_t)ce[k] * TW;
        const float mk = mt[o];
        mt[o] = st[o] + suf;
        suf += mk;
    }
    return temp;
}

// The WIDE launch of the min-sum record form (minsum_rec = 2: columns of 33 ... 64 edges, see var_col_rec_wide below).
// k_var<64, P> is the kernel that already holds a column of 64 edges in registers (mm[64], pp[64]: 136 VGPRs), so the
// record-form pass of such columns is a MODE of it, not an instantiation of k_var_rec: rec non-null = this launch runs
// over blocks [blk0, ..) of the column records -- the (32, 64] bucket -- and rebuilds the messages from the records, as
// k_var_rec does for the columns up to 32.  The narrower builds of k_var never look at it.
struct RecWide {
    const int *var_rows = nullptr, *csc_row = nullptr;  // k_var_rec's var_rows / csc_row
    const float *rec = nullptr;                         // the group's records; null = the message form (plain k_var)
    u64 *sgn = nullptr;
    int m = 0, blk0 = 0, xmap = 0;                      // rows; first block of the slice; blocks per tile under the XCD map (0 = none)
    int last = 0;                                       // k_var_rec's LAST
    Settle stl = Settle{};
};
template <class P>
__device__ __forceinline__ void var_rec_wide_wave(const int *__restrict__ list, const int *__restrict__ csc_edge, const P &prior,
                                                  float *msg, float *__restrict__ post, u64 *__restrict__ hard,
                                                  const u64 *__restrict__ done, int skip_done, int n, long E, int write_out,
                                                  const RecWide &rw);

// One fused launch over all column-degree buckets.  wave = (column, tile), lane = codeword.
// grid (column records / 4, G), block 256 = 4 columns of one bucket.
// write_out: also emit hard-decision planes (merged under the done mask) and, if
// `post` is non-null, the posterior of every not-yet-frozen codeword.
// CAP = largest unroll bound compiled in (see k_check_tanh).
template <int CAP, class P>
__global__ __launch_bounds__(256) void k_var(const int *__restrict__ list, const int *__restrict__ csc_edge,
                                             typename P::Arg prior_arg, float *msg, float *scratch,
                                             float *__restrict__ post, u64 *__restrict__ hard,
                                             const u64 *__restrict__ done, int skip_done, int n, long E,
                                             int write_out, RecWide rw = RecWide{})
{
    const P prior{prior_arg};
    if constexpr (CAP >= 64)
        if (rw.rec) {  // (wave-uniform: a kernel argument)
            var_rec_wide_wave(list, csc_edge, prior, msg, post, hard, done, skip_done, n, E, write_out, rw);
            return;
        }
    const int lane = threadIdx.x & 63;
    const int tl = blockIdx.y;
    // one record per WAVE of the launch (VAR_REC ints: descriptor + the first VAR_INLINE edge ids), at
    // an address that is plain arithmetic on the wave's index, fetched with scalar loads: the
    // wave's whole prologue (walking the bucket table, then a descriptor, then the edge list
    // cost a chain of dependent loads); `csc_edge` is the edge list laid out in launch order
    const int *rec = list + (size_t)rfl((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * VAR_REC;
    const u64 dn = done[tl];
    if (skip_done && dn == ~0ull) return;
    const int v = rec[0];
    if (v < 0) return;
    const int cb = rec[1];
    const int d = rec[2];
    float *mt = msg + (size_t)tl * E * TW + lane;
    const int *ce = csc_edge + cb;
    const float pr = prior(v, tl, lane);
    float L = pr;
    {
        float *tb = msg + (size_t)tl * E * TW;
        const unsigned ul = threadIdx.x & 63u;  // unsigned lane index: lets the gathers take the SGPR-base form
        const int4 *r4 = (const int4 *)rec;
        switch (rec[3]) {
            case 1: L = var_col_s<1>(tb, ul, r4, ce, d, pr); break;
            case 2: L = var_col_s<2>(tb, ul, r4, ce, d, pr); break;
            case 4: L = var_col_s<4>(tb, ul, r4, ce, d, pr); break;
            case 8: L = var_col_s<8>(tb, ul, r4, ce, d, pr); break;
            case 16: L = var_col_s<16>(tb, ul, r4, ce, d, pr); break;
            case 32:
                if constexpr (CAP >= 32) L = var_col_s<32>(tb, ul, r4, ce, d, pr);
                break;
            case 64:
                if constexpr (CAP >= 64) L = var_col_s<64>(tb, ul, r4, ce, d, pr);
                break;
            default: L = var_col_generic(mt, scratch + (size_t)tl * E * TW + lane, ce, d, pr);
        }
    }
    if (write_out) {
        const u64 hb = __ballot(L <= 0.0f);
        const size_t hi = (size_t)tl * n + v;
        if (lane == 0) hard[hi] = (hard[hi] & dn) | (hb & ~dn);
        if (post && !((dn >> lane) & 1)) post[hi * TW + lane] = L;
    }
}
// ITERATION 1 of the tile kernels (see var_col_first): every wave takes TWO column records of the launch order and
// fetches both columns' table entries, then both columns' syndrome words, before it processes either -- the pass is
// three dependent round trips around half a pass's bytes, so a second column in flight per wave is what shortens it
// (one column per wave: 46.9 us per 128-codeword launch on the HQC-128 graph).  Every column of the graph has a
// register-resident degree (the host checks: max column degree <= 64), records come in fours, hence in pairs.
// grid (ceil(nrec / 8), G), block 256 = 4 waves = 8 records.
template <int CAP>
__global__ __launch_bounds__(256) void k_var_first(const int *__restrict__ list, const int *__restrict__ csc_edge,
                                                   const float *__restrict__ prior, float *msg, float *__restrict__ post,
                                                   u64 *__restrict__ hard, const u64 *__restrict__ done, int skip_done, int n,
                                                   long E, int write_out, const int2 *__restrict__ first_tab,
                                                   const u64 *__restrict__ synd, int m, int nrec)
{
    const unsigned lane = threadIdx.x & 63u;
    const int tl = blockIdx.y;
    const int r0 = 2 * rfl((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (r0 >= nrec) return;
    const u64 dn = done[tl];
    if (skip_done && dn == ~0ull) return;
    float *tb = msg + (size_t)tl * E * TW;
    const u64 *st = synd + (size_t)tl * m;
    const int *rec[2] = {list + (size_t)r0 * VAR_REC, list + (size_t)(r0 + 1) * VAR_REC};
    int v[2], cb[2], d[2];
    int2 f[2];
    u64 wv[2];
    float pr[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        v[j] = rec[j][0];
        cb[j] = rec[j][1];
        d[j] = v[j] < 0 ? 0 : rec[j][2];
        f[j] = make_int2(0, 0);
        if ((int)lane < d[j]) f[j] = first_tab[(size_t)cb[j] + lane];
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        wv[j] = st[f[j].y];  // (lanes >= d read row 0: valid, unused)
        pr[j] = prior[v[j] < 0 ? 0 : v[j]];
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (v[j] < 0) continue;  // padding record
        const int4 *r4 = (const int4 *)rec[j];
        const int *ce = csc_edge + cb[j];
        float L = pr[j];
        switch (rec[j][3]) {
            case 1: L = var_col_first<1>(tb, lane, r4, ce, f[j], wv[j], d[j], pr[j]); break;
            case 2: L = var_col_first<2>(tb, lane, r4, ce, f[j], wv[j], d[j], pr[j]); break;
            case 4: L = var_col_first<4>(tb, lane, r4, ce, f[j], wv[j], d[j], pr[j]); break;
            case 8: L = var_col_first<8>(tb, lane, r4, ce, f[j], wv[j], d[j], pr[j]); break;
            case 16: L = var_col_first<16>(tb, lane, r4, ce, f[j], wv[j], d[j], pr[j]); break;
            case 32:
                if constexpr (CAP >= 32) L = var_col_first<32>(tb, lane, r4, ce, f[j], wv[j], d[j], pr[j]);
                break;
            case 64:
                if constexpr (CAP >= 64) L = var_col_first<64>(tb, lane, r4, ce, f[j], wv[j], d[j], pr[j]);
                break;
            default: break;  // (no any-degree columns when this kernel is launched)
        }
        if (write_out) {
            const u64 hb = __ballot(L <= 0.0f);
            const size_t hi = (size_t)tl * n + v[j];
            if (lane == 0) hard[hi] = (hard[hi] & dn) | (hb & ~dn);
            if (post && !((dn >> lane) & 1)) post[hi * TW + lane] = L;
        }
    }
}

// Variable pass of the min-sum RECORD form (see k_check_minsum_rec): the column's messages are rebuilt from the
// records of its edges' rows.  The wave's column record carries the first VAR_INLINE edge ids, a parallel table the
// row words of those edges (`var_rows`, VAR_INLINE ints per record: the row and, in the high bits, the edge's index IN
// that row -- scaldpc_rec_pack.h), both through scalar loads.  Per edge and lane the pass reads the row's arg-min byte
// (a 64-B row, row on the scalar side) and compares it with the edge's in-row index: that is "this edge is the
// codeword's arg-min", and it SELECTS THE ADDRESS of the one magnitude gather that follows -- the lane's word of the
// row's second-magnitude plane instead of the first (the planes lie m rows apart: one v_cndmask on the lane's byte
// offset).  One gather per edge and lane, no execute-mask juggling, no mask kept in SGPRs between a load and a select.
// All arg-min bytes of the column are in flight before the first is waited for, then all magnitudes.  (Fetching both
// magnitudes in one independent 8-byte gather, with the compare selecting a register, saves the second round trip and
// measured 5.7 % SLOWER per step: twice the record bytes between L2 and the CUs.  profiles/minsum_signed_records/.)
// The records carry their row's parity in the sign bit, so the sign of edge k is that bit XOR the column's own sign
// mask of the edge: lane j fetches the mask of the column's j-th edge (contiguous), edge k's word reaches a
// sign-flipping select through v_readlane.  No parity plane, no row word per lane, no per-column parity gather.
// The pass leaves the column's NEW sign masks behind: edge k's is the ballot of (stored float <= 0), taken from the
// very value that is stored, put into lane k of two registers with v_writelane (the compiler's own: writelane()), and
// lanes j < D store the words -- contiguous again.  They follow the messages for EVERY lane: the done bits freeze
// outputs, not messages.
// Like the record-form check pass this kernel is bound by VALU issue (SQ counters: profiles/r03/sq_counters_*record*),
// so it is straight-line code for the column's EXACT degree, dispatched wave-uniformly: the bucketed form (unrolled to
// the bucket's bound, predicated on `k < d`) spent more instructions on the predicates than on the column.
//   csc_row: row word of every position of the re-laid edge list (laid out like it); read for edges beyond VAR_INLINE
//   rec2_off: bytes from a row's first magnitudes to its second ones (m * 256: below 2^32, rec_rows_fit)
typedef __attribute__((address_space(1))) unsigned char gbyte;
__device__ __forceinline__ gbyte *sbase_b(const unsigned char *p)
{
    gbyte *g = (gbyte *)p;
    asm("" : "+s"(g));
    return g;
}

// LAST: the pass after which no check pass follows (the last iteration of a decode).  Nothing reads the messages or the
// sign masks it would leave -- the next call starts over at iteration 1 -- so it only sums: the same gathers and sign
// flips, then prior + mm[0] + mm[1] + ... in the same order, which is the posterior.  No stores, no prefix array, no
// suffix sums, no ballots, no edge ids.
// (Forming the store addresses from the row words -- edge id = row * the rows' common degree + index in the row -- and
// leaving the record's 64 B of inline ids unread was built and measured: 4.5 MB less fetched per launch and 5-7 % MORE
// time per step, the scalar arithmetic in front of every store being issue slots this pass does not have.
// profiles/minsum_trim/README.md.)
template <int D, bool LAST>
__device__ __forceinline__ float var_col_rec(float *tile_base, const float *__restrict__ rec_base, unsigned rec2_off,
                                             const unsigned char *__restrict__ arg_base, u64 *sgn_col, unsigned lane,
                                             const int *__restrict__ rc, const int4 *__restrict__ row4,
                                             const int *__restrict__ ce1, const int *__restrict__ cr1, float pr,
                                             unsigned *mark_word = nullptr, unsigned mark = 0, u64 real = 0,
                                             unsigned *col_flag = nullptr)
{
    int eid[D], rw[D];
    {
        const int4 ra = row4[0], rb = row4[1], rc4 = row4[2], re = row4[3];
        const int rw16[16] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w, rc4.x, rc4.y, rc4.z, rc4.w, re.x, re.y, re.z, re.w};
#pragma unroll
        for (int k = 0; k < D && k < VAR_INLINE; k++) rw[k] = rw16[k];
#pragma unroll
        for (int k = VAR_INLINE; k < D; k++) rw[k] = cr1[k];
        // (the edge ids are wanted by the stores alone: fetched below)
    }
    // lane j: the sign mask of the column's j-th edge (sgn_col = the mask of the column's first position: a column's
    // masks are contiguous); the row's parity comes with the record
    u64 sg = 0;
    if ((int)lane < D) sg = sgn_col[lane];
    const int slo = (int)(unsigned)sg, shi = (int)(unsigned)(sg >> 32);
    float mm[D], pp[D];
    unsigned ab[D];
#pragma unroll
    for (int k = 0; k < D; k++) ab[k] = sbase_b(arg_base + (size_t)rec_row_of(rfl(rw[k])) * TW)[lane];
    const unsigned off1 = lane * 4u, off2 = off1 + rec2_off;
#pragma unroll
    for (int k = 0; k < D; k++) {
        const unsigned off = ab[k] == (unsigned)rec_index_of(rfl(rw[k])) ? off2 : off1;
        mm[k] = *(const gfloat *)((const gbyte *)sbase(rec_base + (size_t)rec_row_of(rfl(rw[k])) * TW) + off);
    }
#pragma unroll
    for (int k = 0; k < D; k++) {
        const u64 ng = ((u64)(unsigned)__builtin_amdgcn_readlane(shi, k) << 32) | (unsigned)__builtin_amdgcn_readlane(slo, k);
        mm[k] = __builtin_amdgcn_inverse_ballot_w64(ng) ? -mm[k] : mm[k];
    }
    if constexpr (LAST) {
        float sum = pr;
#pragma unroll
        for (int k = 0; k < D; k++) sum += mm[k];
        return sum;
    }
    // the record's inline edge ids (wanted by the stores alone)
    {
        const int4 *rec4 = (const int4 *)rc;
        const int4 a = rec4[1], b = rec4[2], c = rec4[3], e = rec4[4];
        const int in16[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, e.x, e.y, e.z, e.w};
#pragma unroll
        for (int k = 0; k < D && k < VAR_INLINE; k++) eid[k] = in16[k];
    }
    float temp = pr;
#pragma unroll
    for (int k = 0; k < D; k++) {
        pp[k] = temp;
        temp += mm[k];
    }
    // (those beyond the record's inline ones come from the edge list)
#pragma unroll
    for (int k = VAR_INLINE; k < D; k++) eid[k] = ce1[k];
    float suf = 0.0f;
    unsigned nlo = 0, nhi = 0;  // lane k keeps edge k's new sign mask
#pragma unroll
    for (int k = D - 1; k >= 0; k--) {
        gfloat *q = sbase(tile_base + (size_t)rfl(eid[k]) * TW) + lane;
        const float out = pp[k] + suf;
        // sc1: the line does not stay in this XCD's L2 (it is read next by a check pass on whichever XCD), which keeps
        // the L2 for the records: 76.2 -> 74.3 ms per step on the HQC-128 bench (profiles/r03/ab_rec_l2.log)
        __hip_atomic_store(q, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const u64 nm = __ballot(out <= 0.0f);  // a float compare on the stored value: +-0 is "negative", NaN is not
        nlo = writelane((unsigned)nm, k, nlo);
        nhi = writelane((unsigned)(nm >> 32), k, nhi);
        suf += mm[k];
    }
    if ((int)lane < D) sgn_col[lane] = ((u64)nhi << 32) | nlo;
    // settled codewords (Settle): lane j holds the mask of edge j it read and the one it stores; mark_word non-null
    // (wave-uniform) = this pass is tracked, and a difference in a real codeword's bit marks the tile
    if (mark_word) {
        const unsigned dlo = (nlo ^ (unsigned)slo) & (unsigned)real, dhi = (nhi ^ (unsigned)shi) & (unsigned)(real >> 32);
        const bool sc = __ballot((int)lane < D && (dlo | dhi) != 0) != 0;
        if (sc && lane == 0) *mark_word = mark;
        // the sparse gate's column flag (Settle): this is variable pass mark - 1, and it ran
        if (col_flag && lane == 0) *col_flag = ((mark - 1u) << 1) | (sc ? 1u : 0u);
    }
    return temp;
}

// The WIDE column: var_col_rec for a column of d = 33 ... 64 edges (minsum_rec = 2; a few dozen columns in tens of
// thousands on the attack's graphs, so this is sized for registers and code size, not for issue slots).  Same inputs, same
// outputs, the same operations on every value in the same order -- prefix from the prior ascending, suffix descending,
// stored message pp[k] + suf, posterior prior + mm[0] + mm[1] + ...; sign masks in and out in lane k as there.  ONE body
// for all 32 degrees: edges 0 ... 31 are there for every such column, the ones behind them are predicated on the
// wave-uniform `k < d`.  Only mm[64] and pp[64] live across the column; row words, arg-min bytes and edge ids are taken
// 16 at a time (scalar loads: the record's inline words for the first 16, csc_row / csc_edge for the others -- the lists
// are padded, a 16-word read that starts inside a column stays inside them), first for the gathers and again, from the
// last chunk down, for the stores.  LAST keeps no array at all: it sums each chunk as it arrives.
template <bool LAST>
__device__ __forceinline__ float var_col_rec_wide(float *tile_base, const float *__restrict__ rec_base, unsigned rec2_off,
                                                  const unsigned char *__restrict__ arg_base, u64 *sgn_col, unsigned lane,
                                                  const int *__restrict__ rc, const int4 *__restrict__ row4,
                                                  const int *__restrict__ ce1, const int *__restrict__ cr1, int d, float pr,
                                                  unsigned *mark_word = nullptr, unsigned mark = 0, u64 real = 0)
{
    constexpr int W = 64, CH = 16, SURE = 32;  // SURE: edges every column that comes here has
    u64 sg = 0;
    if ((int)lane < d) sg = sgn_col[lane];
    const int slo = (int)(unsigned)sg, shi = (int)(unsigned)(sg >> 32);
    const unsigned off1 = lane * 4u, off2 = off1 + rec2_off;
    float mm[W];
    float sum = pr;
#pragma unroll
    for (int c = 0; c < W / CH; c++) {
        if (c * CH >= SURE && c * CH >= d) break;
        int rw[CH];
        if (c == 0) {
            const int4 ra = row4[0], rb = row4[1], rc4 = row4[2], re = row4[3];
            const int rw16[16] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w, rc4.x, rc4.y, rc4.z, rc4.w, re.x, re.y, re.z, re.w};
#pragma unroll
            for (int k = 0; k < CH; k++) rw[k] = rw16[k];
        } else {
#pragma unroll
            for (int k = 0; k < CH; k++) rw[k] = cr1[c * CH + k];
        }
        unsigned ab[CH];
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (c * CH + k < SURE || c * CH + k < d) ab[k] = sbase_b(arg_base + (size_t)rec_row_of(rfl(rw[k])) * TW)[lane];
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (c * CH + k < SURE || c * CH + k < d) {
                const unsigned off = ab[k] == (unsigned)rec_index_of(rfl(rw[k])) ? off2 : off1;
                mm[c * CH + k] = *(const gfloat *)((const gbyte *)sbase(rec_base + (size_t)rec_row_of(rfl(rw[k])) * TW) + off);
            }
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (c * CH + k < SURE || c * CH + k < d) {
                const int e = c * CH + k;
                const u64 ng = ((u64)(unsigned)__builtin_amdgcn_readlane(shi, e) << 32) | (unsigned)__builtin_amdgcn_readlane(slo, e);
                mm[e] = __builtin_amdgcn_inverse_ballot_w64(ng) ? -mm[e] : mm[e];
                if constexpr (LAST) sum += mm[e];
            }
    }
    if constexpr (LAST) return sum;
    float pp[W];
    float temp = pr;
#pragma unroll
    for (int k = 0; k < W; k++)
        if (k < SURE || k < d) {
            pp[k] = temp;
            temp += mm[k];
        }
    float suf = 0.0f;
    unsigned nlo = 0, nhi = 0;  // lane k keeps edge k's new sign mask
#pragma unroll
    for (int c = W / CH - 1; c >= 0; c--) {
        if (c * CH >= SURE && c * CH >= d) continue;
        int eid[CH];
        if (c == 0) {
            const int4 *rec4 = (const int4 *)rc;
            const int4 a = rec4[1], b = rec4[2], c4 = rec4[3], e4 = rec4[4];
            const int in16[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c4.x, c4.y, c4.z, c4.w, e4.x, e4.y, e4.z, e4.w};
#pragma unroll
            for (int k = 0; k < CH; k++) eid[k] = in16[k];
        } else {
#pragma unroll
            for (int k = 0; k < CH; k++) eid[k] = ce1[c * CH + k];
        }
#pragma unroll
        for (int k = CH - 1; k >= 0; k--)
            if (c * CH + k < SURE || c * CH + k < d) {
                const int e = c * CH + k;
                gfloat *q = sbase(tile_base + (size_t)rfl(eid[k]) * TW) + lane;
                const float out = pp[e] + suf;
                __hip_atomic_store(q, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (sc1, as in var_col_rec)
                const u64 nm = __ballot(out <= 0.0f);  // a float compare on the stored value: +-0 is "negative", NaN is not
                nlo = writelane((unsigned)nm, e, nlo);
                nhi = writelane((unsigned)(nm >> 32), e, nhi);
                suf += mm[e];
            }
    }
    if ((int)lane < d) sgn_col[lane] = ((u64)nhi << 32) | nlo;
    // settled codewords (Settle), as in var_col_rec
    if (mark_word) {
        const unsigned dlo = (nlo ^ (unsigned)slo) & (unsigned)real, dhi = (nhi ^ (unsigned)shi) & (unsigned)(real >> 32);
        if (__ballot((int)lane < d && (dlo | dhi) != 0) != 0 && lane == 0) *mark_word = mark;
    }
    return temp;
}

// A wave of the WIDE record-form launch (RecWide, k_var<64, P>): k_var_rec's wave -- slice of the records, XCD map, settled
// tiles, output -- around var_col_rec_wide, with LAST a run-time value (wave-uniform: both bodies are compiled in).
template <class P>
__device__ __forceinline__ void var_rec_wide_wave(const int *__restrict__ list, const int *__restrict__ csc_edge, const P &prior,
                                                  float *msg, float *__restrict__ post, u64 *__restrict__ hard,
                                                  const u64 *__restrict__ done, int skip_done, int n, long E, int write_out,
                                                  const RecWide &rw)
{
    const unsigned lane = threadIdx.x & 63u;
    int tl = blockIdx.y, bx = blockIdx.x;
    if (rw.xmap) {  // (as in k_var_rec)
        const unsigned G = gridDim.y, L = blockIdx.y * gridDim.x + blockIdx.x, xcd = L & 7u, slot = L >> 3;
        tl = (int)(xcd % G);
        bx = (int)(slot * (8u / G) + xcd / G);
        if (bx >= rw.xmap) return;
    }
    const int ri = rfl((bx + rw.blk0) * 4 + (int)(threadIdx.x >> 6));
    const int *rc = list + (size_t)ri * VAR_REC;
    const u64 dn = done[tl];
    if (skip_done && dn == ~0ull) return;
    const bool last = rw.last != 0;
    unsigned *mark_word = nullptr;
    bool decided = false;
    if (rw.stl.words) {  // settled codewords, as in k_var_rec
        unsigned *w = rw.stl.words + (size_t)tl * SETTLE_WORDS;
        const bool frozen = settle_frozen(w, rw.stl.done);
        if (last)
            decided = frozen;
        else {
            if (frozen) return;
            if (rw.stl.mark) mark_word = w + ((unsigned)bx & (SETTLE_SHARDS - 1));
        }
    }
    const int v = rc[0];
    if (v < 0) return;
    const int cb = rc[1];
    const int d = rc[2];
    if (d <= 32 || d > 64) return;  // (never: the slice is the (32, 64] bucket)
    if (last && decided) return;
    float *tb = msg + (size_t)tl * E * TW;
    const float *rb = rw.rec + (size_t)tl * rec_tile_floats(rw.m);
    const unsigned char *ab = (const unsigned char *)(rb + rec_arg_off(rw.m));
    u64 *st = rw.sgn + (size_t)tl * E;
    const int *ce = csc_edge + cb, *cr = rw.csc_row + cb;
    const int4 *w4 = (const int4 *)(rw.var_rows + (size_t)ri * VAR_INLINE);
    const float pr = prior(v, tl, (int)lane);
    const unsigned r2 = (unsigned)rw.m * (TW * (unsigned)sizeof(float));
    // the sparse gate (Settle): a wide column is never gated and always stamps, so that its rows run in the next check pass;
    // its "sign masks changed" bit, which only a column's own gate reads, stays 0
    if (mark_word && rw.stl.colf && lane == 0) rw.stl.colf[(size_t)tl * rw.stl.ncol + v] = ((unsigned)rw.stl.mark - 1u) << 1;
    const float L = last ? var_col_rec_wide<true>(tb, rb, r2, ab, st + cb, lane, rc, w4, ce, cr, d, pr)
                         : var_col_rec_wide<false>(tb, rb, r2, ab, st + cb, lane, rc, w4, ce, cr, d, pr, mark_word,
                                                   (unsigned)rw.stl.mark, ~dn);
    if (write_out) {
        const u64 hb = __ballot(L <= 0.0f);
        const size_t hi = (size_t)tl * n + v;
        if (dn == 0) {
            if (lane == 0) hard[hi] = hb;
        } else if (lane == 0)
            hard[hi] = (hard[hi] & dn) | (hb & ~dn);
        if (post && !((dn >> lane) & 1)) post[hi * TW + lane] = L;
    }
}

// grid (column records / 4, G), block 256 = 4 column records (k_var's launch shape and records).
// (P = SoftPrior: tl is the tile the XCD map chose, the plane row follows it like the records do)
// LAST: the store-free form of a decode's last pass (var_col_rec); it always comes with write_out.
template <int CAP, class P, bool LAST = false>
__global__ __launch_bounds__(256) void k_var_rec(const int *__restrict__ list, const int *__restrict__ var_rows,
                                                 const int *__restrict__ csc_edge, const int *__restrict__ csc_row,
                                                 typename P::Arg prior_arg, float *msg, const float *__restrict__ rec,
                                                 u64 *sgn, float *__restrict__ post,
                                                 u64 *__restrict__ hard, const u64 *__restrict__ done, int skip_done, int n, int m,
                                                 long E, int write_out, int blk0, int xmap, Settle stl = Settle{})
{
    const P prior{prior_arg};
    const unsigned lane = threadIdx.x & 63u;
    int tl = blockIdx.y, bx = blockIdx.x;
    if (xmap) {
        // xmap = blocks per tile of this launch (G = 2, 4 or 8 tiles, grid.x a multiple of 8): workgroups are dealt
        // round-robin over the 8 XCDs by linear index, so tile = (linear index % 8) % G gives every XCD's L2 the record
        // planes of ONE of the launch's tiles instead of all of them.  Placement is a speed matter only.
        const unsigned G = gridDim.y, L = blockIdx.y * gridDim.x + blockIdx.x, xcd = L & 7u, slot = L >> 3;
        tl = (int)(xcd % G);
        bx = (int)(slot * (8u / G) + xcd / G);
        if (bx >= xmap) return;
    }
    const int ri = rfl((bx + blk0) * 4 + (int)(threadIdx.x >> 6));  // blk0: first block of the launch's slice of the records
    const int *rc = list + (size_t)ri * VAR_REC;
    const u64 dn = done[tl];
    if (skip_done && dn == ~0ull) return;
    // settled codewords (Settle).  A pass that is not the last returns for a frozen tile: it would store what is there.
    // The LAST pass is handed the words only where every earlier record-form variable pass of the tile has left its
    // columns' decisions in `hard` (launch_var, keep_hard; stl.done = the group's last test): the last of them that ran on
    // a tile frozen at t, pass t - 1, summed the very records and sign masks this pass would gather, in the same order,
    // so its decisions ARE this pass's.  Those passes leave out the columns of degree <= 1 (launch_var, slim), so on a
    // frozen tile this pass still decides those, and returns for every other column.
    unsigned *mark_word = nullptr;
    bool decided = false;
    if (stl.words) {
        unsigned *w = stl.words + (size_t)tl * SETTLE_WORDS;
        const bool frozen = settle_frozen(w, stl.done);
        if constexpr (LAST)
            decided = frozen;
        else {
            if (frozen) return;
            if (stl.mark) mark_word = w + ((unsigned)bx & (SETTLE_SHARDS - 1));
        }
    }
    const int v = rc[0];
    if (v < 0) return;
    const int cb = rc[1];
    const int d = rc[2];
    if (LAST && decided && d > 1) return;
    const int *ce = csc_edge + cb, *cr = csc_row + cb;
    unsigned *cf = nullptr;
    if constexpr (!LAST)
        if (mark_word && stl.colf && d > 1) {
            // the sparse gate (Settle): lane j looks at the flag of the row of the column's j-th edge; no edge marked by
            // this iteration's check pass and no sign mask of its own changed in its last run = the column's inputs are what
            // they were, and it would store what is there (its decisions in `hard` included)
            cf = stl.colf + (size_t)tl * n + v;
            if (stl.gate) {
                const unsigned t = (unsigned)stl.mark - 1u;
                bool hit = false;
                if ((int)lane < d) {
                    const int w = cr[lane];
                    const uint4 f = stl.rowf[(size_t)tl * m + rec_row_of(w)];
                    const unsigned ix = (unsigned)rec_index_of(w);
                    hit = f.x == t && (((ix < 32u ? f.z : f.w) >> (ix & 31u)) & 1u) != 0;
                }
                const unsigned own = *cf;
                if (__ballot(hit) == 0 && own != (((t - 1u) << 1) | 1u)) return;
            }
        }
    float *tb = msg + (size_t)tl * E * TW;
    const float *rb = rec + (size_t)tl * rec_tile_floats(m);  // the tile's block: [m1 | m2][row][64], arg
    const unsigned char *ab = (const unsigned char *)(rb + rec_arg_off(m));
    u64 *st = sgn + (size_t)tl * E;
    const int4 *w4 = (const int4 *)(var_rows + (size_t)ri * VAR_INLINE);
    const float pr = prior(v, tl, (int)lane);
    float L = pr;
    const unsigned r2 = (unsigned)m * (TW * (unsigned)sizeof(float));  // rec_m2_off(m) in bytes
#define VR(D)                                                                                                \
    case D:                                                                                                  \
        if constexpr (D <= CAP)                                                                              \
            L = var_col_rec<D, LAST>(tb, rb, r2, ab, st + cb, lane, rc, w4, ce, cr, pr, mark_word, (unsigned)stl.mark, ~dn, cf); \
        break;
#define VR8(D) VR(D) VR(D + 1) VR(D + 2) VR(D + 3) VR(D + 4) VR(D + 5) VR(D + 6) VR(D + 7)
    switch (d) {
        VR(1) VR(2) VR(3) VR(4) VR(5) VR(6) VR(7)
        VR8(8) VR8(16) VR8(24) VR(32)
        default: break;  // (degree 0: the posterior is the prior; degrees beyond 32 never reach this kernel: rec_form())
    }
#undef VR8
#undef VR
    if (write_out) {
        const u64 hb = __ballot(L <= 0.0f);
        const size_t hi = (size_t)tl * n + v;
        // (dn == 0, wave-uniform: nothing to keep, so no load in front of the store -- the passes that leave their decisions
        // for the closing pass pay for a store alone on a full tile of a fixed-iteration call)
        if (dn == 0) {
            if (lane == 0) hard[hi] = hb;
        } else if (lane == 0)
            hard[hi] = (hard[hi] & dn) | (hb & ~dn);
        if (post && !((dn >> lane) & 1)) post[hi * TW + lane] = L;
    }
}
// ---------------------------------------------------------------------------
// Row-parallel ("edge-lane") kernels for a HANDFUL of codewords on a graph too large for
// LDS: the single `decode()` of the attack loop (hqc.py:708 -- one codeword, n ~ 20 000,
// up to 100 iterations) and the few stragglers the compact pass re-decodes.  A 64-codeword
// tile would stream 64 lanes of messages to use one; here the layout is per codeword
//     emsg : float [codeword][edge]          (CSR order: a row's messages are contiguous)
// and a wave owns one (row, codeword): LANE = EDGE of the row.  The row's messages are
// one coalesced load, reductions over the row are wave primitives (ballot / popcount for
// the sign parity, xor-shuffle butterflies for the two minima), the tanh rule's exclusive
// forward/backward products walk the row with v_readlane broadcasts IN THE REFERENCE'S
// ORDER, so every value is bit-identical to the tile kernels'.  State (syndrome, hard
// decisions, done / unsat masks, posterior) stays in the tile formats: the codewords are
// bits 0..nb-1 of one tile, so k_parity / k_finalize and all I/O kernels are shared.
// Rows of degree <= 64 only (the host falls back to the tile path otherwise).
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_min_f(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float readlane_f(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// (No message initialisation pass: these kernels serve rows of at most ROW_CAP edges -- the host's el_ok -- and for such
// rows the first check pass of either rule reads the priors, fused_init.)
// METHOD as in the C ABI; FIRST: inputs are the priors (iteration 1).
// grid (ceil(m/4), nb), block 256 = 4 rows of codeword blockIdx.y.
template <int METHOD, bool FIRST, class P>
__global__ __launch_bounds__(256) void k_el_check(const int *__restrict__ row_ptr, const int *__restrict__ col_idx,
                                                  typename P::Arg prior_arg, float *emsg,
                                                  const u64 *__restrict__ synd, const u64 *__restrict__ done,
                                                  int skip_done, int m, long E, float alpha,
                                                  const u64 *__restrict__ hard, int *__restrict__ unsat_prev)
{
    const P prior{prior_arg};
    const int lane = threadIdx.x & 63;
    int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= m) return;
    r = rfl(r);
    const int c = blockIdx.y;
    if (skip_done && ((done[0] >> c) & 1)) return;  // frozen codeword
    const int e0 = rfl(row_ptr[r]);
    const int deg = rfl(row_ptr[r + 1]) - e0;
    const bool act = lane < deg;
    const unsigned sbit = (unsigned)(synd[r] >> c) & 1u;
    // Early-exit runs: the H e == s test of the PREVIOUS iteration's decisions rides on this
    // pass (the wave has the row anyway), k_el_var latches the verdict: two launches per
    // iteration instead of four.  A flag per codeword, set by any unsatisfied row.
    if (unsat_prev) {
        const unsigned hb = act ? (unsigned)(hard[col_idx[e0 + lane]] >> c) & 1u : 0u;
        if ((((unsigned)__popcll(__ballot(hb != 0u)) & 1u) ^ sbit) && lane == 0) unsat_prev[c] = 1;
    }
    if (deg == 0) return;
    float *p = emsg + (size_t)c * E + e0 + lane;
    float x = 0.0f;
    if (act) x = FIRST ? prior(col_idx[e0 + lane], 0, c) : *p;
    if (METHOD == SCALDPC_BP_MIN_SUM) {
        // the sequential form starts its running minima at FLT_MAX: |x| = inf never wins
        const float a = act ? fminf(fabsf(x), FLT_MAX) : FLT_MAX;
        const bool ng = act && x <= 0.0f;
        const unsigned par = sbit ^ ((unsigned)__popcll(__ballot(ng)) & 1u);
        const float m1 = wave_min_f(a);
        const int ix = __ffsll((long long)__ballot(act && a == m1)) - 1;  // first arg-min
        const float m2 = wave_min_f(lane == ix ? FLT_MAX : a);
        if (act) *p = ((lane == ix) ? m2 : m1) * ((par ^ (unsigned)ng) ? -alpha : alpha);
    } else {
        const unsigned xb = act ? __float_as_uint(x) : 0u;
        const float u = act ? tanh_compl(fabsf(x)) : 0.0f;
        const unsigned par = sbit ^ ((unsigned)__popcll(__ballot((xb >> 31) != 0u)) & 1u);
        float pre = 0.0f, suf = 0.0f;  // exclusive forward / backward complements of this lane's edge
#pragma unroll 4
        for (int t = 0; t < deg; t++) {
            const float nv = compl_step(pre, readlane_f(u, t));
            pre = (t < lane) ? nv : pre;
        }
#pragma unroll 4
        for (int t = deg - 1; t >= 0; t--) {
            const float nv = compl_step(suf, readlane_f(u, t));
            suf = (t > lane) ? nv : suf;
        }
        const float Lm = llr_from_compl(compl_step(pre, suf));
        const unsigned sg = ((par << 31) ^ xb) & 0x80000000u;  // parity of the OTHER inputs
        if (act) *p = __uint_as_float(__float_as_uint(Lm) ^ sg);
    }
}
// Variable nodes, lane = EDGE OF A COLUMN.  The host packs whole columns into waves of 64 lane
// slots: a column owns a SEGMENT of `cap` neighbouring lanes, cap >= max(degree, 1), of which the
// first `degree` hold its edges in ascending row order.  A slot is
//   {edge id or -1,  start | pos << 6 | (cap - 1) << 12 | live << 18}
// (start = first lane of the segment, pos = this lane's position in it, live = the segment holds a
// column); `slot_col` names the column at a segment's first lane.  A column's degree is not stored:
// it is the number of lanes of its segment that hold an edge, so appending a row to the graph
// (scaldpc_bp_append_rows) writes ONE slot word per new edge as long as the segment has a free lane.
// A fresh decoder packs columns in degree order with cap = max(degree, 1) -- no lane wasted; one
// that grows leaves a few free lanes per column and moves a column that outgrows its segment.
// All of a wave's messages arrive with ONE gather (a thread walking its column alone pays a
// dependent cross-XCD load per edge: 25 us per pass), then the exclusive prefix / suffix sums
// run over the segment with per-lane shuffles in the reference's sequential order:
//   pre_k = ((prior + m_0) + ... + m_{k-1}),  suf_k = ((0 + m_{d-1}) + ... + m_{k+1}),  out_k = pre_k + suf_k
// exactly the values var_col produces.  The segment's first lane owns the column (prior in,
// posterior and hard decision out); the codewords of one tile word are set / cleared with
// atomics (each launch row owns one bit).
// grid (waves padded to a multiple of 8 over 4, nb), block 256 = 4 packed waves.
template <class P>
__device__ __forceinline__ void el_var_body(const int2 *__restrict__ slots, const int *__restrict__ slot_col,
                                            int nwaves, P prior, float *emsg,
                                            float *__restrict__ post, u64 *__restrict__ hard,
                                            u64 *done, int skip_done, long E, int write_out,
                                            const int *__restrict__ unsat_prev, int it_prev, u64 *conv,
                                            int *__restrict__ iters, int *__restrict__ remaining_prev)
{
    const int lane = threadIdx.x & 63;
    int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nwaves) return;
    w = rfl(w);
    const int c = blockIdx.y;
    const bool frozen = (done[0] >> c) & 1;
    if (skip_done && frozen) return;  // frozen codeword
    if (unsat_prev) {
        // verdict of k_el_check's fused test: no unsatisfied row => the codeword converged at
        // iteration it_prev; its outputs (written by the previous launch of this kernel) stay,
        // the first wave of its launch row records the fact.  Every wave of the row takes the
        // same branch: the flags are read-only here and `done` only gains this very bit.
        const bool newly = !frozen && unsat_prev[c] == 0;
        if (newly) {
            if (w == 0 && lane == 0) {
                atomicOr(done, 1ull << c);
                atomicOr(conv, 1ull << c);
                iters[c] = it_prev;
            }
            return;
        }
        if (w == 0 && lane == 0 && !frozen) atomicAdd(remaining_prev, 1);
    }
    const int2 sl = slots[(size_t)w * 64 + lane];
    const int e = sl.x, start = sl.y & 63, pos = (sl.y >> 6) & 63, cap = ((sl.y >> 12) & 63) + 1;
    const bool live = (sl.y >> 18) & 1;
    const bool head = live && pos == 0;  // first lane of a column's segment
    // degree = lanes of the segment that hold an edge; the wave's loop bound = its largest degree
    const u64 has = __ballot(e >= 0);
    const u64 segmask = (cap == 64 ? ~0ull : ((1ull << cap) - 1ull)) << start;
    const int deg = live ? __popcll(has & segmask) : 0;
    int dmax = deg;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) dmax = max(dmax, __shfl_xor(dmax, off));
    dmax = rfl(dmax);
    float *mt = emsg + (size_t)c * E;
    const float mk = e >= 0 ? mt[e] : 0.0f;
    int v = 0;
    float pr = 0.0f;
    if (head) {
        v = slot_col[(size_t)w * 64 + lane];
        pr = prior(v, 0, c);
    }
    pr = __shfl(pr, start);
    float pre = pr, tot = pr, suf = 0.0f;
    for (int t = 0; t < dmax; t++) {
        const float val = __shfl(mk, (start + t) & 63);
        pre = (t < pos) ? pre + val : pre;
        tot = (t < deg) ? tot + val : tot;
    }
    for (int t = dmax - 1; t >= 0; t--) {
        const float val = __shfl(mk, (start + t) & 63);
        suf = (t > pos && t < deg) ? suf + val : suf;
    }
    if (e >= 0) mt[e] = pre + suf;
    if (write_out && head) {
        if (tot <= 0.0f)
            atomicOr(hard + v, 1ull << c);
        else
            atomicAnd(hard + v, ~(1ull << c));
        if (post) post[(size_t)v * TW + c] = tot;
    }
}
template <class P>
__global__ __launch_bounds__(256) void k_el_var(const int2 *__restrict__ slots, const int *__restrict__ slot_col,
                                                int nwaves, typename P::Arg prior_arg, float *emsg,
                                                float *__restrict__ post, u64 *__restrict__ hard,
                                                u64 *done, int skip_done, long E, int write_out,
                                                const int *__restrict__ unsat_prev, int it_prev, u64 *conv,
                                                int *__restrict__ iters, int *__restrict__ remaining_prev)
{
    el_var_body(slots, slot_col, nwaves, P{prior_arg}, emsg, post, hard, done, skip_done, E, write_out, unsat_prev, it_prev, conv,
                iters, remaining_prev);
}
// dst[idx] = val for a list of {idx, val} pairs (table updates of scaldpc_bp_append_rows).  grid ceil(n/256).
__global__ __launch_bounds__(256) void k_apply_pairs(int *__restrict__ dst, const int2 *__restrict__ pairs, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[pairs[i].x] = pairs[i].y;
}

// ---------------------------------------------------------------------------
// K6  Monte-Carlo helpers: per-trial noise sampling, syndrome and success compare on the
// device (the reference does these per position in Python: simulate/decode.py:36-40,
// 166-168, 173-175; simulate/hqc.py:684-705, 742-749).
// Random numbers: Philox4x32-10 (Salmon et al., SC'11), counter-based, keyed by the seed;
// counter = (block, stream, trial_lo, trial_hi) with the GLOBAL trial index, so a trial's
// inputs do not depend on batch size, tile position or the number of GPUs.
//   stream 0 word x : Bernoulli(p_x) for position x      (flip iff word < floor(p_x * 2^32));
//                     scaldpc_mc_hqc_run_soft: the outcome of check x (k_mc_hqc_outcome) -- the same word
//   stream 1 word j : j-th candidate position of the HQC secret, pos = mulhi(word, N),
//                     accepted if not chosen before, until omega are accepted
// ---------------------------------------------------------------------------
// (U4, philox4x32_10: scaldpc_philox.h, shared with the q-ary trial generator)
// The three generators below are written once, over the source of the trial index (scaldpc_mc_draw.h): these kernels are the
// contiguous form, slot b = trial first + b; the list form of the _at entries (slot b = trial ids[b]) is scaldpc_bp_mc_at.hip's.

// planes[t][x] (bit c) = [stream-`stream` word x of trial first + 64 t + c  <  thr_x]; XOR_INTO flips
// an existing plane instead.  wave = (tile, 16 consecutive x).  grid (ceil(len/64), T), block 256.
template <bool XOR_INTO>
__global__ __launch_bounds__(256) void k_mc_bernoulli(u64 *__restrict__ planes, int len, int batch, long first,
                                                      unsigned stream, unsigned k0, unsigned k1,
                                                      const u64 *__restrict__ thr, u64 thr0)
{
    mc_bernoulli_body<XOR_INTO>(planes, len, batch, TrialRange{first}, stream, k0, k1, thr, thr0);
}

// HQC secret: omega distinct positions per trial, set as bits of planes[t][pos] (pos < N; the
// plane rows have stride n).  One wave per tile, lane = trial; chosen positions kept in LDS.
// grid T, block 64, dynamic LDS omega*64*4 B.
__global__ __launch_bounds__(64) void k_mc_hqc_secret(u64 *__restrict__ planes, int n, int N, int omega, int batch,
                                                      long first, unsigned k0, unsigned k1, int *__restrict__ out_y)
{
    extern __shared__ int chosen[];  // [omega][64]
    mc_hqc_secret_body(chosen, planes, n, N, omega, batch, TrialRange{first}, k0, k1, out_y);
}

// The oracle's answers of scaldpc_mc_hqc_run_soft: every check draws an OUTCOME conditional on its true bit, and the outcome
// brings the reported bit and the prior the decoder is given with it (law: include/scaldpc.h; McHqcLaw, scaldpc_mc_law.h).
//   synd   u64 [tile][R]       in: the true bits c = Hin y; out: the reported bits c ^ flips[outcome]
//   plane  float [tile][R][64] out: the prior LLR of check column N + r per codeword -- the plane k_soft_convert writes and
//                              SoftPrior reads; one 256-B store per (tile, check)
//   acc_flips / acc_cost  int [batch], zeroed by the caller: checks reported wrong / oracle calls spent (acc_cost may be null)
//   out_outcome  uint8 [batch][R] or null: the outcome drawn (an export path: strided byte stores)
// The shape of k_mc_bernoulli: wave = (tile, 16 consecutive checks), lane = trial, one Philox call per four checks, the word
// of check r = stream-0 word r -- the one k_mc_bernoulli<true> flips by.  The thresholds, LLRs and costs are uniform reads of
// the kernel argument; the outcome is the number of thresholds of the true bit's row at or below the word, and since those
// do not decrease, the LLR and cost of the last threshold passed are the outcome's.  The lanes of a ragged last tile get
// bit 0 and LLR 0 and report nothing.  The wave that owns a syndrome word reads it before its lane 0 replaces it.
// grid (ceil(R/64), T), block 256.
__global__ __launch_bounds__(256) void k_mc_hqc_outcome(McHqcLaw law, u64 *synd, float *__restrict__ plane, int R, int batch,
                                                        long first, unsigned k0, unsigned k1, int *__restrict__ acc_flips,
                                                        int *__restrict__ acc_cost, uint8_t *__restrict__ out_outcome)
{
    mc_hqc_outcome_body(law, synd, plane, R, batch, TrialRange{first}, k0, k1, acc_flips, acc_cost, out_outcome);
}

// diff[t] |= OR_v (a[t][v] ^ b[t][v]) over v < nv (plane rows of stride n).  grid (ceil(nv/256), T).
__global__ __launch_bounds__(256) void k_mc_compare(const u64 *__restrict__ a, const u64 *__restrict__ bq, int n, int nv,
                                                    u64 *__restrict__ diff)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int t = blockIdx.y;
    u64 d = 0;
    if (v < nv) d = a[(size_t)t * n + v] ^ bq[(size_t)t * n + v];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) d |= __shfl_xor(d, off);
    if ((threadIdx.x & 63) == 0 && d) atomicOr(diff + t, d);
}

// success[b] = !diff bit; iters passthrough.  grid T, block 64.
__global__ __launch_bounds__(64) void k_mc_result(const u64 *__restrict__ diff, const int *__restrict__ iters, int batch,
                                                  uint8_t *__restrict__ out_success, int *__restrict__ out_iters)
{
    const int t = blockIdx.x, c = threadIdx.x;
    const long b = (long)t * TW + c;
    if (b >= batch) return;
    out_success[b] = (uint8_t)(((diff[t] >> c) & 1) ^ 1);
    if (out_iters) out_iters[b] = iters[b];
}

// ---------------------------------------------------------------------------
// Straggler compaction (early-exit runs).  Codewords are independent, so the ones a
// group has not converged after a few iterations can be re-decoded FROM THEIR INPUTS in
// dense tiles of their own -- bit-identical results, without dragging 64-codeword tiles
// that are mostly finished through the remaining iterations.  These kernels move the
// per-codeword bits / values between the original tiles and the compact ones.
// ids[slot] = original codeword (or -1), slot_of[codeword] = compact slot (or -1).
// ---------------------------------------------------------------------------
// dst[t2][x] bit c2 = src[id>>6][x] bit (id&63), id = ids[64 t2 + c2].  grid (ceil(len/64), T2), block 256.
__global__ __launch_bounds__(256) void k_gather_planes(const u64 *__restrict__ src, int len,
                                                       const int *__restrict__ ids, u64 *__restrict__ dst)
{
    const int lane = threadIdx.x & 63;
    const int x0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const int t2 = blockIdx.y;
    if (x0 >= len) return;
    const int id = ids[(size_t)t2 * TW + lane];
    const int nx = min(16, len - x0);
    for (int j = 0; j < nx; j++) {
        const int bit = id >= 0 ? (int)((src[(size_t)(id >> 6) * len + x0 + j] >> (id & 63)) & 1) : 0;
        const u64 w = __ballot(bit);
        if (lane == 0) dst[(size_t)t2 * len + x0 + j] = w;
    }
}

// The same for the per-codeword prior plane of a soft call (float [tile][cols][64]): dst[t2][j][c2] = src[id>>6][j][id&63],
// LLR 0 in the empty slots.  grid (ceil(cols/4), T2), block 256 = 4 columns, lane = compact slot.
__global__ __launch_bounds__(256) void k_gather_prior(const float *__restrict__ src, int cols, const int *__restrict__ ids,
                                                      float *__restrict__ dst)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t2 = blockIdx.y;
    if (j >= cols) return;
    const int id = ids[(size_t)t2 * TW + lane];
    dst[((size_t)t2 * cols + j) * TW + lane] = id >= 0 ? src[((size_t)(id >> 6) * cols + j) * TW + (id & 63)] : 0.0f;
}

// dst[t][x] bits of the codewords with slot_of >= 0 are replaced by src2[slot>>6][x] bit (slot&63).
// grid (ceil(len/64), T), block 256.
__global__ __launch_bounds__(256) void k_scatter_planes(u64 *__restrict__ dst, int len,
                                                        const int *__restrict__ slot_of,
                                                        const u64 *__restrict__ src2)
{
    const int lane = threadIdx.x & 63;
    const int x0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const int t = blockIdx.y;
    if (x0 >= len) return;
    const int sl = slot_of[(size_t)t * TW + lane];
    const u64 mask = __ballot(sl >= 0);
    if (mask == 0) return;
    const int nx = min(16, len - x0);
    for (int j = 0; j < nx; j++) {
        const int bit = sl >= 0 ? (int)((src2[(size_t)(sl >> 6) * len + x0 + j] >> (sl & 63)) & 1) : 0;
        const u64 w = __ballot(bit);
        if (lane == 0) {
            const size_t o = (size_t)t * len + x0 + j;
            dst[o] = (dst[o] & ~mask) | (w & mask);
        }
    }
}

// iteration counters and converged bits back to the original positions.  grid T, block 64.
__global__ __launch_bounds__(64) void k_scatter_state(int *__restrict__ iters, u64 *__restrict__ conv,
                                                      const int *__restrict__ slot_of,
                                                      const int *__restrict__ iters2, const u64 *__restrict__ conv2)
{
    const int t = blockIdx.x, c = threadIdx.x;
    const int sl = slot_of[(size_t)t * TW + c];
    if (sl >= 0) iters[(size_t)t * TW + c] = iters2[sl];
    const int bit = sl >= 0 ? (int)((conv2[sl >> 6] >> (sl & 63)) & 1) : 0;
    const u64 w = __ballot(bit), mask = __ballot(sl >= 0);
    if (c == 0 && mask) conv[t] = (conv[t] & ~mask) | (w & mask);
}

// posteriors back to the original positions.  grid (n, T), block 64.
__global__ __launch_bounds__(64) void k_scatter_post(float *__restrict__ post, int n, const int *__restrict__ slot_of,
                                                     const float *__restrict__ post2)
{
    const int v = blockIdx.x, t = blockIdx.y, c = threadIdx.x;
    const int sl = slot_of[(size_t)t * TW + c];
    if (sl >= 0) post[((size_t)t * n + v) * TW + c] = post2[((size_t)(sl >> 6) * n + v) * TW + (sl & 63)];
}

// ---------------------------------------------------------------------------
// K6, continued: the per-trial counters of scaldpc_mc_hqc_run_stats.  The kernel belongs with k_mc_compare; its definition
// stands at the END of this header so that the kernels above keep their order in the code object.  Where a new kernel lands
// there moves every other one, and the plain sweep (scaldpc_mc_hqc_run_soft, which never launches this kernel) measured
// 0.2 - 0.9 ms per 161 ms call above the commit before with the definition up there, 0.4 ms with it here; the numbers, and
// what is not understood about them, are in profiles/hqc_stats/hqc_stats_cost_mi355x.txt.
// ---------------------------------------------------------------------------
// The counters tracking.add_decoder_stats keeps per decode (simulate/hqc.py:709-758), for every trial of a sweep, from the three
// bit planes a finished scaldpc_mc_hqc_run_stats call holds -- a column count of bit matrices, nothing else is read:
//   hard   u64 [tile][n]  the error estimate            truth  u64 [tile][n]  the secret's indicator (columns < N)
//   recv   u64 [tile][n]  the message: columns >= N carry the reported check bits
//   stats  int [batch][5], zeroed by the caller: unsatisfied, good_flips, bad_flips, found_bad_satisfied_checks,
//          found_bad_unsatisfied_checks.  The decoded check bit is hard ^ reported, so a check reported 0 and decoded 1 is
//          hard & ~reported, and a check reported 1 and decoded 0 is hard & reported.
// lane = trial (the shape of k_mc_hqc_outcome): a wave takes MC_STATS_RUN consecutive nodes of a tile, reads every plane word
// once as a wave-uniform value, and lane c adds its bit.  The four waves of a block meet in LDS; one integer atomicAdd per
// lane and nonzero counter leaves the block (integer sums: the result does not depend on the order).  The lanes of a ragged
// last tile report nothing.  grid (ceil(n / (4 MC_STATS_RUN)), T), block 256.
constexpr int MC_STATS_RUN = 256;
__global__ __launch_bounds__(256) void k_mc_hqc_stats(const u64 *__restrict__ hard, const u64 *__restrict__ truth,
                                                      const u64 *__restrict__ recv, int n, int N, int batch,
                                                      int *__restrict__ stats)
{
    __shared__ int part[5][TW];
    const int lane = threadIdx.x & 63, w = rfl(threadIdx.x >> 6), t = blockIdx.y;
    for (int i = threadIdx.x; i < 5 * TW; i += 256) (&part[0][0])[i] = 0;
    __syncthreads();
    const int v0 = min((blockIdx.x * 4 + w) * MC_STATS_RUN, n), v1 = min(v0 + MC_STATS_RUN, n);
    const size_t row = (size_t)t * n;
    int unsat = 0, good = 0, bad = 0, bad_sat = 0, bad_unsat = 0;
#pragma unroll 4
    for (int v = v0; v < min(v1, N); v++) {  // the secret's columns
        const u64 e = hard[row + v], y = truth[row + v];
        good += (int)(((e & y) >> lane) & 1);
        bad += (int)(((e & ~y) >> lane) & 1);
    }
#pragma unroll 4
    for (int v = max(v0, N); v < v1; v++) {  // the check columns
        const u64 e = hard[row + v], c = recv[row + v];
        unsat += (int)((c >> lane) & 1);
        bad_sat += (int)(((e & ~c) >> lane) & 1);
        bad_unsat += (int)(((e & c) >> lane) & 1);
    }
    const int mine[5] = {unsat, good, bad, bad_sat, bad_unsat};
#pragma unroll
    for (int k = 0; k < 5; k++)
        if (mine[k]) atomicAdd(&part[k][lane], mine[k]);
    __syncthreads();
    const long b = (long)t * TW + lane;
    if (w != 0 || b >= batch) return;
#pragma unroll
    for (int k = 0; k < 5; k++)
        if (part[k][lane]) atomicAdd(stats + (size_t)b * 5 + k, part[k][lane]);
}

}  // namespace
