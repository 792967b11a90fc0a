// Device code of scaldpc_bp_decode_batch_f64: the reference package's OWN arithmetic -- product-sum in the probability-ratio
// domain, float64 (oracle/bp_oracle_impl.h, method 0 with REAL = double) -- operation for operation, so that
// decisions, iteration counts and converged flags are the oracle's on every trial and the posteriors differ by the last log
// alone.  Included by scaldpc_bp.hip after scaldpc_bp_kernels.h (same anonymous namespace, same bit planes and state).
//
// What it is for: reproducing the reference's numbers, and a full-batch float64 key for the fp32 tanh kernels.  What it is
// not: the throughput path -- no record form, no fused first iteration, no row-parallel or LDS variant; no compaction in
// scaldpc_bp_decode_batch_f64, one level of it in the float64 Monte-Carlo sweeps (ref64_handover; scaldpc_bp_mc64.hip).
//
// Layout: TWO message arrays, as the oracle keeps them,
//     x : double [tile][edge][64]   bit-to-check ratios     (written by the variable pass, read by the check pass)
//     c : double [tile][edge][64]   check-to-bit ratios     (written by the check pass, read by the variable pass)
// edge id = CSR position, lane = codeword: a 512-B coalesced row per (tile, edge), 8 B per lane.  A check wave walks its row's
// contiguous edges, a variable wave gathers its column's rows through the CSC permutation.
// A node of up to REF64_ROW_CAP / REF64_COL_CAP edges is register-resident: its inputs are read ONCE, the oracle's exclusive
// prefixes stay in registers, its outputs are written ONCE -- 16 B per edge, codeword and pass, twice the fp32 message form's
// bytes.  Wider nodes take the any-degree loops, which park the prefixes in the output array's own slots between the forward
// and the backward sweep, exactly where the oracle parks them (40 B per edge, codeword and pass).  The order of
// multiplications is the oracle's in either form.
//
// Arithmetic: only *, +, - and the IEEE-correct double division, in the oracle's order; the translation unit is built with
// -ffp-contract=off, so no multiply-add is fused.  The one library call is the posterior's log().
// Lanes already done (latched by k_parity_fin, or padding) write nothing.
#pragma once

namespace {

// Where the ratio-domain prior r = p / (1 - p) of column v for codeword `lane` of tile `tl` comes from: the handle's shared
// array (cols = 0), or for the columns [first_col, first_col + cols) the per-codeword plane double [tile][cols][64]
// (tl counts from the first tile of the launch: the host passes that tile's plane).
struct Ratio64 {
    const double *ratio;  // [n]
    const double *plane;  // [tile][cols][64] or null
    int first_col, cols;
    __device__ __forceinline__ double operator()(int v, int tl, int lane) const
    {
        const double *src = (cols && v >= first_col) ? plane + ((size_t)tl * cols + (v - first_col)) * TW + lane : ratio + v;
        return *src;
    }
};

// the factor a bit-to-check ratio contributes to its row's products: 2 / (1 + x) - 1
__device__ __forceinline__ double ratio64_factor(double x) { return 2.0 / (1.0 + x) - 1.0; }

// Per-codeword prior probabilities double [batch][cols] (one row per codeword) -> the ratio plane double [tile][cols][64],
// r = p / (1 - p) by the same IEEE division as the shared priors' (p = 0 -> 0, p = 1 -> inf): k_soft_convert's 64 x 64 LDS
// transpose.  The lanes of a ragged last tile get r = 0.  A value that is no probability (outside [0, 1], NaN) leaves the
// smallest such index b * cols + j in *bad (preset to ~0) and r = 1 in the plane.
// grid (ceil(cols/64), T), block 256.
__global__ __launch_bounds__(256) void k_ratio64_convert(const double *__restrict__ probs, int cols, int batch,
                                                         double *__restrict__ plane, u64 *__restrict__ bad)
{
    __shared__ double tile[64][65];
    const int t = blockIdx.y, j0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < 64; c += 4) {
        const long b = (long)t * TW + c;
        double r = 0.0;
        if (b < batch && j0 + lane < cols) {
            const size_t i = (size_t)b * cols + j0 + lane;
            const double p = probs[i];
            if (p >= 0.0 && p <= 1.0)
                r = p / (1.0 - p);
            else {
                r = 1.0;
                atomicMin(bad, (u64)i);
            }
        }
        tile[c][lane] = r;
    }
    __syncthreads();
    for (int j = w; j < 64; j += 4)
        if (j0 + j < cols) plane[((size_t)t * cols + j0 + j) * TW + lane] = tile[lane][j];
}

// posterior double [tile][var][64] -> double [batch][n]: k_unpack_llr in float64.  grid (ceil(n/64), T), block 256.
__global__ __launch_bounds__(256) void k_unpack_llr64(const double *__restrict__ post, int n, int batch,
                                                      double *__restrict__ out)
{
    __shared__ double tile[64][65];
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

// Initial bit-to-check messages: every edge of column j carries r_j.  wave = (edge, tile).
// grid (ceil(E/4), G), block 256.
__global__ __launch_bounds__(256) void k_init_ratio64(const int *__restrict__ col_idx, double *__restrict__ x, long E,
                                                      Ratio64 prior)
{
    const int lane = threadIdx.x & 63;
    const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int tl = blockIdx.y;
    if (e >= E) return;
    x[((size_t)tl * E + e) * TW + lane] = prior(rfl(col_idx[e]), tl, lane);
}

// Check pass.  wave = (row, tile), lane = codeword.  The oracle's two sweeps over the row's edges in ascending column:
//   forward   t = +-1 by the syndrome bit;  c[e] = t;  t *= 2 / (1 + x[e]) - 1
//   backward  s = 1;  c[e] *= s;  c[e] = (1 - c[e]) / (1 + c[e]);  s *= 2 / (1 + x[e]) - 1
// Any-degree form: the prefixes are parked in c[e]; the factor is formed again in the backward sweep from the same x[e] by
// the same operations: the same value.
__device__ __forceinline__ void check_ratio64_loop(const double *xt, double *ct, long e0, long e1, double t, bool live)
{
    for (long e = e0; e < e1; e++) {
        const double f = ratio64_factor(xt[e * TW]);
        if (live) ct[e * TW] = t;
        t *= f;
    }
    double s = 1.0;
    for (long e = e1 - 1; e >= e0; e--) {
        const double f = ratio64_factor(xt[e * TW]);
        double v = ct[e * TW] * s;
        v = (1.0 - v) / (1.0 + v);
        if (live) ct[e * TW] = v;
        s *= f;
    }
}

// Register-resident form for a row of deg <= CAP edges: the factors are formed once and kept (2 * CAP VGPRs), every message is
// read once and written once.  The prefixes of only HALF the row are kept at a time (CAP VGPRs): the forward chain runs over
// the first half without storing, stores the second half's prefixes, the backward sweep consumes them; then the first half's
// prefixes are formed again -- the same multiplications on the same values, so the same prefixes -- and the backward sweep
// goes on.  (Both halves' prefixes at once are 4 * CAP VGPRs: past 256 at CAP = 64, one wave per SIMD.)
// The guards k < deg are wave-uniform.
template <int CAP>
__device__ __forceinline__ void check_ratio64_regs(const double *xt, double *ct, int deg, double t0, bool live)
{
    constexpr int HALF = CAP / 2;
    double f[CAP], p[HALF];
#pragma unroll
    for (int k = 0; k < CAP; k++)
        if (k < deg) f[k] = ratio64_factor(xt[(size_t)k * TW]);
    double t = t0;
#pragma unroll
    for (int k = 0; k < HALF; k++)
        if (k < deg) t *= f[k];
#pragma unroll
    for (int k = HALF; k < CAP; k++)
        if (k < deg) {
            p[k - HALF] = t;
            t *= f[k];
        }
    double s = 1.0;
#pragma unroll
    for (int k = CAP - 1; k >= HALF; k--)
        if (k < deg) {
            double v = p[k - HALF] * s;
            v = (1.0 - v) / (1.0 + v);
            if (live) ct[(size_t)k * TW] = v;
            s *= f[k];
        }
    t = t0;
#pragma unroll
    for (int k = 0; k < HALF; k++)
        if (k < deg) {
            p[k] = t;
            t *= f[k];
        }
#pragma unroll
    for (int k = HALF - 1; k >= 0; k--)
        if (k < deg) {
            double v = p[k] * s;
            v = (1.0 - v) / (1.0 + v);
            if (live) ct[(size_t)k * TW] = v;
            s *= f[k];
        }
}

constexpr int REF64_ROW_CAP = 64;  // widest register-resident row (HQC rows are W + 1 = 51 or 61 edges)
constexpr int REF64_COL_CAP = 32;  // widest register-resident column

// CAP = the register-resident width the launch is built for: the host picks the smallest of 16 / 52 / 64 that holds the graph's
// widest row (a kernel's register allocation is that of its widest form, and the check pass lives on waves per SIMD); rows
// wider than CAP take the loop.
// synd: [tile][m] planes, done: [tile] masks, both of the launch's first tile.
// grid (ceil(m/4), G), block 256.
template <int CAP>
__global__ __launch_bounds__(256, 2) void k_check_ratio64(const int *__restrict__ row_ptr, const double *__restrict__ x,
                                                          double *c, long E, int m, const u64 *__restrict__ synd,
                                                          const u64 *__restrict__ done)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int tl = blockIdx.y;
    if (r >= m) return;
    const u64 dw = done[tl];
    if (dw == ~0ull) return;  // whole tile frozen
    const bool live = !((dw >> lane) & 1);
    const long e0 = rfl(row_ptr[r]), e1 = rfl(row_ptr[r + 1]);
    const int deg = (int)(e1 - e0);
    const double *xt = x + (size_t)tl * E * TW + lane;
    double *ct = c + (size_t)tl * E * TW + lane;
    const double t = ((synd[(size_t)tl * m + r] >> lane) & 1) ? -1.0 : 1.0;
    if (deg <= CAP)
        check_ratio64_regs<CAP>(xt + e0 * TW, ct + e0 * TW, deg, t, live);
    else
        check_ratio64_loop(xt, ct, e0, e1, t, live);
}

// Variable pass.  wave = (column, tile), lane = codeword.  The oracle's two sweeps over the column's edges in ascending row:
//   forward   t = r_j;  x[e] = t;  t *= c[e];  if (t != t) t = 1
//   posterior L = log(1 / t), decision t >= 1      (write_out: early-exit runs every pass, fixed-iteration runs the last)
//   backward  s = 1;  x[e] *= s;  s *= c[e];  if (s != s) s = 1
// Both forms return the forward product t and leave the backward sweep to `finish` (the outputs are written in between, as
// the oracle writes them; nothing depends on that order).
// Any-degree form: the prefixes are parked in x[e].
__device__ __forceinline__ double var_ratio64_loop_fwd(const int *__restrict__ ce, const double *ct, double *xt, int d, double t,
                                                       bool live)
{
    for (int k = 0; k < d; k++) {
        const size_t e = (size_t)rfl(ce[k]) * TW;
        if (live) xt[e] = t;
        t *= ct[e];
        if (t != t) t = 1.0;
    }
    return t;
}
__device__ __forceinline__ void var_ratio64_loop_bwd(const int *__restrict__ ce, const double *ct, double *xt, int d, bool live)
{
    double s = 1.0;
    for (int k = d - 1; k >= 0; k--) {
        const size_t e = (size_t)rfl(ce[k]) * TW;
        const double v = xt[e] * s;
        if (live) xt[e] = v;
        s *= ct[e];
        if (s != s) s = 1.0;
    }
}
// Register-resident form for a column of d <= CAP edges: incoming messages and prefixes in registers (4 * CAP VGPRs).
template <int CAP>
struct VarRatio64Regs {
    double cv[CAP], p[CAP];
    __device__ __forceinline__ double fwd(const int *__restrict__ ce, const double *ct, int d, double t)
    {
#pragma unroll
        for (int k = 0; k < CAP; k++)
            if (k < d) cv[k] = ct[(size_t)rfl(ce[k]) * TW];
#pragma unroll
        for (int k = 0; k < CAP; k++)
            if (k < d) {
                p[k] = t;
                t *= cv[k];
                if (t != t) t = 1.0;
            }
        return t;
    }
    __device__ __forceinline__ void bwd(const int *__restrict__ ce, double *xt, int d, bool live) const
    {
        double s = 1.0;
#pragma unroll
        for (int k = CAP - 1; k >= 0; k--)
            if (k < d) {
                if (live) xt[(size_t)rfl(ce[k]) * TW] = p[k] * s;
                s *= cv[k];
                if (s != s) s = 1.0;
            }
    }
};

// decision plane word (a done lane keeps its bit) and posterior of column j from the forward product t
__device__ __forceinline__ void var_ratio64_out(double t, int tl, int j, int n, int lane, u64 dw, bool live,
                                                u64 *__restrict__ hard, double *__restrict__ post)
{
    const u64 ones = __ballot(t >= 1.0);
    const size_t w = (size_t)tl * n + j;
    if (lane == 0) hard[w] = (hard[w] & dw) | (ones & ~dw);
    if (post && live) post[w * TW + lane] = log(1.0 / t);
}

// CAP = 16 or REF64_COL_CAP, the smallest that holds the graph's widest column; columns wider than CAP take the loop.
// hard: [tile][n] decision planes, post: double [tile][n][64] or null.
// grid (ceil(n/4), G), block 256.
template <int CAP>
__global__ __launch_bounds__(256) void k_var_ratio64(const int *__restrict__ col_ptr, const int *__restrict__ csc_edge,
                                                     const double *__restrict__ c, double *x, long E, int n, Ratio64 prior,
                                                     const u64 *__restrict__ done, int write_out, u64 *__restrict__ hard,
                                                     double *__restrict__ post)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int tl = blockIdx.y;
    if (j >= n) return;
    const u64 dw = done[tl];
    if (dw == ~0ull) return;  // whole tile frozen
    const bool live = !((dw >> lane) & 1);
    const int k0 = rfl(col_ptr[j]), d = rfl(col_ptr[j + 1]) - k0;
    const int *ce = csc_edge + k0;
    const double *ct = c + (size_t)tl * E * TW + lane;
    double *xt = x + (size_t)tl * E * TW + lane;
    const double r = prior(j, tl, lane);
    if (d <= CAP) {
        VarRatio64Regs<CAP> col;
        const double t = col.fwd(ce, ct, d, r);
        if (write_out) var_ratio64_out(t, tl, j, n, lane, dw, live, hard, post);
        col.bwd(ce, xt, d, live);
    } else {
        const double t = var_ratio64_loop_fwd(ce, ct, xt, d, r, live);
        if (write_out) var_ratio64_out(t, tl, j, n, lane, dw, live, hard, post);
        var_ratio64_loop_bwd(ce, ct, xt, d, live);
    }
}

// (The two kernels the float64 Monte-Carlo sweeps add -- the outcome draw that writes the ratio plane and the double twin of
// k_gather_prior -- are a translation unit of their own, scaldpc_bp_mc64.hip: this unit's code object stays what it was.)

}  // namespace
