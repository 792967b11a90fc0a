// Soft output of the q-ary decoders (scaldpc_qary_min_sum_batch_soft / _special_min_sum_batch_soft): what the last
// variable update (decoder.rs:634-658 / decoder_special.rs:566-609) knows beyond the symbol it decides.
//   soft_margin        the first-minimum scan of decoder.rs:694-704 with the runner-up kept: symbol and fl(m2 - m1)
//   k_q_soft_transpose staging [row][Bp] (lane = codeword, what the variable kernels write coalesced) -> the caller's
//                      [batch][rows] through 64 x 64 LDS tiles: the cost table and the margins, up to three row ranges a launch
//   k_q_unmet          checks whose integer sum of h * x over the row's edges is nonzero (decoder.rs:336-337), per codeword
// Included by scaldpc_qary.hip only.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// One scan over a row of totals, the reference's rule (strict <, NaN never selected, default index 0): `ma` is the
// decision; m2 the smallest total over the OTHER symbols by the same rule (+inf if there is none).  A total that lowers
// the minimum hands the old minimum down, one that does not may still lower the runner-up: after the scan m2 is the
// minimum over every non-NaN total except the decided one -- the two-pass definition, in one pass.
struct SoftScan {
    float mv = INFINITY, m2 = INFINITY;
    int ma = 0;
    __device__ __forceinline__ void step(float x, int q)
    {
        if (x < mv) {
            m2 = mv;
            mv = x;
            ma = q;
        } else if (x < m2)
            m2 = x;
    }
};

// Up to three row ranges of staging arrays, each with its own destination and row length (DecoderSpecial: the coefficient
// rows, the row-sum rows; the margins ride along as a third).  Range i owns the blocks tile0[i] .. tile0[i + 1] - 1 of grid.x.
struct SoftSegs {
    const float *src[3];  // [rows[i]][Bp]
    float *dst[3];        // [batch][rows[i]]
    int rows[3];
    int tile0[4];
};

// grid (tile0[3], Bp / 64), block 256.  A block moves 64 rows x 64 codewords: wave w reads rows w, w + 4, ... (lane =
// codeword: one full 256-B row per load) into LDS with pitch 65, then writes codewords w, w + 4, ... (lane = row: 256 B
// of one codeword's row per store; LDS column reads at stride 65 hit 64 different banks).  Rows past rows[i] and codewords
// past `batch` are neither read nor written.
__global__ __launch_bounds__(256) void k_q_soft_transpose(SoftSegs sg, int batch, long Bp)
{
    __shared__ float tile[64 * 65];
    const int i = (int)blockIdx.x >= sg.tile0[2] ? 2 : (int)blockIdx.x >= sg.tile0[1] ? 1 : 0;
    const float *__restrict__ src = sg.src[i];
    float *__restrict__ dst = sg.dst[i];
    const int rows = sg.rows[i];
    const int r0 = ((int)blockIdx.x - sg.tile0[i]) * 64;
    const long b0 = (long)blockIdx.y * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nr = min(64, rows - r0), nc = (int)min(64L, batch - b0);
    if (lane < nc)
        for (int r = w; r < nr; r += 4) tile[r * 65 + lane] = src[(size_t)(r0 + r) * Bp + b0 + lane];
    __syncthreads();
    if (lane < nr)
        for (int c = w; c < nc; c += 4) dst[(size_t)(b0 + c) * rows + r0 + lane] = tile[lane * 65 + c];
}

// hard: the staged symbols [N][Bp] (lane = codeword).  grid (ceil(R / RPB), Bp / 64), block 64: a block takes RPB
// consecutive checks for 64 codewords, so a batch of one still spreads the rows over the machine; each lane adds its count
// to unmet[codeword] with one integer atomic (order free: the count is deterministic).  unmet is zeroed by the caller.
template <int RPB>
__global__ __launch_bounds__(64) void k_q_unmet(const int *__restrict__ row_ptr, const int *__restrict__ edge_var,
                                                const int *__restrict__ edge_h, const signed char *__restrict__ hard, int R,
                                                int batch, long Bp, int *__restrict__ unmet)
{
    const long b = (long)blockIdx.y * 64 + threadIdx.x;
    if (b >= batch) return;
    const int c0 = blockIdx.x * RPB, c1 = min(R, c0 + RPB);
    int cnt = 0;
    for (int c = c0; c < c1; c++) {
        int s = 0;
        for (int e = row_ptr[c]; e < row_ptr[c + 1]; e++) s += edge_h[e] * (int)hard[(size_t)edge_var[e] * Bp + b];
        cnt += s != 0;
    }
    if (cnt) atomicAdd(unmet + b, cnt);
}

}  // namespace
