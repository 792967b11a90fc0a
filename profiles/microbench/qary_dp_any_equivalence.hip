// k_q_special_check_dp_any (the min-plus recursion of DecoderSpecial's check update for rows of any length, tables in LDS)
// compared MESSAGE FOR MESSAGE, as bit patterns, against a plain enumeration on the CPU in the reference's own form
// (decoder_special.rs:531-554 restated below: every assignment forms S left to right and lowers beta_j[d_j] with
// S - a_j[d_j], f32::min semantics).  The kernel is included from the product's header as it stands.
//   B = 1: rows of 0, 1, 2, 5, 9, 12 coefficient edges;  B = 2: 1, 3, 6, 8, 9, 10;  B = 3: 2, 6, 8
//   BSUM = nb B (every row-sum symbol within reach of an assignment or beyond the alphabet) and nb B + 2 (symbols nothing reaches)
//   inputs: smooth random LLRs over 20 binades (every addition rounds), heavy ties, impossible symbols (+inf), NaN alphas
//   (the variable update's inf - inf), zeros, sums that overflow to +inf.
// Rows of at most 20 000 assignments: 2 checks x 70 codewords (a ragged batch: two blocks per check), all compared.  Longer
// rows: one check, the kernel runs all 70 columns and the host enumerates the codewords at lanes 0, 63, 64 and 69.
// At B = 2, nb = 6 the Kyber kernel k_q_special_check_dp<5, 6, 1> is held to the same messages.
// A difference is a bug in the kernel or a hole in the monotonicity argument of the header.
// Run by tests/test_qary_special_any_gpu.py.  Build: make -C profiles/microbench qary_dp_any_equivalence
// (--host-only: the enumerations alone, timed, without touching a device)
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef unsigned long long u64;
#include "../../sca-ldpc_amd/csrc/scaldpc_qary_special.h"

#define HIPOK(x)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) {                                                                   \
            fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);           \
            return 2;                                                                             \
        }                                                                                         \
    } while (0)

namespace {
constexpr int BATCH = 70;
constexpr long Bp = 128;
constexpr int MAXNB = 12;

u64 rng_state = 0x9E3779B97F4A7C15ull;
unsigned rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33);
}
float unit() { return (float)(rnd() & 0xFFFFFF) / 16777216.0f; }

// one alpha of the given flavour
float draw(int flavour)
{
    switch (flavour) {
        case 0: return -logf(unit() + 1e-7f) * ldexpf(1.0f, (int)(rnd() % 20) - 10);  // smooth, 20 binades
        case 1: return 0.25f * (float)(rnd() % 8);                                    // ties everywhere
        case 2: return (rnd() % 4 == 0) ? INFINITY : -logf(unit() + 1e-7f);            // impossible symbols
        case 3: return (rnd() % 6 == 0) ? NAN : (rnd() % 6 == 0 ? INFINITY : 3.0f * unit());  // NaN alphas
        case 4: return (rnd() % 3 == 0) ? 0.0f : unit();                               // zeros (normalised messages have one)
        default: return (rnd() % 5 == 0) ? FLT_MAX * (0.3f + 0.5f * unit()) : 1e30f * unit();  // sums overflow
    }
}

// f32::min(m, c) for a running minimum m that starts at +inf: a NaN candidate is ignored, and m is never NaN itself
inline float fmin32(float m, float c) { return c < m ? c : m; }

// decoder_special.rs:531-554, one check of one codeword: nb coefficient edges of QB symbols, then the row-sum edge.  (Built
// with -ffp-contract=off and without fast-math: every + and - below is one f32 operation.)
void host_check(int nb, int QB, int B, int BSUM, const float *a /* [nb][QB] */, const float *as /* [QS] */, float *bb, float *bs)
{
    const int QS = 2 * BSUM + 1;
    for (int i = 0; i < nb * QB; i++) bb[i] = INFINITY;
    for (int i = 0; i < QS; i++) bs[i] = INFINITY;
    // The assignments in an order that moves the LAST digit fastest, so that the partial sums of S (formed left to right, as the
    // reference forms them) are kept for the digits that did not move: P[j] = ((0 + a_0[d_0]) + ...) + a_{j-1}[d_{j-1}].
    int d[MAXNB + 1] = {0}, ds[MAXNB + 1] = {0};  // digits q = d + B; ds[j]: sum of the first j digits' values
    float P[MAXNB + 1] = {0.0f};
    int from = 0;  // the first digit that moved
    for (;;) {
        for (int j = from; j < nb; j++) {
            ds[j + 1] = ds[j] + d[j] - B;
            P[j + 1] = P[j] + a[j * QB + d[j]];
        }
        const int t = -ds[nb] + BSUM;
        const float S = P[nb] + as[t];
        for (int j = 0; j < nb; j++) bb[j * QB + d[j]] = fmin32(bb[j * QB + d[j]], S - a[j * QB + d[j]]);
        bs[t] = fmin32(bs[t], S - as[t]);
        int j = nb - 1;
        for (; j >= 0; j--) {
            if (d[j] < QB - 1) {
                d[j]++;
                break;
            }
            d[j] = 0;
        }
        if (j < 0) break;
        from = j;
    }
}

struct Case {
    int B, nb;
};
const Case cases[] = {{1, 0}, {1, 1}, {1, 2}, {1, 5}, {1, 9}, {1, 12}, {2, 1}, {2, 3}, {2, 6}, {2, 8}, {2, 9}, {2, 10}, {3, 2}, {3, 6}, {3, 8}};

template <int QB>
void launch_any(const int *d_row_ptr, float *d_work, int R, int BSUM, int W, int L)
{
    hipLaunchKernelGGL((k_q_special_check_dp_any<QB>), dim3(R, Bp / 64), dim3(64), (size_t)3 * L * 256, 0, d_row_ptr, d_work, BSUM, W, Bp,
                       BATCH, L);
}
}  // namespace

int main(int argc, char **argv)
{
    const bool host_only = argc > 1 && !strcmp(argv[1], "--host-only");
    const char *names[6] = {"smooth", "ties", "impossible", "nan", "zeros", "overflow"};
    int bad_total = 0;
    double host_s = 0.0;
    for (const Case &cs : cases)
        for (int extra = 0; extra <= 2; extra += 2) {
            const int B = cs.B, nb = cs.nb, QB = 2 * B + 1, BSUM = nb * B + extra, QS = 2 * BSUM + 1, W = QS > QB ? QS : QB;
            const int L = (QB - 1) * nb + 1;
            double assignments = 1.0;
            for (int j = 0; j < nb; j++) assignments *= QB;
            const bool large = assignments > 20000.0;
            const int R = large ? 1 : 2;
            const long cols[4] = {0, 63, 64, BATCH - 1};
            const size_t n = (size_t)R * (nb + 1) * W * Bp;
            const auto at = [&](int c, int j, int q, long b) { return ((size_t)(c * (nb + 1) + j) * W + q) * Bp + b; };
            std::vector<int> row_ptr(R + 1);
            for (int c = 0; c <= R; c++) row_ptr[c] = c * (nb + 1);
            int *d_row_ptr = nullptr;
            float *d_work = nullptr;
            if (!host_only) {
                HIPOK(hipMalloc(&d_row_ptr, sizeof(int) * (R + 1)));
                HIPOK(hipMalloc(&d_work, sizeof(float) * n));
                HIPOK(hipMemcpy(d_row_ptr, row_ptr.data(), sizeof(int) * (R + 1), hipMemcpyHostToDevice));
            }
            const bool kyber = B == 2 && nb == 6;
            for (int flavour = 0; flavour < 6; flavour++) {
                std::vector<float> in(n, 7.0f), host, out[2];
                for (int c = 0; c < R; c++)
                    for (long b = 0; b < BATCH; b++) {
                        for (int j = 0; j < nb; j++)
                            for (int q = 0; q < QB; q++) in[at(c, j, q, b)] = draw(flavour);
                        for (int q = 0; q < QS; q++) in[at(c, nb, q, b)] = draw(flavour);
                    }
                host = in;
                std::vector<long> compared;
                for (long b = 0; b < BATCH; b++)
                    if (!large || b == cols[0] || b == cols[1] || b == cols[2] || b == cols[3]) compared.push_back(b);
                const auto t0 = std::chrono::steady_clock::now();
                std::vector<float> a((size_t)MAXNB * 7), as(QS), bb((size_t)MAXNB * 7), bs(QS);
                for (int c = 0; c < R; c++)
                    for (long b : compared) {
                        for (int j = 0; j < nb; j++)
                            for (int q = 0; q < QB; q++) a[j * QB + q] = in[at(c, j, q, b)];
                        for (int q = 0; q < QS; q++) as[q] = in[at(c, nb, q, b)];
                        host_check(nb, QB, B, BSUM, a.data(), as.data(), bb.data(), bs.data());
                        for (int j = 0; j < nb; j++)
                            for (int q = 0; q < QB; q++) host[at(c, j, q, b)] = bb[j * QB + q];
                        for (int q = 0; q < QS; q++) host[at(c, nb, q, b)] = bs[q];
                    }
                host_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (host_only) continue;
                const int nk = kyber ? 2 : 1;
                for (int k = 0; k < nk; k++) {
                    HIPOK(hipMemcpy(d_work, in.data(), sizeof(float) * n, hipMemcpyHostToDevice));
                    if (k == 1)
                        hipLaunchKernelGGL((k_q_special_check_dp<5, 6, 1>), dim3(R, Bp / 64), dim3(64), 0, 0, d_row_ptr, d_work, BSUM, W, Bp,
                                           BATCH);
                    else if (QB == 3) launch_any<3>(d_row_ptr, d_work, R, BSUM, W, L);
                    else if (QB == 5) launch_any<5>(d_row_ptr, d_work, R, BSUM, W, L);
                    else launch_any<7>(d_row_ptr, d_work, R, BSUM, W, L);
                    HIPOK(hipGetLastError());
                    HIPOK(hipDeviceSynchronize());
                    out[k].resize(n);
                    HIPOK(hipMemcpy(out[k].data(), d_work, sizeof(float) * n, hipMemcpyDeviceToHost));
                }
                long cnt = 0, diff[2] = {0, 0}, inf_out = 0, pad_touched = 0;
                for (int c = 0; c < R; c++) {
                    for (long b : compared)
                        for (int j = 0; j <= nb; j++)
                            for (int q = 0; q < (j < nb ? QB : QS); q++) {
                                const size_t i = at(c, j, q, b);
                                uint32_t h;
                                memcpy(&h, &host[i], 4);
                                cnt++;
                                inf_out += std::isinf(host[i]);
                                for (int k = 0; k < nk; k++) {
                                    uint32_t g;
                                    memcpy(&g, &out[k][i], 4);
                                    if (g != h && diff[k]++ < 3)
                                        fprintf(stderr, "B %d nb %d BSUM %d %s kernel %d: check %d codeword %ld edge %d symbol %d: %a (host) vs %a\n", B,
                                                nb, BSUM, names[flavour], k, c, b, j, q, host[i], out[k][i]);
                                }
                            }
                    // the padding lanes store nothing
                    for (long b = BATCH; b < Bp; b++)
                        for (int j = 0; j <= nb; j++)
                            for (int q = 0; q < W; q++) pad_touched += memcmp(&out[0][at(c, j, q, b)], &in[at(c, j, q, b)], 4) != 0;
                }
                if (kyber)
                    printf("CASE B=%d nb=%-2d BSUM=%-2d %-10s %ld messages (%ld of them +inf): %ld differ in dp_any, %ld differ in dp<5,6,1>, %ld "
                           "differ in the padding\n", B, nb, BSUM, names[flavour], cnt, inf_out, diff[0], diff[1], pad_touched);
                else
                    printf("CASE B=%d nb=%-2d BSUM=%-2d %-10s %ld messages (%ld of them +inf): %ld differ in dp_any, %ld differ in the padding\n", B,
                           nb, BSUM, names[flavour], cnt, inf_out, diff[0], pad_touched);
                bad_total += (int)(diff[0] + diff[1] + pad_touched != 0);
            }
            if (!host_only) {
                hipFree(d_row_ptr);
                hipFree(d_work);
            }
        }
    printf("host enumeration: %.1f s\n", host_s);
    return bad_total ? 1 : 0;
}
