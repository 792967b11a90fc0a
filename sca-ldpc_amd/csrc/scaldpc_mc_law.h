// The trial laws of the Monte-Carlo entry points as the HOST builds them, before anything is queued: the cumulative thresholds of
// a table of weights (one rule, shared by scaldpc_mc_qary_run and scaldpc_mc_hqc_run_soft) and the validated outcome table of
// scaldpc_mc_hqc_run_soft in the form its kernel takes by value.  The laws themselves are stated in include/scaldpc.h.
// Plain C++17 with no HIP in it: tests/mc_law_main.cc drives this header from a host program under the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

// floor(p 2^32), 0 for p <= 0, 2^32 for p >= 1: a 32-bit word is below it with probability p (to 2^-32)
static inline unsigned long long bernoulli_threshold(double p)
{
    return p >= 1.0 ? (1ull << 32) : p <= 0.0 ? 0ull : (unsigned long long)(p * 4294967296.0);
}

// T_k = thr(w_0 + ... + w_k), the sum accumulated left to right in float64; from the last entry of nonzero weight on T_k is
// 2^32, so that an entry of weight 0 is never drawn by "the smallest k with word < T_k" -- in the middle of a table (T_k =
// T_{k-1}) or at its end.  Refused (1, with the reason in msg): a weight that is no probability, a sum outside 1 +- 1e-6.
static inline int mc_cumulative_thresholds(const char *name, const double *w, int K, unsigned long long *t, char *msg, size_t len)
{
    double sum = 0.0;
    int last = 0;
    for (int k = 0; k < K; k++) {
        if (!(w[k] >= 0.0 && w[k] <= 1.0)) {
            snprintf(msg, len, "%s: weight %d is %g, not a probability", name, k, w[k]);
            return 1;
        }
        sum += w[k];
        t[k] = bernoulli_threshold(sum);
        if (w[k] > 0.0) last = k;
    }
    if (!(std::fabs(sum - 1.0) <= 1e-6)) {
        snprintf(msg, len, "%s: the weights sum to %.9g, not to 1 +- 1e-6", name, sum);
        return 1;
    }
    for (int k = last; k < K; k++) t[k] = 1ull << 32;
    return 0;
}

constexpr int MC_HQC_MAX_OUTCOMES = 32;

// The outcome table of scaldpc_mc_hqc_run_soft as k_mc_hqc_outcome takes it, by value (776 B of kernel arguments, read
// uniformly): a check whose TRUE bit is b draws the smallest k with word < t[b][k]; bit k of `flips` says whether outcome k
// reports the complement; llr[k] is the prior LLR the decoder is given with it, cost[k] the oracle calls it spent.
// Entries from K on are never read (thresholds 2^32 from the last outcome of nonzero weight on).
struct McHqcLaw {
    unsigned long long t[2][MC_HQC_MAX_OUTCOMES];
    float llr[MC_HQC_MAX_OUTCOMES];
    int cost[MC_HQC_MAX_OUTCOMES];
    unsigned flips;
    int K;
};

// Everything that can be refused about the tables of scaldpc_mc_hqc_run_soft (1, with the reason in msg), and the law.
// weights [2][K], flips [K], probs [K], costs [K] or null; R = checks per trial (a trial's cost must fit an int32);
// want_cost: the caller asked for out_cost.  llr[k] = logf((1.0f - p) / p) in float32, the expression of the decoder's own
// priors (p = 0 / p = 1: +-inf).
static inline int mc_hqc_law(const double *weights, const uint8_t *flips, const float *probs, const int32_t *costs, int K, int R,
                             bool want_cost, McHqcLaw *law, char *msg, size_t len)
{
    *law = McHqcLaw();
    if (!weights || !flips || !probs) {
        snprintf(msg, len, "NULL table");
        return 1;
    }
    if (K < 1 || K > MC_HQC_MAX_OUTCOMES) {
        snprintf(msg, len, "%d outcomes, 1 .. %d are taken", K, MC_HQC_MAX_OUTCOMES);
        return 1;
    }
    if (want_cost && !costs) {
        snprintf(msg, len, "out_cost needs the costs of the outcomes");
        return 1;
    }
    static const char *const name[2] = {"weights[0]", "weights[1]"};
    for (int b = 0; b < 2; b++)
        if (mc_cumulative_thresholds(name[b], weights + (size_t)b * K, K, law->t[b], msg, len)) return 1;
    int max_cost = 0;
    for (int k = 0; k < K; k++) {
        if (flips[k] > 1) {
            snprintf(msg, len, "flips[%d] = %d is neither 0 nor 1", k, (int)flips[k]);
            return 1;
        }
        if (!(probs[k] >= 0.0f && probs[k] <= 1.0f)) {
            snprintf(msg, len, "probs[%d] = %g is not a probability", k, (double)probs[k]);
            return 1;
        }
        if (costs && (costs[k] < 0 || costs[k] > 65535)) {
            snprintf(msg, len, "costs[%d] = %d is outside [0, 65535]", k, (int)costs[k]);
            return 1;
        }
        law->flips |= (unsigned)flips[k] << k;
        law->llr[k] = logf((1.0f - probs[k]) / probs[k]);
        law->cost[k] = costs ? costs[k] : 0;
        if (law->cost[k] > max_cost) max_cost = law->cost[k];
    }
    if ((long long)R * max_cost >= (1ll << 31)) {
        snprintf(msg, len, "%d checks of up to %d oracle calls each do not fit a trial's int32 cost", R, max_cost);
        return 1;
    }
    law->K = K;
    return 0;
}
