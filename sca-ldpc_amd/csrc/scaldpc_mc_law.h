// The trial laws of the Monte-Carlo entry points as the HOST builds them, before anything is queued: the cumulative thresholds of
// a table of weights (one rule, shared by scaldpc_mc_qary_run and scaldpc_mc_hqc_run_soft) and the validated outcome table of
// scaldpc_mc_hqc_run_soft in the form its kernel takes by value, and the law of scaldpc_mc_qary_run_secret (a drawn secret, outcomes
// conditional on every variable's true symbol).  The laws themselves are stated in include/scaldpc.h.
// Plain C++17 with no HIP in it: tests/mc_law_main.cc drives this header from a host program under the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

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

// The same table for the float64 sweeps (scaldpc_mc_hqc_run_stats_f64), as k_mc_hqc_outcome64 takes it by value (904 B): the
// thresholds, flips and costs are McHqcLaw's -- the trial law does not know the decode's precision -- and an outcome brings the
// RATIO r = p / (1 - p) of its prior, formed here in double by the division the float64 decode's own priors go through
// (p = 0 -> 0, p = 1 -> inf).
struct McHqcLaw64 {
    unsigned long long t[2][MC_HQC_MAX_OUTCOMES];
    double ratio[MC_HQC_MAX_OUTCOMES];
    int cost[MC_HQC_MAX_OUTCOMES];
    unsigned flips;
    int K;
};

// mc_hqc_law with probs double [K], taken as they are: the values are checked in double (a value that only rounds into [0, 1]
// is refused), everything else is mc_hqc_law's on the rounded values, whose thresholds, flips and costs are copied.
static inline int mc_hqc_law64(const double *weights, const uint8_t *flips, const double *probs, const int32_t *costs, int K, int R,
                               bool want_cost, McHqcLaw64 *law, char *msg, size_t len)
{
    *law = McHqcLaw64();
    float rounded[MC_HQC_MAX_OUTCOMES] = {};
    if (probs && K >= 1 && K <= MC_HQC_MAX_OUTCOMES)
        for (int k = 0; k < K; k++) {
            if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) {
                snprintf(msg, len, "probs[%d] = %g is not a probability", k, probs[k]);
                return 1;
            }
            rounded[k] = (float)probs[k];
        }
    McHqcLaw law32;
    if (mc_hqc_law(weights, flips, probs ? rounded : nullptr, costs, K, R, want_cost, &law32, msg, len)) return 1;
    for (int b = 0; b < 2; b++)
        for (int k = 0; k < MC_HQC_MAX_OUTCOMES; k++) law->t[b][k] = law32.t[b][k];
    for (int k = 0; k < K; k++) {
        law->ratio[k] = probs[k] / (1.0 - probs[k]);
        law->cost[k] = law32.cost[k];
    }
    law->flips = law32.flips;
    law->K = K;
    return 0;
}

// ------------------------------------------------------------------------------------------ scaldpc_mc_qary_run_secret

constexpr int MC_SECRET_MAX_LEVELS = 32;
// A launch keeps one table in dynamic LDS: its K LLR rows (K Q floats), the thresholds of every true symbol (Q K 32-bit words)
// and the number of thresholds below 2^32 per true symbol (Q words).
constexpr size_t MC_SECRET_MAX_LDS = 65536;
static inline size_t mc_secret_lds_bytes(int K, int Q) { return 4 * ((size_t)2 * K * Q + (size_t)Q); }

// One pmf row as decoder.rs:668-692 reads it (the rule of PmfScan in scaldpc_qary.hip, restated without HIP): the f32 sum, left
// to right from 0.0, must lie within 1 +- 1e-3, and *best is the first strict maximum (a NaN is never chosen) -- the symbol whose
// LLR is the row's first zero, i.e. what the arg-min rule of decoder.rs:694-704 decides from the row alone.
// 0: fine, 1: the sum fails, 2: no maximum (all NaN).
static inline int mc_pmf_row(const float *p, int Q, int *best)
{
    float sum = 0.0f, mx = 0.0f;
    bool have = false;
    *best = 0;
    for (int q = 0; q < Q; q++) {
        const float x = p[q];
        sum += x;
        if (x == x && (!have || x > mx)) {
            mx = x;
            have = true;
            *best = q;
        }
    }
    if (!have) return 2;
    return !(sum < 1.0f + 0.001f) || !(sum > 1.0f - 0.001f);
}

// The law of scaldpc_mc_qary_run_secret as the host builds it (table 0: coefficient variables, 1: row-sum variables):
//   prior    [Q[0]]        cumulative thresholds of prior_b: the secret symbol is the smallest q with word < prior[q]
//   t[i]     [Q[i]][K[i]]  row s: the cumulative thresholds of weights_i[s], the outcomes of a variable whose TRUE symbol is s
//   best[i]  [K[i]]        the VALUE (index - (Q[i] - 1) / 2) a variable decides from the pmf row of level k alone
struct McSecretLaw {
    int Q[2] = {0, 0}, K[2] = {0, 0};
    std::vector<unsigned long long> prior, t[2];
    std::vector<signed char> best[2];
};

enum { MC_SECRET_OK = 0, MC_SECRET_EINVAL = 1, MC_SECRET_EPMF = 2, MC_SECRET_EDEGREE = 3 };

// Everything that can be refused about the tables and the trial range of scaldpc_mc_qary_run_secret (the kind of refusal, with
// the reason in msg), and the law.  levels[i] float [K[i]][Q[i]], weights[i] double [Q[i]][K[i]], prior_b double [Q[0]].
static inline int mc_qary_secret_law(const double *prior_b, const float *const levels[2], const double *const weights[2], const int K[2],
                                     const int Q[2], long long first_trial, int batch, bool async, McSecretLaw *law, char *msg,
                                     size_t len)
{
    static const char *const lname[2] = {"levels_b", "levels_s"}, *const wname[2] = {"weights_b", "weights_s"};
    *law = McSecretLaw();
    if (!prior_b || !levels[0] || !levels[1] || !weights[0] || !weights[1]) {
        snprintf(msg, len, "NULL prior or table");
        return MC_SECRET_EINVAL;
    }
    if (batch <= 0) {
        snprintf(msg, len, "batch must be positive");
        return MC_SECRET_EINVAL;
    }
    if (first_trial < 0) {
        snprintf(msg, len, "first_trial must not be negative");
        return MC_SECRET_EINVAL;
    }
    if (async) {
        snprintf(msg, len, "SCALDPC_F_ASYNC: a q-ary Monte-Carlo call is synchronous");
        return MC_SECRET_EINVAL;
    }
    for (int i = 0; i < 2; i++) {
        if (Q[i] < 1 || Q[i] > 255 || !(Q[i] & 1)) {
            snprintf(msg, len, "%s: an alphabet of %d symbols", lname[i], Q[i]);
            return MC_SECRET_EINVAL;
        }
        if (K[i] < 1 || K[i] > MC_SECRET_MAX_LEVELS) {
            snprintf(msg, len, "%s: %d levels, 1 .. %d are taken", lname[i], K[i], MC_SECRET_MAX_LEVELS);
            return MC_SECRET_EINVAL;
        }
    }
    for (int i = 0; i < 2; i++)
        if (mc_secret_lds_bytes(K[i], Q[i]) > MC_SECRET_MAX_LDS) {
            snprintf(msg, len, "%s: %d levels of %d symbols need %zu B of LDS in a launch (4 (2 K Q + Q)), %zu are there", lname[i],
                     K[i], Q[i], mc_secret_lds_bytes(K[i], Q[i]), MC_SECRET_MAX_LDS);
            return MC_SECRET_EDEGREE;
        }
    law->prior.resize(Q[0]);
    if (mc_cumulative_thresholds("prior_b", prior_b, Q[0], law->prior.data(), msg, len)) return MC_SECRET_EINVAL;
    for (int i = 0; i < 2; i++) {
        law->t[i].resize((size_t)Q[i] * K[i]);
        for (int s = 0; s < Q[i]; s++) {
            const std::string name = std::string(wname[i]) + "[" + std::to_string(s) + "]";
            if (mc_cumulative_thresholds(name.c_str(), weights[i] + (size_t)s * K[i], K[i], law->t[i].data() + (size_t)s * K[i], msg, len))
                return MC_SECRET_EINVAL;
        }
    }
    for (int i = 0; i < 2; i++) {
        law->best[i].resize(K[i]);
        for (int k = 0; k < K[i]; k++) {
            int best = 0;
            const int bad = mc_pmf_row(levels[i] + (size_t)k * Q[i], Q[i], &best);
            if (bad) {
                snprintf(msg, len, bad == 2 ? "%s: level %d: No maximum probability found" : "%s: level %d does not sum to 1 +- 1e-3 (decoder.rs:683-684)",
                         lname[i], k);
                return MC_SECRET_EPMF;
            }
            law->best[i][k] = (signed char)(best - (Q[i] - 1) / 2);
        }
        law->Q[i] = Q[i];
        law->K[i] = K[i];
    }
    return MC_SECRET_OK;
}
