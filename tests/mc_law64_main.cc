// Prints the outcome law scaldpc_mc_hqc_run_stats_f64 builds from its tables (mc_hqc_law64, sca-ldpc_amd/csrc/scaldpc_mc_law.h)
// for tests/test_ref64_mc.py.  Every line of standard input is one table, blank separated, as tests/mc_law_main.cc takes them:
//   K R want_cost have_costs  w[0][0..K-1]  w[1][0..K-1]  flips[0..K-1]  probs[0..K-1]  [costs[0..K-1]]
// -> one line: "refused=1 <reason>", or "refused=0 K=.. flips=.. t0=a,b,.. t1=.. ratio=<float64 bit patterns, hex> cost=..",
// followed by " same32=1" when thresholds, flips and costs equal those mc_hqc_law builds from the probabilities rounded to float.
// The arrays are allocated at exactly their length, so that a read past K is the sanitizer's to report.  Host code only.
#include "../sca-ldpc_amd/csrc/scaldpc_mc_law.h"

#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

template <typename T>
static bool read_array(std::istringstream &in, int count, std::unique_ptr<T[]> &out)
{
    out.reset(new T[count > 0 ? count : 0]);
    for (int i = 0; i < count; i++) {
        std::string word;
        if (!(in >> word)) return false;
        out[i] = (T)strtod(word.c_str(), nullptr);  // ("nan", "inf" and negative numbers included)
    }
    return true;
}

static int one_table(const std::string &line)
{
    std::istringstream in(line);
    int K, R, want_cost, have_costs;
    if (!(in >> K >> R >> want_cost >> have_costs)) return 2;
    std::unique_ptr<double[]> w, flips_in, costs_in, probs;
    if (!read_array(in, 2 * K, w) || !read_array(in, K, flips_in) || !read_array(in, K, probs)) return 2;
    if (have_costs && !read_array(in, K, costs_in)) return 2;
    std::unique_ptr<uint8_t[]> flips(new uint8_t[K > 0 ? K : 0]);
    std::unique_ptr<int32_t[]> costs(new int32_t[K > 0 ? K : 0]);
    std::unique_ptr<float[]> rounded(new float[K > 0 ? K : 0]);
    for (int k = 0; k < K; k++) {
        flips[k] = (uint8_t)(int)flips_in[k];
        rounded[k] = (float)probs[k];
        if (have_costs) costs[k] = (int32_t)(long long)costs_in[k];
    }
    McHqcLaw64 law;
    char why[160];
    if (mc_hqc_law64(w.get(), flips.get(), probs.get(), have_costs ? costs.get() : nullptr, K, R, want_cost != 0, &law, why, sizeof why)) {
        printf("refused=1 %s\n", why);
        return 0;
    }
    printf("refused=0 K=%d flips=%u", law.K, law.flips);
    for (int b = 0; b < 2; b++) {
        printf(" t%d=", b);
        for (int k = 0; k < law.K; k++) printf("%s%llu", k ? "," : "", law.t[b][k]);
    }
    printf(" ratio=");
    for (int k = 0; k < law.K; k++) {
        uint64_t bits;
        memcpy(&bits, &law.ratio[k], 8);
        printf("%s%016llx", k ? "," : "", (unsigned long long)bits);
    }
    printf(" cost=");
    for (int k = 0; k < law.K; k++) printf("%s%d", k ? "," : "", law.cost[k]);
    McHqcLaw law32;
    bool same = !mc_hqc_law(w.get(), flips.get(), rounded.get(), have_costs ? costs.get() : nullptr, K, R, want_cost != 0, &law32, why, sizeof why);
    same = same && law32.K == law.K && law32.flips == law.flips && !memcmp(law32.t, law.t, sizeof law.t) && !memcmp(law32.cost, law.cost, sizeof law.cost);
    printf(" same32=%d\n", same ? 1 : 0);
    return 0;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        if (const int rc = one_table(line)) {
            fprintf(stderr, "malformed line: %s\n", line.c_str());
            return rc;
        }
    }
    return 0;
}
