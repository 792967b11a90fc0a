// Prints the outcome law scaldpc_mc_hqc_run_soft builds from its tables (sca-ldpc_amd/csrc/scaldpc_mc_law.h) for
// tests/test_hqc_soft_mc.py.  Every line of standard input is one table, blank separated:
//   K R want_cost have_costs  w[0][0..K-1]  w[1][0..K-1]  flips[0..K-1]  probs[0..K-1]  [costs[0..K-1]]
// -> one line: "refused=1 <reason>", or "refused=0 K=.. flips=.. t0=a,b,.. t1=.. llr=<float32 bit patterns, hex> cost=..".
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
        const double v = strtod(word.c_str(), nullptr);  // ("nan", "inf" and negative numbers included)
        out[i] = (T)v;
    }
    return true;
}

static int one_table(const std::string &line)
{
    std::istringstream in(line);
    int K, R, want_cost, have_costs;
    if (!(in >> K >> R >> want_cost >> have_costs)) return 2;
    std::unique_ptr<double[]> w;
    std::unique_ptr<double[]> flips_in, costs_in;
    std::unique_ptr<float[]> probs;
    if (!read_array(in, 2 * K, w) || !read_array(in, K, flips_in) || !read_array(in, K, probs)) return 2;
    if (have_costs && !read_array(in, K, costs_in)) return 2;
    std::unique_ptr<uint8_t[]> flips(new uint8_t[K > 0 ? K : 0]);
    std::unique_ptr<int32_t[]> costs(new int32_t[K > 0 ? K : 0]);
    for (int k = 0; k < K; k++) {
        flips[k] = (uint8_t)(int)flips_in[k];
        if (have_costs) costs[k] = (int32_t)(long long)costs_in[k];
    }
    McHqcLaw law;
    char why[160];
    if (mc_hqc_law(w.get(), flips.get(), probs.get(), have_costs ? costs.get() : nullptr, K, R, want_cost != 0, &law, why, sizeof why)) {
        printf("refused=1 %s\n", why);
        return 0;
    }
    printf("refused=0 K=%d flips=%u", law.K, law.flips);
    for (int b = 0; b < 2; b++) {
        printf(" t%d=", b);
        for (int k = 0; k < law.K; k++) printf("%s%llu", k ? "," : "", law.t[b][k]);
    }
    printf(" llr=");
    for (int k = 0; k < law.K; k++) {
        uint32_t bits;
        memcpy(&bits, &law.llr[k], 4);
        printf("%s%08x", k ? "," : "", bits);
    }
    printf(" cost=");
    for (int k = 0; k < law.K; k++) printf("%s%d", k ? "," : "", law.cost[k]);
    printf("\n");
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
