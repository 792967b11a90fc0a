// Prints the law scaldpc_mc_qary_run_secret builds from its prior and tables (sca-ldpc_amd/csrc/scaldpc_mc_law.h) for
// tests/test_qary_secret_mc.py.  Every line of standard input is one call, blank separated:
//   Qb Kb Qs Ks first_trial batch async null_mask  prior[Qb]  levels_b[Kb][Qb]  weights_b[Qb][Kb]  levels_s[Ks][Qs]  weights_s[Qs][Ks]
// (null_mask: bit 0 prior, 1 levels_b, 2 weights_b, 3 levels_s, 4 weights_s are passed as NULL)
// -> one line: "refused=<kind> <reason>", or "refused=0 prior=a,b,.. tb=.. ts=.. bestb=.. bests=..".
// The arrays are allocated at exactly their length, so that a read past them is the sanitizer's to report.  Host code only.
#include "../sca-ldpc_amd/csrc/scaldpc_mc_law.h"

#include <iostream>
#include <memory>
#include <sstream>
#include <string>

template <typename T>
static bool read_array(std::istringstream &in, long count, std::unique_ptr<T[]> &out)
{
    out.reset(new T[count > 0 ? count : 0]);
    for (long i = 0; i < count; i++) {
        std::string word;
        if (!(in >> word)) return false;
        out[i] = (T)strtod(word.c_str(), nullptr);  // ("nan", "inf" and negative numbers included)
    }
    return true;
}

template <typename T>
static void print_list(const char *name, const std::vector<T> &v)
{
    printf(" %s=", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s%lld", i ? "," : "", (long long)v[i]);
}

static int one_call(const std::string &line)
{
    std::istringstream in(line);
    int Q[2], K[2], batch, async, null_mask;
    long long first;
    if (!(in >> Q[0] >> K[0] >> Q[1] >> K[1] >> first >> batch >> async >> null_mask)) return 2;
    std::unique_ptr<double[]> prior, w[2];
    std::unique_ptr<float[]> lv[2];
    const long nb = (long)(K[0] > 0 ? K[0] : 0) * Q[0], ns = (long)(K[1] > 0 ? K[1] : 0) * Q[1];
    if (!read_array(in, Q[0], prior) || !read_array(in, nb, lv[0]) || !read_array(in, nb, w[0]) || !read_array(in, ns, lv[1]) ||
        !read_array(in, ns, w[1]))
        return 2;
    const float *levels[2] = {null_mask & 2 ? nullptr : lv[0].get(), null_mask & 8 ? nullptr : lv[1].get()};
    const double *weights[2] = {null_mask & 4 ? nullptr : w[0].get(), null_mask & 16 ? nullptr : w[1].get()};
    McSecretLaw law;
    char why[200];
    const int kind = mc_qary_secret_law(null_mask & 1 ? nullptr : prior.get(), levels, weights, K, Q, first, batch, async != 0, &law, why,
                                        sizeof why);
    if (kind) {
        printf("refused=%d %s\n", kind, why);
        return 0;
    }
    printf("refused=0");
    print_list("prior", law.prior);
    print_list("tb", law.t[0]);
    print_list("ts", law.t[1]);
    print_list("bestb", law.best[0]);
    print_list("bests", law.best[1]);
    printf("\n");
    return 0;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        if (const int rc = one_call(line)) {
            fprintf(stderr, "malformed line\n");
            return rc;
        }
    }
    return 0;
}
