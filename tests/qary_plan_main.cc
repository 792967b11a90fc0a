// Prints the launch plan of a q-ary call (sca-ldpc_amd/csrc/scaldpc_qary_plan.h) for tests/test_qary_plan.py:
//   qary_plan_main special R N E Q QS W maxdc mindc maxdv batch [key=value ...]
// -> one line of name=value pairs (refused=1 alone when the plan refuses the shape).
//   qary_plan_main -
// -> the same for every line of standard input (the same words, blank separated): one process for a sweep.  Host code only.
#include "../sca-ldpc_amd/csrc/scaldpc_qary_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static int one_plan(const std::vector<std::string> &a)
{
    if (a.size() < 11) {
        fprintf(stderr, "usage: qary_plan_main special R N E Q QS W maxdc mindc maxdv batch [key=value ...]\n");
        return 2;
    }
    QaryShape g;
    g.special = atoi(a[0].c_str()) != 0;
    int *const field[] = {&g.R, &g.N, &g.E, &g.Q, &g.QS, &g.W, &g.maxdc, &g.mindc, &g.maxdv};
    for (int i = 0; i < 9; i++) *field[i] = atoi(a[1 + i].c_str());
    const int batch = atoi(a[10].c_str());
    QaryKnobs kn;
    for (size_t i = 11; i < a.size(); i++) {
        const size_t eq = a[i].find('=');
        if (eq == std::string::npos || !set_knob(kn, a[i].substr(0, eq).c_str(), a[i].substr(eq + 1).c_str())) {
            fprintf(stderr, "unknown knob %s\n", a[i].c_str());
            return 2;
        }
    }
    printf("wave=%d unroll=%d tree=%d dp=%d dp_min=%d dp_split=%d dp_split2=%d llr_tiled=%d var_small=%d timing=%d ", kn.wave, kn.unroll,
           kn.tree, kn.dp, kn.dp_min, kn.dp_split, kn.dp_split2, kn.llr_tiled, kn.var_small, kn.timing);
    QaryPlan p;
    if (qary_plan(g, kn, batch, &p)) {
        printf("refused=1\n");
        return 0;
    }
    printf("refused=0 check=%d var=%d llr=%d llr_tiled_b=%d llr_tiled_s=%d init=%d check_parts=%d check_words128=%d wave_fallback_nb=%d T=%d "
           "var_T=%d check_lds=%zu wave_lds=%zu tree_lds=%zu var_lds=%zu dp_any_lds=%zu\n",
           (int)p.check, (int)p.var, (int)p.llr, (int)p.llr_tiled_b, (int)p.llr_tiled_s, (int)p.init, p.check_parts, (int)p.check_words128,
           p.wave_fallback_nb, p.T, p.var_T, p.check_lds, p.wave_lds, p.tree_lds, p.var_lds, p.dp_any_lds);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::string(argv[1]) == "-") {
        std::string line;
        while (std::getline(std::cin, line)) {
            std::istringstream in(line);
            std::vector<std::string> a;
            for (std::string w; in >> w;) a.push_back(w);
            if (a.empty()) continue;
            if (const int rc = one_plan(a)) return rc;
        }
        return 0;
    }
    return one_plan(std::vector<std::string>(argv + 1, argv + argc));
}
