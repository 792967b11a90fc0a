// Prints the launch plan of a q-ary call (sca-ldpc_amd/csrc/scaldpc_qary_plan.h) for tests/test_qary_plan.py:
//   qary_plan_main special R N E Q QS W maxdc mindc maxdv batch [key=value ...]
// -> one line of name=value pairs (refused=1 alone when the plan refuses the shape).  Host code only.
#include "../sca-ldpc_amd/csrc/scaldpc_qary_plan.h"

#include <cstdio>
#include <string>

int main(int argc, char **argv)
{
    if (argc < 12) {
        fprintf(stderr, "usage: %s special R N E Q QS W maxdc mindc maxdv batch [key=value ...]\n", argv[0]);
        return 2;
    }
    QaryShape g;
    g.special = atoi(argv[1]) != 0;
    int *const field[] = {&g.R, &g.N, &g.E, &g.Q, &g.QS, &g.W, &g.maxdc, &g.mindc, &g.maxdv};
    for (int i = 0; i < 9; i++) *field[i] = atoi(argv[2 + i]);
    const int batch = atoi(argv[11]);
    QaryKnobs kn;
    for (int i = 12; i < argc; i++) {
        const std::string a = argv[i];
        const size_t eq = a.find('=');
        if (eq == std::string::npos || !set_knob(kn, a.substr(0, eq).c_str(), a.substr(eq + 1).c_str())) {
            fprintf(stderr, "unknown knob %s\n", argv[i]);
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
           "check_lds=%zu wave_lds=%zu tree_lds=%zu var_lds=%zu\n",
           (int)p.check, (int)p.var, (int)p.llr, (int)p.llr_tiled_b, (int)p.llr_tiled_s, (int)p.init, p.check_parts, (int)p.check_words128,
           p.wave_fallback_nb, p.T, p.check_lds, p.wave_lds, p.tree_lds, p.var_lds);
    return 0;
}
