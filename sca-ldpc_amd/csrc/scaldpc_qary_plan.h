// Which kernels a q-ary call runs, decided ONCE per call by a pure function of the graph's shape, the handle's knobs and
// the batch: scaldpc_qary.hip's qary_run asks qary_plan before anything is queued and every launch reads the answer.
// Plain C++17, no HIP: tests/qary_plan_main.cc builds it with a host compiler and tests/test_qary_plan.py holds it to
// the rules of include/scaldpc.h and DESIGN.md 4.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>

// What qary_build works out of H (Q = 2B + 1 coefficient symbols, QS row-sum symbols (= Q for the plain decoder),
// W = max(Q, QS) = width of a message row, E edges, the extreme check degrees and the largest variable degree).
struct QaryShape {
    bool special = false;
    int R = 0, N = 0, E = 0, Q = 0, QS = 0, W = 0, maxdc = 0, mindc = 0, maxdv = 0;
};

// Test / tuning knobs of one handle (include/scaldpc.h, scaldpc_qary_configure).
struct QaryKnobs {
    int wave = -1;        // -1: wave-parallel enumeration for batches <= 256 and the special decoder; 0 / 1 force
    int unroll = 1;       // register-resident unrolled enumeration for small alphabets
    int tree = 1;         // special decoder: tree-walk check kernel for the Kyber shape (QB = 5, 6 coefficient edges)
    int dp = 1;           // min-plus recursion instead of the enumeration (Kyber shape: batches >= dp_min; Q = 3: always)
    int dp_min = 5;       // (below, one wave per (check, codeword) of the tree walk is as fast or faster: profiles/r04/kyber_form_sweep.log)
    int dp_split = 64;    // up to this batch the row's edges are split over four waves (same log)
    int dp_split2 = 192;  // ... and up to this one over two
    int llr_tiled = 1;    // probability -> LLR conversion through an LDS tile (coalesced reads)
    int var_small = 1;    // register-resident variable update for Q = 3 / 5 / 7 / 15 and columns of at most 4 checks
    int dp_any = -1;      // special decoder, Q = 3 / 5 / 7: min-plus recursion for rows of any length (tables in LDS). -1: for checks of
                          // more than 8 edges, which nothing else takes; 1: for every shape; 0: never (such checks are then refused)
    int timing = 0;       // bracket every check / variable launch with HIP events (scaldpc_qary_last_timing); off: nothing is recorded
};

inline bool set_knob(QaryKnobs &k, const char *key, const char *val)
{
    if (!key || !val) return false;
    const int x = atoi(val);
    if (!strcmp(key, "wave")) k.wave = x < 0 ? -1 : x != 0;
    else if (!strcmp(key, "unroll")) k.unroll = x != 0;
    else if (!strcmp(key, "tree")) k.tree = x != 0;
    else if (!strcmp(key, "dp")) k.dp = x != 0;
    else if (!strcmp(key, "dp_min")) k.dp_min = std::max(1, x);
    else if (!strcmp(key, "dp_split")) k.dp_split = std::max(0, x);
    else if (!strcmp(key, "dp_split2")) k.dp_split2 = std::max(0, x);
    else if (!strcmp(key, "timing")) k.timing = x != 0;
    else if (!strcmp(key, "llr_tiled")) k.llr_tiled = x != 0;
    else if (!strcmp(key, "var_small")) k.var_small = x != 0;
    else if (!strcmp(key, "dp_any")) k.dp_any = x < 0 ? -1 : x != 0;
    else return false;
    return true;
}

// The check kernel: the values are scaldpc_qary_last_timing's info[1] and the indices of qary.CHECK_KERNELS.
enum class QCheck : int {
    NONE = -1,  // a graph without edges
    UNROLLED_3_7 = 0,
    UNROLLED_5_5 = 1,
    SPECIAL_TREE = 2,  // (+ the wave kernel for rows of another degree: wave_fallback_nb)
    SPECIAL_WAVE = 3,
    WAVE = 4,
    SPECIAL_LANE = 5,  // k_q_special_check
    LANE = 6,          // k_q_check
    SPECIAL_DP = 7,    // (any number of parts; + the wave kernel as for the tree)
    DP_3_7 = 8,
    SPECIAL_DP_ANY = 9,  // k_q_special_check_dp_any<Q>: every row, whatever its length
};
enum class QVar : int { GENERIC = 0, SMALL = 1 /* <Q, 4> */, SMALL_SPECIAL = 2 /* <5, 4, 25> */ };
enum class QLlr : int {
    FUSED_BOTH = 0,  // tiled, writes the first messages too; both alphabets of the special decoder in one launch
    FUSED_EACH = 1,  // the same, one launch per alphabet
    UNFUSED = 2,     // per alphabet tiled (llr_tiled_b / _s) or plain, then k_q_init (init)
};

struct QaryPlan {
    QCheck check = QCheck::NONE;
    QVar var = QVar::GENERIC;
    QLlr llr = QLlr::UNFUSED;
    bool llr_tiled_b = false, llr_tiled_s = false;  // UNFUSED: the coefficient rows' / the row-sum rows' conversion through the tile
    bool init = false;                              // k_q_init is launched
    int check_parts = 1;         // SPECIAL_DP: waves that share a (check, 64 codewords)
    bool check_words128 = false;  // LANE: 128-bit digit words (checks of 9 .. 16 edges)
    int wave_fallback_nb = -1;    // SPECIAL_TREE / SPECIAL_DP: skip_nb of the k_q_special_check_wave launch that follows for the rows of
                                  // another degree; -1: no such launch (every row has that many coefficient edges, or another form)
    int T = 64;                   // threads (= codewords) per block of the LDS-staged lane kernels
    int var_T = 64;               // threads (= codewords) per block of k_q_var: as many (<= 64) as keep its two W-row tables within 64 KB
    size_t check_lds = 0, wave_lds = 0, tree_lds = 0, var_lds = 0;  // dynamic LDS of LANE / SPECIAL_LANE, the wave kernels, the tree walk, k_q_var
    size_t dp_any_lds = 0;        // SPECIAL_DP_ANY: three tables of (Q - 1)(maxdc - 1) + 1 entries, 64 lanes each
};

// Nonzero: nothing runs this shape.  1: the LDS-staged enumeration does not fit (plan->check_lds / plan->T then hold the bytes
// one codeword needs).  2: a special decoder's check of more than 8 edges that the any-length recursion does not take (another
// alphabet than 3 / 5 / 7 symbols, tables beyond 64 KB (plan->dp_any_lds), or the dp_any knob at 0).
inline int qary_plan(const QaryShape &g, const QaryKnobs &kn, int batch, QaryPlan *plan)
{
    constexpr size_t LDS = 64 * 1024;
    QaryPlan p;
    // threads per block of the enumeration kernels: as many (<= 64) as fit 64 KB of LDS
    const size_t per_thread = g.special ? (size_t)2 * ((g.maxdc - 1) * g.Q + g.QS) * 4 : (size_t)g.maxdc * g.Q * 9;
    while (p.T > 8 && per_thread * p.T > LDS) p.T >>= 1;
    p.check_lds = per_thread * p.T;
    if (p.check_lds > LDS) {
        *plan = p;
        return 1;
    }
    // conversion: alphabets of up to 32 symbols go through the LDS tile (coalesced reads of [codeword][variable][Q]), which also
    // writes the first variable-to-check messages (k_q_init's job) when every alphabet takes it
    const bool fused = kn.llr_tiled && g.Q <= 32 && (!g.special || g.QS <= 32) && g.E > 0;
    p.llr = !fused ? QLlr::UNFUSED : g.special ? QLlr::FUSED_BOTH : QLlr::FUSED_EACH;
    p.llr_tiled_b = !fused && kn.llr_tiled && g.Q <= 32;
    p.llr_tiled_s = !fused && kn.llr_tiled && g.special && g.QS <= 32;
    p.init = !fused && g.E > 0;
    // variable update
    const bool q_small = g.Q == 3 || g.Q == 5 || g.Q == 7 || g.Q == 15;  // (15: B = 7, the reference's criterion and unit-test decoders)
    if (!g.special && kn.var_small && g.maxdv <= 4 && q_small) p.var = QVar::SMALL;
    if (g.special && kn.var_small && g.maxdv <= 4 && g.Q == 5 && g.QS == 25) p.var = QVar::SMALL_SPECIAL;  // the Kyber SW6 classes (lib.rs:54-75)
    // k_q_var stages two rows of W floats per codeword: 64 codewords per block up to W = 128, 32 beyond (W <= 255: 65 280 B)
    while (p.var_T > 8 && (size_t)2 * g.W * p.var_T * 4 > LDS) p.var_T >>= 1;
    p.var_lds = (size_t)2 * g.W * p.var_T * 4;
    // check update.  Small batch: wave per (check, codeword), lanes share the assignment space
    // measured: wave mode 0.69 vs 3.2 ms at batch 64 (config-4 decoder), 24 vs 70 ms (Kyber SW6);
    // a tie at batch 1024, where one codeword per lane keeps global accesses coalesced
    // the special decoder (15625 assignments per check at the Kyber shape) prefers wave mode at
    // every batch size measured (93 vs 153 ms at batch 256)
    p.wave_lds = g.special ? (size_t)(((g.maxdc - 1) * g.Q + g.QS) * 65) * 4
                           : (size_t)g.maxdc * g.Q * 4 * 65 + (size_t)g.maxdc * g.Q + g.maxdc + 16;
    const bool wave_fits = p.wave_lds <= LDS;
    bool wave = kn.wave >= 0 ? kn.wave != 0 : batch <= 256 || g.special;
    wave = wave && wave_fits && g.maxdc <= 8;  // (64-bit digit words in the wave kernels)
    // special decoder, Kyber shape (B = 2, rows of up to 6 coefficient edges + the row-sum edge): tree walk, and from a few
    // codewords on the min-plus recursion (lane = codeword) instead of any enumeration
    const bool kyber = g.special && kn.wave != 0 && g.Q == 5 && g.maxdc - 1 == 6 && wave_fits;
    p.tree_lds = ((size_t)6 * g.Q + g.QS + (size_t)(6 * g.Q + g.QS) * 64) * 4;
    // special decoder, rows of any length: the recursion over LDS tables, for the checks no enumeration reaches (or on demand)
    const bool any_q = g.special && g.E > 0 && (g.Q == 3 || g.Q == 5 || g.Q == 7);
    p.dp_any_lds = g.special ? (size_t)3 * ((size_t)(g.Q - 1) * std::max(g.maxdc - 1, 0) + 1) * 64 * 4 : 0;
    const bool any = any_q && p.dp_any_lds <= LDS && (kn.dp_any == 1 || (kn.dp_any == -1 && g.maxdc > 8));
    if (g.special && g.maxdc > 8 && !any) {
        *plan = p;
        return 2;
    }
    if (!g.E) p.check = QCheck::NONE;
    else if (any) p.check = QCheck::SPECIAL_DP_ANY;
    else if (!g.special && kn.unroll && g.Q == 3 && g.maxdc <= 7) p.check = kn.dp ? QCheck::DP_3_7 : QCheck::UNROLLED_3_7;
    else if (!g.special && kn.unroll && g.Q == 5 && g.maxdc <= 5) p.check = QCheck::UNROLLED_5_5;
    else if (kyber && kn.dp && batch >= kn.dp_min) p.check = QCheck::SPECIAL_DP;
    else if (kyber && kn.tree) p.check = QCheck::SPECIAL_TREE;
    else if (wave) p.check = g.special ? QCheck::SPECIAL_WAVE : QCheck::WAVE;
    else p.check = g.special ? QCheck::SPECIAL_LANE : QCheck::LANE;
    if (p.check == QCheck::SPECIAL_DP) p.check_parts = batch <= kn.dp_split ? 4 : batch <= kn.dp_split2 ? 2 : 1;
    if ((p.check == QCheck::SPECIAL_DP || p.check == QCheck::SPECIAL_TREE) && g.mindc != g.maxdc) p.wave_fallback_nb = 6;
    p.check_words128 = p.check == QCheck::LANE && g.maxdc > 8;
    *plan = p;
    return 0;
}
