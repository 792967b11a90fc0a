// libscaldpc -- binary LDPC belief propagation on MI355X (gfx950), flooding schedule.
//
// Replaces the decode loop behind `ldpc.bp_decoder(H, ...).decode(v)` as the
// reference calls it (simulate-with-python/simulate/decode.py:155-161,171;
// simulate/hqc.py:694-699,708).  The arithmetic follows that package's sweep
// order: per check an exclusive forward/backward sweep
// over the row in ascending column, per variable an exclusive prefix/suffix
// SUM over the column in ascending row, hard decision `L <= 0 -> 1`, then
// H e == s.  Nothing is ever "total minus self", so +-inf priors (certainty-1.0
// checks, hqc.py:689) never meet an inf - inf.
//
// Memory design (measured on MI355X, profiles/microbench/rmw_stream.hip):
//   * ONE fp32 message array, updated IN PLACE: a check node reads all its v2c
//     and then overwrites them with c2v at the same addresses; a variable node
//     does the converse.  Every node owns its edges exclusively, so no other
//     thread ever sees a half-updated edge.
//         msg : float [tile][edge][64]      edge id = CSR position, tile = 64 codewords
//     A check node's edges are one contiguous range: a wave working on
//     (row, tile) streams deg x 256 B of consecutive memory; a variable node
//     gathers its 256 B edge rows through the CSC permutation.
//   * Codeword tiles are decoded in GROUPS whose message array fits the 256 MiB
//     Infinity Cache (~<= 200 MB): all max_iter iterations of a group run
//     back-to-back, so after the first touch the messages never go to HBM again
//     (an in-place read-all/write-all stream runs at ~6.5-7.3 TB/s from the
//     Infinity Cache against ~4.5 TB/s from HBM).
//   * Bit planes (syndrome, received word, hard decision, done mask):
//         u64 [tile][node]      bit c = codeword c of the tile
//     posterior : float [tile][var][64]
//
// No MFMA anywhere: this is a sparse gather/scatter stream, not a contraction.
#include "scaldpc_common.h"
#include "scaldpc_bp_sched.h"
#include "scaldpc_mc_law.h"
#include "scaldpc_trials.h"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

typedef unsigned long long u64;

using namespace scaldpc;

#include "scaldpc_bp_kernels.h"
#include "scaldpc_bp_ref64.h"  // scaldpc_bp_decode_batch_f64: the ratio-domain float64 kernels

// The two kernels the float64 sweeps add live in scaldpc_bp_mc64.hip, behind these launches (that file says why).
namespace scaldpc {
int launch_mc_hqc_outcome64(const McHqcLaw64 &law, unsigned long long *synd, double *plane, int R, int batch, int T, long first,
                            unsigned k0, unsigned k1, int *acc_flips, int *acc_cost, uint8_t *out_outcome, hipStream_t s);
int launch_gather_prior64(const double *src, int cols, const int *ids, double *dst, int T2, hipStream_t s);
// the list forms of the Monte-Carlo generators (scaldpc_bp_mc_at.hip): slot b = trial ids[b], ids on the device
int launch_mc_bernoulli_at(bool xor_into, unsigned long long *planes, int len, int batch, int T, const long long *ids, unsigned stream,
                           unsigned k0, unsigned k1, const unsigned long long *thr, unsigned long long thr0, hipStream_t s);
int launch_mc_hqc_secret_at(unsigned long long *planes, int n, int N, int omega, int batch, int T, const long long *ids, unsigned k0,
                            unsigned k1, int *out_y, hipStream_t s);
int launch_mc_hqc_outcome_at(const McHqcLaw &law, unsigned long long *synd, float *plane, int R, int batch, int T, const long long *ids,
                             unsigned k0, unsigned k1, int *acc_flips, int *acc_cost, uint8_t *out_outcome, hipStream_t s);
int launch_mc_hqc_outcome64_at(const McHqcLaw64 &law, unsigned long long *synd, double *plane, int R, int batch, int T,
                               const long long *ids, unsigned k0, unsigned k1, int *acc_flips, int *acc_cost, uint8_t *out_outcome,
                               hipStream_t s);
}  // namespace scaldpc

namespace {

// Degree buckets of one fused launch (a host-side notion: the kernels read per-wave descriptor lists built from it):
// blocks [blk[b], blk[b+1]) work on the nodes list[off[b] .. off[b]+cnt[b]) with unroll bound maxd[b] (0 = any-degree
// fallback).
struct Buckets {
    int nb;
    int maxd[MAXB];
    int off[MAXB];
    int cnt[MAXB];
    int blk[MAXB + 1];
};

struct HostBuckets {
    Buckets bk;
    pvec<int> list;
    bool has_generic = false;
};

}  // namespace

// ===========================================================================
// handle
// ===========================================================================
// Tuning / test knobs of a handle.  The environment is read ONCE, when the handle is created
// (SCALDPC_PATH, _SPLIT, _GROUP_MB, _EL_MAX, _COMPACT_AFTER, ...); afterwards
// scaldpc_bp_configure() changes them -- the decode entry points never call getenv().
// Round 4 pruned the knobs that only switched a measured-and-rejected variant back on (test_overlap, var_form = 0,
// rec_maskpos = 0, rec_xmap = 0, rec_sc1 = 0, fuse_finalize = 0, speculate = 0, minsum_loop; numbers in
// profiles/HISTORY.md): what is left selects a path, a size, or a form that something still falls back to.
struct Knobs {
    enum Path { AUTO = 0, STREAM = 1, EDGE = 2, LDS = 3 };
    int path = AUTO;
    int split = 2;            // stream lanes per tile group
    double group_mb = 215.0;  // cache-resident group budget (auto_group)
    int el_max = -1;          // row-parallel limit; -1 = per-method default (6 / 4)
    int compact_after = -1;   // -1 = default (4); 0 = no compact pass.  The fp32 scheduler: the iteration FROM which a hand-over may happen; the float64 sweeps: the iteration AT which the one hand-over happens (ref64_handover)
    int fuse_test = 1;        // early-exit tile loop: the convergence test of iteration it rides on the check pass of it + 1 wherever the host does not need the verdict in between
    int first_fused = 1;      // iteration 1 of the tile kernels without its check pass (k_var_first from the first-message table); 0 = check pass + plain variable pass
    int minsum_rec = 1;       // min-sum on the tile kernels: check pass writes per-row records + lane masks instead of messages (k_check_minsum_rec / k_var_rec); 0 = message form; 2 = 1, and columns of 33 ... 64 edges stay in the record form (rec_form)
    int settle = -1;          // fixed-iteration record-form calls: -1 = 2 on a graph [Hin | I], 0 on any other (settle_mode); 0 = every pass runs; 1 = passes return at once for tiles whose message state has stopped changing (Settle); 2 = and a learned horizon keeps them from being enqueued
    int settle_horizon = 0;   // > 0: the horizon K, forced (tiles it is wrong for are decoded again: results never depend on it)
    int settle_sparse = -1;   // tracked levels: 1 = a pass returns for rows and columns none of whose inputs changed (Settle's sparse gate); 0 = off; -1 = on where settle is 2 on a graph [Hin | I] (settle_sparse_mode)
};

// The handle's streams and events, released when the handle goes.  scaldpc_bp derives from it, so every buffer member
// has returned its device memory before they are released.
struct HandleStreams {
    int device = 0;  // the device the handle (and its stream) was created on
    hipStream_t own_stream = nullptr;
    hipStream_t aux_stream[4] = {};  // further lanes of a tile group (iterate_tiles)
    hipEvent_t ev_join[4] = {}, ev_phase[4] = {};
    HandleStreams() = default;
    HandleStreams(const HandleStreams &) = delete;
    HandleStreams &operator=(const HandleStreams &) = delete;
    ~HandleStreams()
    {
        if (own_stream) stream_release(own_stream, device);
        for (int k = 0; k < 4; k++) {
            if (aux_stream[k]) stream_release(aux_stream[k], device);
            if (ev_join[k]) (void)hipEventDestroy(ev_join[k]);
            if (ev_phase[k]) (void)hipEventDestroy(ev_phase[k]);
        }
    }
};

// Every block the handle owns is a Buf member; plain pointers below are views into one of them.
struct scaldpc_bp : HandleStreams {
    Knobs kn;
    int m = 0, n = 0;
    long E = 0;
    int max_row_deg = 0, max_col_deg = 0, min_row_deg = 0;
    // device graph (views: into d_graph, or d_csr_rp / d_csr_ci once the graph grows; d_row_list, d_var_meta and
    // d_csc_list into d_tile_tab)
    int *d_row_ptr = nullptr, *d_col_idx = nullptr, *d_col_ptr = nullptr, *d_csc_edge = nullptr;
    int *d_var_list = nullptr, *d_row_list = nullptr;
    int *d_var_meta = nullptr, *d_csc_list = nullptr;  // k_var: packed column descriptors + edge lists in launch order
    Buckets var_bk{}, row_bk{};
    bool need_scratch = false;
    // priors (view: into d_graph, or d_prior_buf once the graph grows)
    float *d_prior = nullptr;
    bool have_prior = false;
    int prior_n = 0;  // columns whose prior is set (a grown graph needs scaldpc_bp_set_channel_probs_tail for the new ones)
    // workspace (state arrays sized for cap_tiles, messages for cap_group tiles)
    int cap_tiles = 0, cap_group = 0, tile_group = 0;
    Buf<float> d_msg, d_scratch, d_post;
    Buf<u64> d_synd, d_recv, d_hard, d_done, d_conv, d_unsat;
    Buf<int> d_iters, d_remaining;
    // a soft call's per-codeword prior LLRs (scaldpc_bp_decode_batch_soft): float [tile][prob_cols][64], sized by the call;
    // d_soft_bad = the conversion kernel's "first value that is no probability" word; d_probs_in stages host input
    Buf<float> d_pprior, d_probs_in;
    Buf<u64> d_soft_bad;
    int cap_remaining = 0;  // counters per row of d_remaining (and of h_remaining)
    // d_remaining holds rem.rows rows of cap_remaining "codewords still running after iteration it" counters: every tile
    // group of a call takes the next row (zeroed once per call, not once per group: a memset is a 5 us launch in the
    // group's dependency chain); rem.slot = next free row, rem.rows = all used (the next taker zeroes the array).
    // rem.rows follows the groups a call can run (at most REM_SLOTS): max_iter defaults to n, and 512 rows of n + 2
    // counters were 44 MB -- allocated and cleared -- on an HQC-sized decoder that decodes ONE codeword.
    RemRing rem;  // slot = next free row, rows = all (scaldpc_bp_sched.h)
    SchedCounters sched;  // what the scheduler did in the last call (scaldpc_bp_last_schedule): host integers only
    // host-I/O staging
    Buf<uint8_t> d_in, d_out_bits, d_out_conv;
    Buf<float> d_out_llr;
    Buf<int> d_out_iters;
    PinnedBuf<int> h_remaining;
    // small host calls (one tile, a handful of codewords): fused reshaping kernels, one pinned staging buffer
    PinnedBuf<uint8_t> h_io;
    Buf<uint8_t> d_out_all;
    // Monte-Carlo helpers
    pvec<double> h_probs;
    Buf<u64> d_thr, d_mc, d_diff;
    Buf<int> d_ylist;
    Buf<uint8_t> d_succ;
    bool thr_valid = false;
    Buf<int> d_mc_acc;            // scaldpc_mc_hqc_run_soft: [2][batch] checks reported wrong / oracle calls spent
    Buf<int> d_mc_stats;          // scaldpc_mc_hqc_run_stats: [batch][5] counters of k_mc_hqc_stats (host callers)
    Buf<uint8_t> d_mc_outcome;    // ... and the staging block of a host call's out_outcome
    Buf<long long> d_trial_ids;   // the _at entries: the device copy of the call's trial list, [batch]
    // compact second pass over stragglers (early-exit runs)
    // (level k re-decodes the stragglers of level k-1 in dense tiles of their own; level 0 = the call's arrays)
    struct Level {
        int cap_tiles = 0;
        Buf<u64> synd, hard, done, conv, unsat;
        Buf<int> iters, ids, slot_of;
        Buf<float> post, pprior;  // pprior: the stragglers' rows of a soft call's prior plane
        Buf<double> pratio64;     // the same rows of a float64 soft sweep's ratio plane (level 1 only: ref64_handover)
    };
    static constexpr int MAX_LEVELS = SCHED_MAX_LEVELS;
    Level lv[MAX_LEVELS + 1];  // [0] unused
    long stat_levels = 0;      // deepest compact level the last call reached
    long stat_deferred = 0;  // codewords re-decoded by the compact pass in the last call
    // row-parallel path (a handful of codewords): per-codeword message / prefix arrays [codeword][edge]
    Buf<float> d_emsg;
    Buf<int> d_el_unsat;  // [iteration][64] "some row unsatisfied" flags of the fused early-exit loop
    // k_el_var: columns packed into waves ("bins") of 64 lane slots, each column a segment of `cap` lanes
    int *d_el_slots = nullptr, *d_el_slot_col = nullptr;  // views into d_el_tab: [2 * 64 * el_cap_bins] and [64 * el_cap_bins] ints
    int el_waves = 0;     // bins in use
    int el_cap_bins = 0;  // bins d_el_tab has room for
    bool el_ok = false;   // the row-parallel path can take this graph (non-empty, no row / column wider than a wave: rows <= ROW_CAP)
    pvec<int> h_el_slots, h_el_col;  // host mirrors of the two parts of d_el_tab
    pvec<int> seg_slot;            // per column: bin * 64 + first lane of its segment (-1: none)
    pvec<unsigned char> seg_cap;   // per column: lanes of its segment
    int el_open_used = 0;                 // lanes handed out in the last bin
    // A handle whose graph grows (scaldpc_bp_append_rows): CSR and priors move to allocations of their
    // own with spare capacity, the row-parallel tables keep a few free lanes per column and are
    // updated in place; everything only the tile / LDS kernels need (CSC, degree buckets, their
    // tables) is marked stale and rebuilt from the host mirror when one of those paths is next taken.
    bool incremental = false, full_stale = false;
    pvec<int> hg_col_idx;  // host CSR mirror (incremental handles)
    Buf<int> d_csr_rp, d_csr_ci;
    Buf<float> d_prior_buf;
    int ws_m = 0, ws_n = 0;  // what the workspace planes are sized for
    pvec<int> el_dirty_slot, el_dirty_col;  // words an append call changed (kept for their capacity)
    Buf<int> d_pairs;  // staging of table updates
    PinnedBuf<int> h_pairs;
    Buf<int> d_graph;  // ONE allocation behind the arrays every path needs (CSR, CSC, var list, d_prior: views into it)
    // The tables only one kernel family reads are built on that family's first use -- a decoder
    // that lives for one single decode (hqc.py:694) never pays for the tile kernels' tables, a
    // benchmark never for the row-parallel ones.  What the builders need stays on the host:
    Buf<int> d_tile_tab;  // row descriptors, k_var records, re-laid edge list (d_row_list, d_var_meta, d_csc_list)
    // iteration 1 without its check pass: {first check-to-variable message of a zero-syndrome codeword, row} per position
    // of the re-laid edge list; valid for one (method, alpha of iteration 1) and the current priors / graph
    Buf<int2> d_first_tab;
    // record form of min-sum on the tile kernels: d_rec = per tile a block of rec_tile_floats(m) floats (per row and
    // codeword the two magnitudes with the row's parity in their sign bit, and the arg-min byte), d_mask = per (tile, position of the re-laid edge
    // list) the lane mask "the variable pass's message on this edge is <= 0";
    // d_csc_row = row word of every position of the re-laid edge list (inside d_tile_tab; scaldpc_rec_pack.h)
    Buf<float> d_rec;
    Buf<u64> d_mask;
    int cap_rec_group = 0;
    int *d_csc_row = nullptr, *d_var_rows = nullptr, *d_csr_pos = nullptr;  // views into d_tile_tab
    bool var_reversed = false;  // the column records are laid out heaviest first (column order 2): the degree-1 bucket is at the END
    bool first_valid = false;
    int first_method = -1;
    float first_alpha = 0.0f;
    Buf<int> d_el_tab;  // k_el_var slots and wave info (d_el_slots, d_el_winfo)
    pvec<int> hg_row_ptr, hg_cdeg, hg_col_ptr, hg_csc_edge;
    HostBuckets hg_var, hg_row;
    int stat_el = 0;  // codewords the row-parallel kernels decoded in the last call
    int identity_from = -1;  // n - m if the last m columns of H are I_m (H = [Hin | I]), else -1
    // Set by the first SCALDPC_F_ASYNC call and never cleared: work may be in flight when a later call
    // (or destroy) releases a buffer, so this handle's blocks go back through hipFree (which
    // waits for the device) instead of being parked for immediate reuse.
    bool async_used = false;
    // Set when scaldpc_bp_append_rows failed part-way (an allocation, a copy): host mirrors and device arrays may
    // disagree, so every later call on the handle returns an error instead of decoding on it (check_usable); destroy
    // still frees all.
    bool broken = false;
    // scaldpc_bp_decode_batch_f64 (the reference's ratio-domain float64 arithmetic; kernels in scaldpc_bp_ref64.h):
    // d_ratio = the shared priors as r = p / (1 - p) from h_probs, built on first use (ratio_valid); d_x64 / d_c64 = the two
    // message arrays double [tile][edge][64] of one tile group; d_post64 = the posterior plane double [tile][n][64];
    // d_pratio = a call's per-codeword ratio plane double [tile][prob_cols][64]; d_probs_in64 / d_out_llr64 stage host I/O;
    // d_rem64 = the group's "still running" counters, one per iteration, read through h_rem64
    Buf<double> d_ratio, d_x64, d_c64, d_post64, d_pratio, d_probs_in64, d_out_llr64;
    Buf<int> d_rem64;
    PinnedBuf<int> h_rem64;
    bool ratio_valid = false;
    // Settled codewords (Settle, scaldpc_bp_kernels.h; the rules: scaldpc_bp_sched.h).  d_settle = [tile][SETTLE_WORDS]
    // words of the call's tiles, h_settle their host copy; settle_next = the horizon the next call runs with (0 = it
    // learns), valid for the key below; what the last call did is kept for scaldpc_bp_last_settle.
    Buf<unsigned> d_settle;
    // the sparse gate's tables (Settle: rowf [tile][m], colf [tile][n]); sparse_m / sparse_n / sparse_T = the shape they were
    // last zeroed for (scaldpc_bp_debug_sparse_flags), 0 = the last call did not use them
    Buf<uint4> d_rowf;
    Buf<unsigned> d_colf;
    int sparse_m = 0, sparse_n = 0, sparse_T = 0;
    // the start the next call gates from (settle_sparse_next_start; 0 = the first test), forgotten with settle_next; and
    // the one the last call ran with
    int sparse_start_next = 0, sparse_start = 0;
    PinnedBuf<unsigned> h_settle;
    int settle_next = 0;
    int settle_key_iter = 0, settle_key_soft = 0;
    float settle_key_alpha = -1.0f;
    std::vector<int> settle_frozen_at;  // per tile of the last call, 0 = never froze; empty = the call did not track
    long settle_saved = 0, settle_rerun = 0;
    int settle_K = 0;
    int last_group = 0;  // tiles of the last decoded group (for scaldpc_bp_time_kernels)
    bool last_early = false;  // ... and whether that decode ran with early exit (its variable passes then all write decisions)
    std::mutex mu;
};

namespace {

// one knob from its textual value; false = unknown key or bad value
bool set_knob(Knobs &k, const char *key, const char *val)
{
    if (!key || !val) return false;
    if (!strcmp(key, "path")) {
        if (!strcmp(val, "auto") || !*val) k.path = Knobs::AUTO;
        else if (!strcmp(val, "stream")) k.path = Knobs::STREAM;
        else if (!strcmp(val, "edge")) k.path = Knobs::EDGE;
        else if (!strcmp(val, "lds")) k.path = Knobs::LDS;
        else return false;
        return true;
    }
    char *end = nullptr;
    const double x = strtod(val, &end);
    if (end == val) return false;
    if (!strcmp(key, "split")) k.split = (int)x;
    else if (!strcmp(key, "group_mb")) k.group_mb = x;
    else if (!strcmp(key, "el_max")) k.el_max = (int)x;
    else if (!strcmp(key, "compact_after")) k.compact_after = (int)x;
    else if (!strcmp(key, "first_fused")) k.first_fused = (int)x != 0;
    else if (!strcmp(key, "minsum_rec")) k.minsum_rec = x == 2.0 ? 2 : (int)x != 0;  // (2: wide columns too; else 0 / 1)
    else if (!strcmp(key, "fuse_test")) k.fuse_test = (int)x != 0;
    else if (!strcmp(key, "settle") && x >= -1 && x <= 2) k.settle = (int)x;
    else if (!strcmp(key, "settle_horizon") && x >= 0) k.settle_horizon = (int)x;
    else if (!strcmp(key, "settle_sparse") && x >= -1 && x <= 1) k.settle_sparse = (int)x;
    else return false;
    return true;
}

void knobs_from_env(Knobs &k)
{
    static const char *const names[][2] = {{"SCALDPC_PATH", "path"}, {"SCALDPC_SPLIT", "split"},
                                           {"SCALDPC_GROUP_MB", "group_mb"}, {"SCALDPC_EL_MAX", "el_max"},
                                           {"SCALDPC_COMPACT_AFTER", "compact_after"}, {"SCALDPC_FIRST_FUSED", "first_fused"},
                                           {"SCALDPC_FUSE_TEST", "fuse_test"}, {"SCALDPC_MINSUM_REC", "minsum_rec"},
                                           {"SCALDPC_SETTLE", "settle"}, {"SCALDPC_SETTLE_HORIZON", "settle_horizon"},
                                           {"SCALDPC_SETTLE_SPARSE", "settle_sparse"}};
    for (auto &nm : names)
        if (const char *e = getenv(nm[0])) (void)set_knob(k, nm[1], e);
}

// bucket b holds nodes with bounds[b-1] < deg <= bounds[b]; beyond the last bound -> generic (maxd 0)
void build_buckets(const pvec<int> &deg, const int *bounds, int nb, bool keep_isolated, HostBuckets &out)
{
    // Stable counting sort by degree (ascending node id inside a degree): bucket lists are
    // degree ranges of it, so neighbouring waves of a launch run the same exact-degree code
    // path.  (Decoder construction is on the attack loop's critical path: no per-bucket
    // vectors, no comparison sort.)
    const int n = (int)deg.size();
    int maxdeg = 0;
    for (int d : deg) maxdeg = std::max(maxdeg, d);
    pvec<int> start(maxdeg + 2, 0);
    for (int d : deg) start[d + 1]++;
    for (int d = 0; d <= maxdeg; d++) start[d + 1] += start[d];
    pvec<int> order(n), cursor(start.begin(), start.end() - 1);
    for (int i = 0; i < n; i++) order[cursor[deg[i]]++] = i;
    out.list.clear();
    out.list.reserve(n);
    out.has_generic = false;
    Buckets &bk = out.bk;
    memset(&bk, 0, sizeof bk);
    int lo = keep_isolated ? 0 : 1;  // smallest degree of the bucket being formed
    for (int b = 0; b <= nb && lo <= maxdeg; b++) {
        const int hi = b < nb ? std::min(bounds[b], maxdeg) : maxdeg;  // beyond the last bound: any-degree fallback
        if (hi < lo) continue;
        const int first = start[lo], last = start[hi + 1];
        if (last > first) {
            const int i = bk.nb++;
            bk.maxd[i] = b < nb ? bounds[b] : 0;
            if (b == nb) out.has_generic = true;
            bk.off[i] = (int)out.list.size();
            bk.cnt[i] = last - first;
            bk.blk[i + 1] = bk.blk[i] + (bk.cnt[i] + 3) / 4;
            out.list.insert(out.list.end(), order.begin() + first, order.begin() + last);
        }
        lo = hi + 1;
    }
}

// room for `need` elements with a little headroom: the buffers of a decoder whose graph grows would otherwise be re-made
// at every step
template <typename T, bool P>
int grow(Buf<T, P> &b, size_t need)
{
    return b.ensure(need, need + need / 8);
}

// tiles per group: the in-place message array of a group should stay resident in the
// 256 MiB Infinity Cache (measured knee between 209 and 261 MB, profiles/microbench)
// plane_cols: columns of a soft call's prior plane the group's passes keep reading (256 B per tile and column next to the messages)
int auto_group(const scaldpc_bp *h, int T, int plane_cols = 0)
{
    const double budget = h->kn.group_mb * 1e6;  // default 215: 4 tiles of the HQC-128 bench graph = 208.9 MB, fastest measured; 261 MB falls off
    const double per_tile = ((double)h->E + plane_cols) * TW * sizeof(float);
    const int g = per_tile > 0 ? (int)(budget / per_tile) : T;
    return std::max(1, std::min(g, T));
}

// blocks per tile of a k_parity / k_parity_fin launch over m rows: 4 waves of ROWS_PER_WAVE rows each
int parity_blocks(int m) { return (m + 4 * ROWS_PER_WAVE - 1) / (4 * ROWS_PER_WAVE); }
// waves per tile of such a launch = words per tile of the unsat arrays
int parity_waves(const scaldpc_bp *h) { return 4 * parity_blocks(h->m); }

int ensure_workspace(scaldpc_bp *h, int T, int G, bool want_post, int max_iter, int prob_cols = 0)
{
    if (prob_cols) SC_TRY(grow(h->d_pprior, (size_t)T * prob_cols * TW));
    if (T > h->cap_tiles || h->m > h->ws_m || h->n > h->ws_n) {
        h->d_synd.reset(); h->d_recv.reset(); h->d_hard.reset(); h->d_done.reset();
        h->d_conv.reset(); h->d_unsat.reset(); h->d_iters.reset(); h->d_post.reset();
        T = std::max(T, h->cap_tiles);
        h->cap_tiles = 0;
        // a growing graph gets planes with room for the rows / columns still to come
        const int wm = h->incremental ? h->m + h->m / 2 + 64 : h->m, wn = h->incremental ? h->n + h->n / 2 + 64 : h->n;
        const size_t pw = (size_t)4 * parity_blocks(wm);
        SC_TRY(h->d_synd.ensure((size_t)T * wm));
        SC_TRY(h->d_recv.ensure((size_t)T * wn));
        SC_TRY(h->d_hard.ensure((size_t)T * wn));
        SC_TRY(h->d_done.ensure((size_t)T));
        SC_TRY(h->d_conv.ensure((size_t)T));
        SC_TRY(h->d_unsat.ensure((size_t)T * pw));
        SC_TRY(h->d_iters.ensure((size_t)T * TW));
        h->cap_tiles = T;
        h->ws_m = wm;
        h->ws_n = wn;
    }
    if (want_post) SC_TRY(h->d_post.ensure((size_t)h->cap_tiles * h->ws_n * TW));  // (released above whenever the planes move)
    // (the message arrays are allocated by the path that uses them: ensure_msg / ensure_el)
    // rows of counters: one per tile group of the call, the compact levels' groups (fewer tiles each) included, + row 0
    const int want_rows = ring_rows_wanted(T, G);
    if (max_iter + 2 > h->cap_remaining || want_rows > h->rem.rows) {
        h->d_remaining.reset();
        h->h_remaining.reset();
        h->cap_remaining = 0;
        h->rem.rows = 0;
        const int len = max_iter + 2;
        SC_TRY(h->d_remaining.ensure((size_t)want_rows * (size_t)len));
        SC_TRY(h->h_remaining.ensure((size_t)len));
        h->cap_remaining = len;
        h->rem.rows = want_rows;
    }
    h->rem.slot = h->rem.rows;  // a new call: the first tile group that needs counters zeroes the array
    h->sched.w[SCHED_RING_ROWS] = h->rem.rows;
    return 0;
}

// the next zeroed row of "still running" counters (the row-parallel and small-call paths keep using row 0 with a
// memset of their own; they run between tile groups on the same stream)
// lanes_open: the lanes of the group before are not joined into s yet (decode_level never lets that meet a clear)
int next_remaining_row(scaldpc_bp *h, hipStream_t s, int **row, bool lanes_open)
{
    bool clears = false;
    const int slot = ring_take(h->rem, &clears);
    h->sched.note_take(clears, lanes_open);
    if (clears) SC_HIP(hipMemsetAsync(h->d_remaining, 0, sizeof(int) * (size_t)h->rem.rows * h->cap_remaining, s));
    *row = h->d_remaining + (size_t)slot * h->cap_remaining;
    return 0;
}

// Host staging buffer for table uploads, reused by the thread's later constructions (fresh pages
// for a multi-megabyte vector cost more page-fault time than filling it).  Not cleared.
int *stage_buffer(size_t ints)
{
    struct Staging {
        int *p = nullptr;
        size_t cap = 0;
        ~Staging() { free(p); }
    };
    static thread_local Staging stage;
    if (ints > stage.cap || stage.cap > ((size_t)64 << 20)) {  // (and do not sit on more than 256 MB)
        free(stage.p);
        stage.cap = 0;
        stage.p = (int *)malloc(std::max<size_t>(ints, 1) * sizeof(int));
        if (!stage.p) return nullptr;
        stage.cap = ints;
    }
    return stage.p;
}

int upload_table(Buf<int> &dst, const int *host, size_t ints)
{
    SC_TRY(dst.ensure(ints));
    SC_HIP(hipMemcpy(dst, host, ints * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

// Tables of the 64-codeword-tile kernels: one descriptor per wave of a check launch, one record per
// wave of a k_var launch (descriptor + first edges inline), the edge lists in launch order.
int ensure_tile_tables(scaldpc_bp *h)
{
    if (h->d_tile_tab) return 0;
    const HostBuckets &hv = h->hg_var, &hr = h->hg_row;
    const int *row_ptr = h->hg_row_ptr.data(), *cdeg = h->hg_cdeg.data(), *col_ptr = h->hg_col_ptr.data(),
              *csc_edge = h->hg_csc_edge.data();
    size_t total = 0;
    auto reserve = [&](size_t cnt) {
        const size_t off = total;
        total += (cnt + 63) / 64 * 64;
        return off;
    };
    const size_t o_var_meta = reserve((size_t)4 * VAR_REC * hv.bk.blk[hv.bk.nb] + 4), o_csc_list = reserve((size_t)h->E + 1 + 64);
    const size_t o_row_list = reserve((size_t)16 * hr.bk.blk[hr.bk.nb] + 4);
    const size_t o_csc_row = reserve((size_t)h->E + 1 + 64);
    const size_t o_csr_pos = reserve((size_t)h->E + 64);  // position of every CSR edge in the re-laid list
    const size_t o_var_rows = reserve((size_t)4 * VAR_INLINE * hv.bk.blk[hv.bk.nb] + 4);  // rows of the records' inline edges
    int *host = stage_buffer(total);
    if (!host) return fail(SCALDPC_ENOMEM, "out of host memory");
    // rows whose last edge goes into a column of degree 1 (scaldpc_rec_trim.h): rebuilt with the tables, so a column
    // that appended rows gave a second edge has lost its row's mark by the next decode
    pvec<int> const_last((size_t)h->m);
    rec_mark_const_last(h->m, h->n, row_ptr, col_ptr, csc_edge, const_last.data());
    for (int b = 0; b < hr.bk.nb; b++) {
        const int blocks = hr.bk.blk[b + 1] - hr.bk.blk[b];
        for (int sl = 0; sl < blocks * 4; sl++) {
            int *md = host + o_row_list + 4 * ((size_t)hr.bk.blk[b] * 4 + sl);
            const bool pad = sl >= hr.bk.cnt[b];
            const int r = pad ? -1 : hr.list[hr.bk.off[b] + sl];
            md[0] = r;
            md[1] = pad ? 0 : row_ptr[r];
            md[2] = pad ? 0 : row_ptr[r + 1] - row_ptr[r];
            md[3] = rec_desc_word(hr.bk.maxd[b], pad ? 0 : const_last[r]);  // (k_check_tanh asks "== 0": any-degree rows stay 0)
        }
    }
    int *meta = host + o_var_meta, *relaid = host + o_csc_list, *relaid_row = host + o_csc_row;
    int pos = 0;
    pvec<int> edge_row((size_t)h->E);
    for (int r = 0; r < h->m; r++)
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; e++) edge_row[e] = r;
    // launch order of the columns: the bucket lists are sorted by degree, ascending column id inside a
    // degree.  Order bit 0 re-sorts each run of equal degree by the column's FIRST edge id, so that
    // neighbouring waves of a launch start their gathers in neighbouring rows of the message array
    // (the records carry the column id, so the order is free; results cannot depend on it).
    pvec<int> order_buf;
    const int *vlist = hv.list.data();
    // A tile group that runs as ONE stream lane (a tile too large to share the cache with a second one:
    // the HQC-256 graph) has nothing to fill the tail of its launches with, so its heaviest columns go first (bit 1)
    // (measured 321.5 -> 315.5 ms per step, k_var 51.5 -> 49.9 us); with two lanes the other lane's kernel
    // lives in that tail and the same order costs 0.8 % (HQC-128: 95.2 -> 96.0 ms): there the columns of a
    // degree are ordered by their first edge instead (profiles/r02/ab_*order*.json)
    const bool single_lane = auto_group(h, 1 << 20) < 2 || h->kn.split < 2;
    const int order = single_lane ? 2 : 1;
    if ((order & 1) && !hv.list.empty()) {
        order_buf = hv.list;
        size_t i = 0;
        while (i < order_buf.size()) {
            size_t j = i;
            while (j < order_buf.size() && cdeg[order_buf[j]] == cdeg[order_buf[i]]) j++;
            if (cdeg[order_buf[i]] > 0)
                std::sort(order_buf.begin() + i, order_buf.begin() + j,
                          [&](int a, int b2) { return csc_edge[col_ptr[a]] < csc_edge[col_ptr[b2]]; });
            i = j;
        }
        vlist = order_buf.data();
    }
    for (int b = 0; b < hv.bk.nb; b++) {
        const int blocks = hv.bk.blk[b + 1] - hv.bk.blk[b];
        for (int sl = 0; sl < blocks * 4; sl++) {
            int *md = meta + (size_t)VAR_REC * ((size_t)hv.bk.blk[b] * 4 + sl);
            int *mr = host + o_var_rows + (size_t)VAR_INLINE * ((size_t)hv.bk.blk[b] * 4 + sl);
            if (sl >= hv.bk.cnt[b]) {
                md[0] = -1;
                for (int k = 1; k < VAR_REC; k++) md[k] = 0;
                for (int k = 0; k < VAR_INLINE; k++) mr[k] = 0;
                continue;
            }
            const int v = vlist[hv.bk.off[b] + sl], d = cdeg[v];
            md[0] = v;
            md[1] = pos;
            md[2] = d;
            md[3] = hv.bk.maxd[b];
            for (int k = 0; k < d; k++) {
                relaid[pos + k] = csc_edge[(size_t)col_ptr[v] + k];
                const int e = relaid[pos + k], r = edge_row[e];
                // (the row word of the record form: row | index in the row << 24; a graph it cannot hold never runs
                // that form -- rec_form() -- and nothing else reads these tables)
                relaid_row[pos + k] = rec_pack_row(rec_row_of(r), (e - row_ptr[r]) & (REC_MAX_ROW_DEG - 1));
                host[o_csr_pos + relaid[pos + k]] = pos + k;
            }
            for (int k = 0; k < VAR_INLINE; k++) md[4 + k] = k < d ? relaid[pos + k] : 0;
            for (int k = 0; k < VAR_INLINE; k++) mr[k] = k < d ? relaid_row[pos + k] : 0;
            pos += d;
        }
    }
    h->var_reversed = (order & 2) != 0;
    if (order & 2) {
        // heaviest columns FIRST: the waves that start last are then the cheapest ones (degree-1 identity
        // columns), which shortens the tail of the launch (longest-processing-time-first)
        const size_t nrec = (size_t)4 * hv.bk.blk[hv.bk.nb];
        int *rows = host + o_var_rows;
        for (size_t i = 0, j = nrec ? nrec - 1 : 0; i < j; i++, j--) {
            std::swap_ranges(meta + i * VAR_REC, meta + (i + 1) * VAR_REC, meta + j * VAR_REC);
            std::swap_ranges(rows + i * VAR_INLINE, rows + (i + 1) * VAR_INLINE, rows + j * VAR_INLINE);
        }
    }
    SC_TRY(upload_table(h->d_tile_tab, host, total));
    h->first_valid = false;  // (first_tab follows the re-laid edge list)
    h->d_var_meta = h->d_tile_tab + o_var_meta;
    h->d_csc_list = h->d_tile_tab + o_csc_list;
    h->d_row_list = h->d_tile_tab + o_row_list;
    h->d_csc_row = h->d_tile_tab + o_csc_row;
    h->d_var_rows = h->d_tile_tab + o_var_rows;
    h->d_csr_pos = h->d_tile_tab + o_csr_pos;
    return 0;
}

// ---- tables of the row-parallel path (k_el_var) ------------------------------------------------
// d_el_tab = [slots: 2 ints per lane slot][slot_col: 1 int per lane slot] for el_cap_bins bins of 64
// lane slots; h_el mirrors it on the host.
inline int el_tag(int start, int pos, int cap, bool live) { return start | (pos << 6) | ((cap - 1) << 12) | ((live ? 1 : 0) << 18); }
inline size_t el_col_off(const scaldpc_bp *h) { return (size_t)128 * h->el_cap_bins; }

// free lanes a column's segment gets on top of its degree: none on a decoder whose graph is fixed
// (and for the degree-1 columns of an identity block, which never grow); a few on one that grows
int el_slack(const scaldpc_bp *h, int col, int deg)
{
    if (!h->incremental) return 0;
    if (h->identity_from >= 0 && col >= h->identity_from) return 0;
    return 2 + deg / 4;
}

// hands out `cap` neighbouring lanes (a segment never wraps around a bin); returns bin * 64 + start.
// The host mirrors grow with the bins (dead lanes: no edge, not live); the device table is
// re-uploaded by the caller when the bins outgrow el_cap_bins.
int el_alloc_segment(scaldpc_bp *h, int cap)
{
    if (h->el_waves == 0 || h->el_open_used + cap > 64) {
        h->el_waves++;
        h->el_open_used = 0;
        if (h->h_el_col.size() < (size_t)64 * h->el_waves) {
            const size_t lanes = (size_t)64 * (h->el_waves + h->el_waves / 2 + 16), old = h->h_el_col.size();
            h->h_el_slots.resize(2 * lanes, 0);
            h->h_el_col.resize(lanes, 0);
            for (size_t i = old; i < lanes; i++) h->h_el_slots[2 * i] = -1;
        }
    }
    const int slot = (h->el_waves - 1) * 64 + h->el_open_used;
    h->el_open_used += cap;
    return slot;
}

// device copy of the mirrors: [slots: 2 ints per lane][slot_col: 1 int per lane] for el_cap_bins bins.
// EVERY lane of the table is initialised (bins not yet in use hold dead lanes): an append that opens a
// new bin only sends the words it changes, and a launch covers whole bins.
int el_upload(scaldpc_bp *h)
{
    h->d_el_tab.reset();
    h->el_cap_bins = h->incremental ? h->el_waves + h->el_waves / 2 + 64 : h->el_waves;
    const size_t lanes = (size_t)64 * h->el_cap_bins, old = h->h_el_col.size();
    h->h_el_slots.resize(2 * lanes, 0);
    h->h_el_col.resize(lanes, 0);
    for (size_t i = old; i < lanes; i++) h->h_el_slots[2 * i] = -1;
    SC_TRY(h->d_el_tab.ensure(3 * lanes));
    h->d_el_slots = h->d_el_tab;
    h->d_el_slot_col = h->d_el_tab + el_col_off(h);
    if (lanes) {
        SC_HIP(hipMemcpy(h->d_el_slots, h->h_el_slots.data(), 2 * lanes * sizeof(int), hipMemcpyHostToDevice));
        SC_HIP(hipMemcpy(h->d_el_slot_col, h->h_el_col.data(), lanes * sizeof(int), hipMemcpyHostToDevice));
    }
    return 0;
}

// (re)builds host mirrors + device table from the host graph mirror: columns in degree order (hg_var.list)
int refresh_full(scaldpc_bp *h);
int ensure_el_tables(scaldpc_bp *h)
{
    if (h->d_el_tab || !h->el_ok) return 0;
    SC_TRY(refresh_full(h));  // built from the host's CSC mirror: bring it up to date with appended rows first
    const HostBuckets &hv = h->hg_var;
    const int *cdeg = h->hg_cdeg.data(), *col_ptr = h->hg_col_ptr.data(), *csc_edge = h->hg_csc_edge.data();
    h->seg_slot.assign(h->n, -1);
    h->seg_cap.assign(h->n, 0);
    h->el_waves = 0;
    h->el_open_used = 0;
    h->h_el_slots.clear();
    h->h_el_col.clear();
    for (size_t i = 0; i < hv.list.size(); i++) {
        const int v = hv.list[i], d = cdeg[v];
        const int cap = std::min(64, std::max(d, 1) + el_slack(h, v, d));
        const int s0 = el_alloc_segment(h, cap), start = s0 & 63;
        h->seg_slot[v] = s0;
        h->seg_cap[v] = (unsigned char)cap;
        const int *ce = csc_edge + col_ptr[v];
        for (int k = 0; k < cap; k++) {
            h->h_el_slots[2 * (size_t)(s0 + k)] = k < d ? ce[k] : -1;
            h->h_el_slots[2 * (size_t)(s0 + k) + 1] = el_tag(start, k, cap, true);
        }
        h->h_el_col[s0] = v;
    }
    return el_upload(h);
}

// Min-sum in its record form (k_check_minsum_rec / k_var_rec)?  Rows and columns that live in registers, the
// exact-degree check kernels, the scalar-id variable kernel.
bool rec_form(const scaldpc_bp *h, int method)
{
    // (columns of 33-64 edges: message form -- the exact-degree variable pass is compiled up to 32 -- unless minsum_rec
    // is 2: then a second launch takes them, k_var<64, ..> in its record mode over the (32, 64] bucket, launch_var)
    // (and the variable pass's row words hold 24 bits of row beside the edge's index in it: rec_rows_fit)
    const int col_cap = h->kn.minsum_rec == 2 ? 64 : 32;
    return method == SCALDPC_BP_MIN_SUM && h->kn.minsum_rec && h->E > 0 && h->max_row_deg <= 64 && h->max_col_deg <= col_cap &&
           !h->hg_var.has_generic && rec_rows_fit(h->m, h->max_row_deg);
}

// message array of the tile path, G tiles (and the records of the min-sum record form)
int ensure_msg(scaldpc_bp *h, int G, int method)
{
    SC_TRY(ensure_tile_tables(h));
    if (rec_form(h, method) && G > h->cap_rec_group) {  // (append_rows resets cap_rec_group too)
        h->d_rec.reset(); h->d_mask.reset();
        h->cap_rec_group = 0;
        SC_TRY(h->d_rec.ensure((size_t)G * rec_tile_floats(h->m)));
        SC_TRY(h->d_mask.ensure((size_t)G * h->E));
        h->cap_rec_group = G;
    }
    if (G > h->cap_group) {  // (append_rows resets cap_group: the arrays are sized by E)
        h->d_msg.reset(); h->d_scratch.reset();
        h->cap_group = 0;
        SC_TRY(h->d_msg.ensure((size_t)G * h->E * TW));
        if (h->need_scratch) SC_TRY(h->d_scratch.ensure((size_t)G * h->E * TW));
        h->cap_group = G;
    }
    return 0;
}

// message + prefix arrays of the row-parallel path, nb codewords
int ensure_el(scaldpc_bp *h, int nb)
{
    SC_TRY(ensure_el_tables(h));
    const size_t need = (size_t)nb * h->E;
    return h->d_emsg.ensure(need, h->incremental ? need + need / 4 : need);  // room for the edges still to come
}

// How many codewords the row-parallel kernels take (0 = none: use 64-codeword tiles).
// Their cost grows with the codeword count (12 us per iteration for one codeword, +3.7 us per
// further one with min-sum, 16 / +6.5 us with the tanh rule, HQC-128 bench graph), a tile's
// does not (40 / 43 us): the default limit is where the two meet
// (profiles/microbench/small_batch_latency.py).  SCALDPC_PATH=edge lifts the limit to a whole
// tile, SCALDPC_PATH=stream disables the path (tests pin either).
int el_limit(const scaldpc_bp *h, int method)
{
    if (!h->el_ok) return 0;  // empty graph, or a row / column wider than a wave
    int lim = method == SCALDPC_BP_MIN_SUM ? 6 : 4;
    if (h->kn.el_max >= 0) lim = h->kn.el_max;
    if (h->kn.path == Knobs::STREAM) lim = 0;
    if (h->kn.path == Knobs::EDGE) lim = TW;
    return std::max(0, std::min(lim, TW));
}

#define LAUNCH_CHECK() SC_HIP(hipGetLastError())

// One decode call, from its entry point (begin_call) down to the launches.  A compact level runs on a copy with its own
// batch and T.
struct DecodeCall {
    hipStream_t s = nullptr;
    int batch = 0, T = 0, G = 0, max_iter = 0, method = 0;  // codewords, tiles of 64 of them, tiles per cache-resident group
    float alpha = 0.0f;
    bool early = false, want_post = false;
    bool state_ready = false;  // the call's state planes and counters are already reset (k_small_prepare): nothing below resets them
    bool no_sync = false;      // this call may not synchronise (SCALDPC_F_ASYNC): settled codewords by device-side skipping only
};

// The state planes of a call's (or a compact level's) tiles.
struct TileState {
    const u64 *synd;
    u64 *hard, *done, *conv, *unsat;
    int *iters;
    float *post;
    // a soft call: prior LLRs per codeword for the columns [first_col, n), float [tile][n - first_col][64] (null: shared priors)
    const float *pprior = nullptr;
    int first_col = 0;
    // the same planes from tile `ta` on -- what a launch whose first tile is ta works on (null stays null)
    TileState at(const scaldpc_bp *h, int ta) const
    {
        const size_t t = (size_t)ta;
        return TileState{synd + t * h->m, hard + t * h->n, done + t, conv + t, unsat + t * parity_waves(h), iters + t * TW,
                         post ? post + t * h->n * TW : nullptr, pprior ? pprior + t * (h->n - first_col) * TW : nullptr, first_col};
    }
};
// the convergence test of iteration `it` on a view's tiles; *remaining counts who still runs after it; latch = early exit
FusedTest fused_test(const scaldpc_bp *h, const TileState &tv, int *remaining, int it, bool latch)
{
    return FusedTest{tv.hard, tv.unsat, tv.done, tv.conv, tv.iters, remaining, h->n, parity_waves(h), it, latch ? 1 : 0};
}

// Compile-time dispatch of the launches.  with_cap<16, 32, 64>(deg, f) calls f(std::integral_constant<int, CAP>) with the
// first CAP of the ladder that holds a node degree `deg` (the last CAP takes anything wider: the kernels' any-degree
// fallback); every kernel is instantiated for exactly the ladder its launch names.  with_bool / with_method hand f a
// runtime bool / update rule as a compile-time one; with_prior hands it the prior source of the call as a type (a value of
// it, for decltype) with the kernel argument that goes with it: plane non-null = a soft call, SoftPrior over the plane (of
// the launch's first tile) for the columns from first_col on; else SharedPrior and the handle's priors.  with_first_prior is
// for the check kernels, whose FIRST pass alone reads priors, on the tiles of a view: f(FIRST, source, argument), and
// FIRST = false comes with SharedPrior only -- no <.., false, .., SoftPrior> instantiation.
template <int CAP, int... WIDER, typename F>
void with_cap(int deg, F &&f)
{
    if constexpr (sizeof...(WIDER) == 0)
        f(std::integral_constant<int, CAP>{});
    else if (deg <= CAP)
        f(std::integral_constant<int, CAP>{});
    else
        with_cap<WIDER...>(deg, f);
}
template <typename F>
void with_bool(bool b, F &&f)
{
    if (b) f(std::true_type{}); else f(std::false_type{});
}
template <typename F>
void with_method(int method, F &&f)
{
    if (method == SCALDPC_BP_MIN_SUM) f(std::integral_constant<int, SCALDPC_BP_MIN_SUM>{});
    else f(std::integral_constant<int, SCALDPC_BP_PRODUCT_SUM>{});
}
template <typename F>
void with_prior(const scaldpc_bp *h, const float *plane, int first_col, F &&f)
{
    plane ? f(SoftPrior{}, SoftPrior{h->d_prior, plane, first_col, h->n - first_col}) : f(SharedPrior{}, (const float *)h->d_prior);
}
template <typename F>
void with_first_prior(const scaldpc_bp *h, bool first, const TileState &tv, F &&f)
{
    if (first)
        with_prior(h, tv.pprior, tv.first_col, [&](auto P, auto prior) { f(std::true_type{}, P, prior); });
    else
        f(std::false_type{}, SharedPrior{}, (const float *)h->d_prior);
}

// No message initialisation pass: the first check update reads the priors (v2c = prior of the
// edge's column by definition).  The tanh rule's any-degree fallback (rows wider than 64) keeps it.
bool fused_init(const scaldpc_bp *h, int method)
{
    return h->E > 0 && (method == SCALDPC_BP_MIN_SUM || h->max_row_deg <= ROW_CAP);
}

// Which check kernels can carry the convergence test of the previous iteration (fused_test)?  The register-resident
// ones: the tanh kernel always, min-sum in its exact-degree form.
bool check_can_test(const scaldpc_bp *h, int method)
{
    if (h->E == 0) return false;
    if (method == SCALDPC_BP_MIN_SUM) return h->max_row_deg <= ROW_CAP;
    return true;
}

// One check pass over G tiles.
struct CheckPass {
    float alpha = 0.0f;
    // The first check pass of these tiles in a call -- iteration 1 with first_fused off, or of a soft call: the only one that
    // reads priors (a soft call's per codeword, from the view), and in min-sum it writes MESSAGES whatever the form, followed
    // by the message form's variable pass -- the records start with iteration 2.
    bool first = false;
    int tile0 = 0;  // first tile of the launch inside the group's message / record arrays
    FusedTest test{};  // hard non-null = the pass also runs the test of the iteration before (check_can_test, never `first`)
    // The first record-form pass of these tiles in a call: the sign masks a k_var_rec would have left are not there yet
    // (the messages come from k_var_first / k_var), so this pass writes them too.
    bool boot = false;
    Settle settle{};  // settled codewords (record-form passes of a fixed-iteration call); the default = off
};
int launch_check(scaldpc_bp *h, const TileState &tv, int G, int method, int skip_done, hipStream_t s, const CheckPass &p)
{
    if (h->E == 0) return 0;
    float *const msg0 = h->d_msg + (size_t)p.tile0 * h->E * TW;
    float *const scr0 = h->d_scratch ? h->d_scratch + (size_t)p.tile0 * h->E * TW : nullptr;
    const dim3 grid(h->row_bk.blk[h->row_bk.nb], G), block(256);  // one wave per row descriptor
    const bool test = p.test.hard && !p.first;
    if (method != SCALDPC_BP_MIN_SUM) {  // (first: fused_init holds, so the rows are register-resident)
        with_cap<16, 32, 64>(h->max_row_deg, [&](auto cap) {
            if (test)
                hipLaunchKernelGGL((k_check_tanh<cap, false, true, SharedPrior>), grid, block, 0, s, h->d_row_list, msg0, scr0, tv.synd,
                                   tv.done, skip_done, h->m, h->E, h->d_col_idx, h->d_prior, p.test);
            else
                with_first_prior(h, p.first, tv, [&](auto fst, auto P, auto prior) {
                    hipLaunchKernelGGL((k_check_tanh<cap, fst, false, decltype(P)>), grid, block, 0, s, h->d_row_list, msg0, scr0,
                                       tv.synd, tv.done, skip_done, h->m, h->E, h->d_col_idx, prior, FusedTest{});
                });
        });
    } else if (rec_form(h, method) && !p.first) {
        float *const rec0 = h->d_rec + (size_t)p.tile0 * rec_tile_floats(h->m);
        u64 *const mask0 = h->d_mask + (size_t)p.tile0 * h->E;
        // the constant last edge of a marked row is read from the shared priors as they are NOW (set_channel_probs on a live
        // decoder needs no rebuild); a soft call's columns of degree 1 may carry per-codeword priors: no constant there
        const float *const cprior = tv.pprior ? nullptr : h->d_prior;
        with_cap<16, 32, 64>(h->max_row_deg, [&](auto cap) {
            with_bool(p.boot, [&](auto bt) {
                with_bool(test, [&](auto par) {
                    hipLaunchKernelGGL((k_check_minsum_rec<cap, bt, par>), grid, block, 0, s, h->d_row_list, msg0, tv.synd, tv.done,
                                       skip_done, h->m, h->E, p.alpha, h->d_col_idx, rec0, mask0, h->d_csr_pos, cprior, p.test, p.settle);
                });
            });
        });
    } else if (h->max_row_deg <= ROW_CAP) {
        with_cap<16, 32, 64>(h->max_row_deg, [&](auto cap) {
            if (test)
                hipLaunchKernelGGL((k_check_minsum_x<cap, false, true, SharedPrior>), grid, block, 0, s, h->d_row_list, msg0, tv.synd,
                                   tv.done, skip_done, h->m, h->E, p.alpha, h->d_col_idx, h->d_prior, p.test);
            else
                with_first_prior(h, p.first, tv, [&](auto fst, auto P, auto prior) {
                    hipLaunchKernelGGL((k_check_minsum_x<cap, fst, false, decltype(P)>), grid, block, 0, s, h->d_row_list, msg0,
                                       tv.synd, tv.done, skip_done, h->m, h->E, p.alpha, h->d_col_idx, prior, FusedTest{});
                });
        });
    } else {  // a row wider than 64: the loop form
        with_first_prior(h, p.first, tv, [&](auto fst, auto P, auto prior) {
            hipLaunchKernelGGL((k_check_minsum<fst, decltype(P)>), dim3((h->m + 3) / 4, G), block, 0, s, h->d_row_ptr, msg0, tv.synd,
                               tv.done, skip_done, h->m, h->E, p.alpha, h->d_col_idx, prior);
        });
    }
    LAUNCH_CHECK();
    return 0;
}

// Can iteration 1 run without its check pass (k_var_first)?  The first messages come from the row-parallel check
// kernel (rows of at most 64 edges), the first variable pass keeps every column in registers (columns of at most 64).
bool first_fusable(const scaldpc_bp *h, int method)
{
    return h->kn.first_fused && fused_init(h, method) && h->E > 0 && h->max_row_deg <= 64 && h->max_col_deg <= 64 &&
           !h->hg_var.has_generic;
}

// first_tab for (method, alpha of iteration 1) and the current priors: the row-parallel check kernel decodes the first
// pass of ONE codeword with an all-zero syndrome into a scratch array (its values are the tile kernels' own, bit for
// bit), k_first_tab lays them out beside each edge's row in the order of the re-laid edge list.
int ensure_first_table(scaldpc_bp *h, int method, float alpha1, hipStream_t s)
{
    if (h->first_valid && h->first_method == method && h->first_alpha == alpha1) return 0;
    h->first_valid = false;  // (until the new table is complete)
    SC_TRY(grow(h->d_first_tab, (size_t)h->E + 128));  // (a column's scalar loads may run past its last edge, as in the edge list)
    Buf<u64> zero;  // (declared first: released after tmp)
    Buf<float> tmp;
    SC_TRY(tmp.ensure((size_t)h->E));
    SC_TRY(zero.ensure((size_t)h->m + 1));
    hipError_t e = hipMemsetAsync(zero, 0, sizeof(u64) * ((size_t)h->m + 1), s);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_first_tab, 0, sizeof(int2) * h->d_first_tab.cap(), s);
    if (e == hipSuccess) {
        with_method(method, [&](auto M) {
            hipLaunchKernelGGL((k_el_check<M, true, SharedPrior>), dim3((h->m + 3) / 4, 1), dim3(256), 0, s, h->d_row_ptr, h->d_col_idx,
                               h->d_prior, tmp, zero, zero + h->m, 0, h->m, h->E, alpha1, (const u64 *)nullptr, (int *)nullptr);
        });
        hipLaunchKernelGGL(k_first_tab, dim3((unsigned)((h->E + 255) / 256)), dim3(256), 0, s, h->d_csc_list, tmp, h->d_row_ptr, h->m,
                           h->E, h->d_first_tab);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // tmp / zero go back to the allocator on return
    if (e != hipSuccess) return fail(SCALDPC_EHIP, "first-message table: %s", hipGetErrorString(e));
    h->first_valid = true;
    h->first_method = method;
    h->first_alpha = alpha1;
    return 0;
}

// One variable pass over G tiles.
struct VarPass {
    int write_out = 0;  // also emit the decisions (merged under the done mask) and, where the view has a plane for them, the posteriors
    int tile0 = 0;      // first tile of the launch inside the group's message / record arrays
    // Iteration 1 without its check pass (k_var_first, from the first-message table and the view's syndrome planes;
    // ensure_first_table first).  Never in a soft call: the table is a function of shared priors.
    bool first_synd = false;
    bool rec = false;    // the check pass left records, not messages (rec_form)
    bool light = false;  // a pass after iteration 1: without output, the record form leaves the degree-1 bucket out (rec_var_slices)
    // No check pass follows this one on these tiles (the last iteration of a decode, always with write_out): the record form
    // then runs its store-free instantiation, which leaves messages and sign masks as the pass before left them.
    bool final_pass = false;
    // A record-form pass without output still merges its columns' decisions into the view's hard planes, from the sum it has
    // anyway (settled codewords: the closing pass of a frozen tile then finds them there, k_var_rec).  It stays slim.
    bool keep_hard = false;
    Settle settle{};  // settled codewords; the default = off
};
int launch_var(scaldpc_bp *h, const TileState &tv, int G, int skip_done, hipStream_t s, const VarPass &p)
{
    float *const msg0 = h->d_msg + (size_t)p.tile0 * h->E * TW;
    float *const scr0 = h->d_scratch ? h->d_scratch + (size_t)p.tile0 * h->E * TW : nullptr;
    const Buckets &bk = h->var_bk;
    const int nblk = bk.blk[bk.nb];
    if (p.first_synd) {
        const int nrec = 4 * nblk;  // one record per wave of a plain k_var launch; two per wave here
        const dim3 grid2((unsigned)((nrec + 7) / 8), G);
        with_cap<16, 32, 64>(h->max_col_deg, [&](auto cap) {
            hipLaunchKernelGGL((k_var_first<cap>), grid2, dim3(256), 0, s, h->d_var_meta, h->d_csc_list, h->d_prior, msg0, tv.post,
                               tv.hard, tv.done, skip_done, h->n, h->E, p.write_out, (const int2 *)h->d_first_tab, tv.synd, h->m, nrec);
        });
    } else if (p.rec) {
        // k_var_rec on the narrow slice of the column records, k_var<64, ..> in its record mode on the wide one (rec_var_slices)
        const RecVarSlices sl = rec_var_slices(bk.nb, bk.maxd, bk.blk, h->var_reversed, p.light, p.write_out != 0, G, h->max_col_deg);
        const int out = (p.write_out || p.keep_hard) ? 1 : 0;
        float *const rec0 = h->d_rec + (size_t)p.tile0 * rec_tile_floats(h->m);
        u64 *const mask0 = h->d_mask + (size_t)p.tile0 * h->E;
        const bool fin_pass = p.final_pass && p.write_out;
        if (sl.narrow_n > 0)
            with_cap<16, 32>(sl.narrow_deg, [&](auto cap) {
                with_prior(h, tv.pprior, tv.first_col, [&](auto P, auto prior) {
                    with_bool(fin_pass, [&](auto fin) {
                        hipLaunchKernelGGL((k_var_rec<cap, decltype(P), fin>), dim3((unsigned)sl.narrow_grid, G), dim3(256), 0, s,
                                           h->d_var_meta, h->d_var_rows, h->d_csc_list, h->d_csc_row, prior, msg0, rec0, mask0, tv.post,
                                           tv.hard, tv.done, skip_done, h->n, h->m, h->E, out, sl.narrow0, sl.xmap ? sl.narrow_n : 0,
                                           p.settle);
                    });
                });
            });
        if (sl.wide_n > 0) {
            // (var_rows, csc_row, rec, sgn, m, blk0, xmap, last, stl)
            const RecWide rw{h->d_var_rows, h->d_csc_row, rec0, mask0, h->m, sl.wide0, sl.xmap ? sl.wide_n : 0, fin_pass, p.settle};
            with_prior(h, tv.pprior, tv.first_col, [&](auto P, auto prior) {
                hipLaunchKernelGGL((k_var<64, decltype(P)>), dim3((unsigned)sl.wide_grid, G), dim3(256), 0, s, h->d_var_meta,
                                   h->d_csc_list, prior, msg0, scr0, tv.post, tv.hard, tv.done, skip_done, h->n, h->E, out, rw);
            });
        }
    } else {
        with_cap<16, 32, 64>(h->max_col_deg, [&](auto cap) {
            with_prior(h, tv.pprior, tv.first_col, [&](auto P, auto prior) {
                hipLaunchKernelGGL((k_var<cap, decltype(P)>), dim3(nblk, G), dim3(256), 0, s, h->d_var_meta, h->d_csc_list, prior, msg0,
                                   scr0, tv.post, tv.hard, tv.done, skip_done, h->n, h->E, p.write_out, RecWide{});
            });
        });
    }
    LAUNCH_CHECK();
    return 0;
}

// The row-parallel pair on the nb codewords of a view.  hard_g non-null (early exit): the check pass also tests H e == s on
// the decisions of the iteration before and leaves the verdicts in unsat_prev ...
int launch_el_check(scaldpc_bp *h, const TileState &tv, int nb, int method, float alpha, int skip_done, hipStream_t s, bool first,
                    const u64 *hard_g, int *unsat_prev)
{
    with_method(method, [&](auto M) {
        with_first_prior(h, first, tv, [&](auto fst, auto P, auto prior) {
            hipLaunchKernelGGL((k_el_check<M, fst, decltype(P)>), dim3((h->m + 3) / 4, nb), dim3(256), 0, s, h->d_row_ptr,
                               h->d_col_idx, prior, h->d_emsg, tv.synd, tv.done, skip_done, h->m, h->E, alpha, hard_g, unsat_prev);
        });
    });
    LAUNCH_CHECK();
    return 0;
}
// ... and with remaining_prev non-null (early exit) the variable pass first latches the codewords that passed the test of
// iteration it_prev, and counts the others there.
int launch_el_var(scaldpc_bp *h, const TileState &tv, int nb, int skip_done, int write_out, hipStream_t s, const int *unsat_prev,
                  int it_prev, int *remaining_prev)
{
    // grid.x a multiple of 8: block x lands on the same XCD for every codeword row, so an XCD's L2
    // keeps its share of the slot table
    const unsigned gx = (unsigned)(((h->el_waves + 3) / 4 + 7) / 8 * 8);
    with_prior(h, tv.pprior, tv.first_col, [&](auto P, auto prior) {
        hipLaunchKernelGGL((k_el_var<decltype(P)>), dim3(gx, nb), dim3(256), 0, s, (const int2 *)h->d_el_slots, h->d_el_slot_col,
                           h->el_waves, prior, h->d_emsg, tv.post, tv.hard, tv.done, skip_done, h->E, write_out, unsat_prev, it_prev,
                           remaining_prev ? tv.conv : nullptr, remaining_prev ? tv.iters : nullptr, remaining_prev);
    });
    LAUNCH_CHECK();
    return 0;
}

// syndrome planes of T tiles: synd = H x (k_parity without the convergence test)
int launch_syndrome(const scaldpc_bp *h, const u64 *x, u64 *synd, int T, hipStream_t s)
{
    hipLaunchKernelGGL(k_parity<false>, dim3(parity_blocks(h->m), T), dim3(256), 0, s, h->d_row_ptr, h->d_col_idx, x, h->m, h->n,
                       synd, (u64 *)nullptr, (const u64 *)nullptr);
    LAUNCH_CHECK();
    return 0;
}

// The LDS-resident single-launch decoder (k_bp_small): LDS bytes of a launch on this graph ...
size_t small_lds_bytes(const scaldpc_bp *h) { return (size_t)2 * h->E * sizeof(float) + (size_t)2 * h->n + h->m + 64; }
// ... and whether a call takes it: those bytes, or 0 = another path (the graph does not fit, or "stream" / "edge" pin one)
size_t small_lds(const scaldpc_bp *h)
{
    const size_t lds = small_lds_bytes(h);
    const bool fits = h->E > 0 && lds <= 60 * 1024;
    return fits && h->kn.path != Knobs::STREAM && h->kn.path != Knobs::EDGE ? lds : 0;
}

// k_bp_small over `batch` codewords, one workgroup each.  PLANES: input syndromes and outputs are the tile path's bit
// planes (Monte-Carlo entry points); else bytes per codeword in the caller's layout.  pprior non-null = per-codeword priors
// (scaldpc_bp_decode_batch_soft; with PLANES, scaldpc_mc_hqc_run_soft).
template <bool PLANES>
int launch_small(scaldpc_bp *h, size_t lds, int method, int batch, const void *in, int input_kind, int max_iter, float alpha,
                 bool early, void *bits, float *llr, int *iters, void *conv, hipStream_t s, const float *pprior = nullptr,
                 int first_col = 0)
{
    with_method(method, [&](auto M) {
        auto launch = [&](auto P, auto prior) {
            hipLaunchKernelGGL((k_bp_small<M, PLANES, decltype(P)>), dim3(batch), dim3(256), lds, s, h->d_row_ptr, h->d_col_idx,
                               h->d_col_ptr, h->d_csc_edge, prior, h->m, h->n, (int)h->E, in, input_kind, max_iter, alpha,
                               early ? 1 : 0, bits, llr, iters, conv);
        };
        with_prior(h, pprior, first_col, launch);
    });
    LAUNCH_CHECK();
    return 0;
}

float alpha_for(float alpha, int it)
{
    // ms_scaling_factor == 0 -> 1 - 2^-iter
    return alpha == 0.0f ? (float)(1.0 - std::pow(2.0, -1.0 * it)) : alpha;
}

int ensure_el_unsat(scaldpc_bp *h, int max_iter) { return h->d_el_unsat.ensure(((size_t)max_iter + 2) * TW); }

// All iterations of the row-parallel kernels on the nb codewords of `st` (ONE tile: a handful of codewords, el_limit),
// two launches per iteration.  With early exit check(it) also tests H e == s on the decisions of iteration it-1, and
// var(it) latches the codewords that passed (frozen at it-1) before it updates the others.  The last iteration is
// followed by the ordinary k_parity / k_finalize pair (latching only with early exit).  The host looks at "still running
// after it-1" one iteration late, so a finished call enqueues one iteration of (skipped) launches more than a loop with
// the test as launches of its own -- and half as many launches overall.
int iterate_el(scaldpc_bp *h, const DecodeCall &c, const TileState &st, int nb)
{
    const hipStream_t s = c.s;
    const bool early = c.early;
    const int max_iter = c.max_iter, skip = early ? 1 : 0;
    if (early) {
        SC_TRY(ensure_el_unsat(h, max_iter));
        if (!c.state_ready) {  // (else k_small_prepare has zeroed both)
            SC_HIP(hipMemsetAsync(h->d_el_unsat, 0, sizeof(int) * ((size_t)max_iter + 2) * TW, s));
            SC_HIP(hipMemsetAsync(h->d_remaining, 0, sizeof(int) * ((size_t)max_iter + 2), s));
        }
    }
    static_assert(ROW_CAP == TW, "el_ok (a row = at most one wave of edge lanes) must imply fused_init's rows <= ROW_CAP");
    // No initialisation pass: el_ok holds here (el_limit), i.e. a non-empty graph with no row wider than ROW_CAP, so
    // fused_init does for either rule -- the first check pass reads the priors.
    for (int it = 1; it <= max_iter; it++) {
        const bool last = it == max_iter;
        // early exit only: the verdicts on iteration it - 1 (none yet in iteration 1), and what the latch of var(it) counts
        int *const up = early && it > 1 ? h->d_el_unsat + (size_t)(it - 1) * TW : nullptr;
        int *const rem_prev = early ? h->d_remaining + it - 1 : nullptr;
        SC_TRY(launch_el_check(h, st, nb, c.method, alpha_for(c.alpha, it), skip, s, it == 1, early ? st.hard : nullptr, up));
        SC_TRY(launch_el_var(h, st, nb, skip, (early || last) ? 1 : 0, s, up, early ? it - 1 : 0, rem_prev));
        if (last) {
            hipLaunchKernelGGL(k_parity<true>, dim3(parity_blocks(h->m), 1), dim3(256), 0, s, h->d_row_ptr, h->d_col_idx, st.hard,
                               h->m, h->n, const_cast<u64 *>(st.synd), st.unsat, (const u64 *)st.done);
            LAUNCH_CHECK();
            hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, s, it, early ? 1 : 0, st.done, st.conv, st.unsat, parity_waves(h),
                               st.iters, h->d_remaining + it);
            LAUNCH_CHECK();
            break;
        }
        // Poll sparsely: a poll drains the queue and costs about as much as an iteration here,
        // while iterations enqueued for codewords that turn out to be finished return at once.
        const int ip = it - 1;  // the iteration whose verdict var(it) just latched
        // Graphs that come here are too large for LDS: a decode that converges does so in 3-5 iterations (the
        // attack loop once enough checks are in; measured 3-4 on the HQC-128 graph), one that does not runs to
        // max_iter.  Poll densely where convergence is likely, sparsely afterwards.
        if (early && el_poll_point(ip)) {
            h->sched.w[SCHED_EL_POLLS]++;
            SC_HIP(hipMemcpyAsync(h->h_remaining + ip, h->d_remaining + ip, sizeof(int), hipMemcpyDeviceToHost, s));
            SC_HIP(hipStreamSynchronize(s));
            if (h->h_remaining[ip] == 0) break;
        }
    }
    return 0;
}

// All iterations of one tile group on the 64-codeword-tile kernels, on SEVERAL streams
// ("lanes"): the group's tiles are dealt to lanes whose launch sequences (independent: a pass
// depends only on the previous pass over the same tiles) run one kernel out of phase, so that
// while one lane drains the tail of its kernel another lane's kernel fills the machine.  Same
// kernels, same cache footprint, same results.  Early-exit runs join the lanes at every poll.
constexpr int MAX_LANES = SCHED_MAX_LANES;
// measured on the HQC-128 bench (4-tile groups, ms per 4096-codeword step): 1 lane 104.0,
// 2 lanes 98.5, 3 lanes 101.3, 4 lanes 106.8 -- two kernels in flight fill each other's tails,
// more only shrink the launches.  SCALDPC_SPLIT=n overrides (1 = single stream).
int fixed_lanes(const scaldpc_bp *h, int g)
{
    if (h->E == 0) return 1;
    return lanes_of(h->kn.split, g);
}
int ensure_lanes(scaldpc_bp *h, int nl)
{
    for (int k = 1; k < nl; k++)
        if (!h->aux_stream[k]) {
            int dev = 0;
            SC_TRY(stream_acquire(&h->aux_stream[k], &dev));
            SC_HIP(hipEventCreateWithFlags(&h->ev_join[k], hipEventDisableTiming));
            SC_HIP(hipEventCreateWithFlags(&h->ev_phase[k], hipEventDisableTiming));
        }
    if (nl > 1 && !h->ev_join[0]) SC_HIP(hipEventCreateWithFlags(&h->ev_join[0], hipEventDisableTiming));  // [0]: the fork event
    return 0;
}
// The lanes of a call: lane 0 is the call's stream, lanes 1.. the handle's further streams.  fork() starts them behind
// everything enqueued on the call's stream so far, join() orders everything enqueued on them before it.  Lanes left open
// -- by a group the next one continues, or by an error return -- are joined when the scope ends.  So, held by decode_level:
// when decode_level returns, successfully or with an error, all work on the lanes is ordered before the call's stream.
struct Lanes {
    scaldpc_bp *h;
    hipStream_t s;
    int n = 1;          // lanes in use
    bool open = false;  // lanes 1.. may hold work that is not ordered before s yet
    Lanes(scaldpc_bp *h_, hipStream_t s_) : h(h_), s(s_) {}
    Lanes(const Lanes &) = delete;
    Lanes &operator=(const Lanes &) = delete;
    ~Lanes() { if (open) (void)join(); }
    hipStream_t operator[](int k) const { return k ? h->aux_stream[k] : s; }
    int fork(int nl)  // (ensure_lanes(h, nl) first)
    {
        n = nl;
        open = nl > 1;
        if (!open) return 0;
        SC_HIP(hipEventRecord(h->ev_join[0], s));
        for (int k = 1; k < n; k++) SC_HIP(hipStreamWaitEvent(h->aux_stream[k], h->ev_join[0], 0));
        return 0;
    }
    int join()
    {
        for (int k = 1; k < n; k++) {
            SC_HIP(hipEventRecord(h->ev_join[k], h->aux_stream[k]));
            SC_HIP(hipStreamWaitEvent(s, h->ev_join[k], 0));
        }
        open = false;
        return 0;
    }
};

// What the groups of one call learn from each other about polling -- PollState, poll_point, stops_unseen, runs_unseen --
// and what the host decides after a poll (after_poll) are in scaldpc_bp_sched.h.

// All iterations of the tile group [g0, g0+g) of `st`.  With defer_after > 0 the group stops at the first poll point from
// that iteration on at which at most half of its codewords are still running, and reports *deferred = true: those go to
// the compact pass.
// chain: bit 0 = this group CONTINUES the lanes of the group before it (same geometry, no host in between): no fork -- a
//        lane's work on the new group is ordered behind its own work on the previous one by its stream, and nothing else
//        feeds it;
//        bit 1 = the group after this one will continue them: no join at the end.  Without the per-group join / fork the lane
//        that runs a kernel ahead flows straight into the next group instead of idling for the other lane's last pass (and
//        the other lane for its first): ~75 us per group of 3.7 ms on the HQC-128 bench.
// sl: settled codewords (a fixed-iteration level on the record-form kernels; the default = off).  With sl.horizon = K > 0
//     the group enqueues iterations 1 ... K -- the check pass of K closes test K -- and then its closing sequence: the last
//     variable pass and the final test, as iteration max_iter.  The caller decodes again what was not frozen by K.
struct SettlePlan {
    unsigned *words = nullptr;  // [tile][SETTLE_WORDS] of the level's tiles, zero when the level starts
    int first_test = 0, horizon = 0;
    unsigned *of(int tile) const { return words + (size_t)tile * SETTLE_WORDS; }  // the words of a launch whose first tile it is
    // the sparse gate's tables (null = off), [tile][m] and [tile][n], zero when the level starts
    uint4 *rowf = nullptr;
    unsigned *colf = nullptr;
    int m = 0, n = 0;
    int gate_start = 0;  // the variable pass from which the level gates (settle_sparse_next_start; 0 = from the first test)
    // a tracked launch's argument: the words and tables of its first tile, what it is told about the tests, whether it gates
    Settle pass(int tile, int done, int mark, int gate) const
    {
        Settle s{of(tile), done, mark};
        if (rowf && mark) {
            s.rowf = rowf + (size_t)tile * m;
            s.colf = colf + (size_t)tile * n;
            s.ncol = n;
            s.gate = gate;
        }
        return s;
    }
};
int iterate_tiles(scaldpc_bp *h, const DecodeCall &c, Lanes &lanes, const TileState &st, int g0, int g, int defer_after,
                  bool *deferred, PollState &ps, int chain, const SettlePlan &sl)
{
    const hipStream_t s = lanes.s;
    const bool early = c.early;
    const int max_iter = c.max_iter, method = c.method, skip = early ? 1 : 0;
    const int nl = fixed_lanes(h, g);
    SC_TRY(ensure_lanes(h, nl));
    int gs[MAX_LANES], t0[MAX_LANES];
    deal_tiles(g, nl, gs, t0);
    TileState tv[MAX_LANES];  // lane k's tiles
    for (int k = 0; k < nl; k++) tv[k] = st.at(h, g0 + t0[k]);
    const int pw = parity_waves(h);
    const bool fused = fused_init(h, method);
    if (h->E && !fused) {
        with_prior(h, tv[0].pprior, st.first_col, [&](auto P, auto prior) {
            hipLaunchKernelGGL((k_init_msg<decltype(P)>), dim3((unsigned)((h->E + 3) / 4), g), dim3(256), 0, s, h->d_col_idx,
                               h->d_msg.get(), h->E, prior);
        });
        LAUNCH_CHECK();
    }
    int *rem = h->d_remaining;  // this group's row of "still running" counters
    if (early) SC_TRY(next_remaining_row(h, s, &rem, lanes.open));
    // (the accumulators / block counters of k_parity_fin and fused_commit are zeroed once per level, in decode_level,
    // and every launch leaves them zero)
    if (!(chain & 1)) SC_TRY(lanes.fork(nl));  // the other lanes start after everything enqueued on `s` so far
    // iteration 1 without its check pass: the first variable pass reads the first-message table and the syndrome planes
    // (a soft call runs iteration 1 WITH its check pass, reading the codewords' own priors: the first_fused = 0 sequence)
    const bool first_fuse = first_fusable(h, method) && !st.pprior;
    if (first_fuse) SC_TRY(ensure_first_table(h, method, alpha_for(c.alpha, 1), s));
    // The convergence test of iteration it rides on the check pass of it + 1 (fused_test) wherever the host does not need
    // its verdict in between: at the iterations it polls at, stops a group at, or ends with, the stand-alone launch stays.
    // (Running the test on a side stream beside the check pass instead was measured and rejected: -3.4 % on the config-5
    // sweep, profiles/r03/ab_test_overlap.log; so was the two-launch k_parity + k_finalize form in this loop.)
    const bool ride = early && h->kn.fuse_test && check_can_test(h, method) && pw >= FT_WORDS;
    bool verdict_pending[MAX_LANES] = {};  // lane k's last variable pass has not been tested yet: its next check pass will
    const bool recf = rec_form(h, method);
    bool rec_booted[MAX_LANES] = {};  // lane k has run its first record-form check pass (the one that also writes the sign masks)
    int boot_it[MAX_LANES] = {};      // ... and the iteration it did so in (0 = not yet)
    const bool tracked = sl.words && recf && !early;
    const int K = tracked ? sl.horizon : 0, last_test = K ? K : max_iter;
    // (re-)establish the one-kernel offset between neighbouring lanes -- in a chained group too (phase_reestablished,
    // scaldpc_bp_sched.h, with the measurements)
    bool set_phase = phase_reestablished(chain, K, max_iter);
    if (K) h->settle_saved += (long)nl * settle_launches_saved(K, max_iter);
    // A tracked group of a call that wants no posteriors: every record-form variable pass leaves its columns' decisions, and
    // the closing pass returns for the columns of a frozen tile that have them (k_var_rec).
    const bool keep_hard = tracked && st.post == nullptr;
    for (int it = 1; it <= max_iter; it++) {
        const bool last = it == max_iter;
        if (!settle_enqueued(it, K, max_iter)) continue;  // beyond the horizon
        const bool no_check = (first_fuse && it == 1) || !settle_has_check(it, K, max_iter);
        const bool poll = poll_point(it, defer_after, ps);
        lanes.open = nl > 1;  // (this iteration enqueues on them)
        for (int k = 0; k < nl && !no_check; k++) {
            CheckPass cp;
            cp.alpha = alpha_for(c.alpha, it);
            cp.first = fused && it == 1;
            cp.tile0 = t0[k];
            if (verdict_pending[k]) {
                cp.test = fused_test(h, tv[k], rem + (it - 1), it - 1, true);
                verdict_pending[k] = false;
            }
            cp.boot = recf && !cp.first && !rec_booted[k];
            if (cp.boot) rec_booted[k] = true;
            boot_it[k] = cp.boot ? it : boot_it[k];
            if (tracked)
                cp.settle = sl.pass(g0 + t0[k], settle_check_done(it, sl.first_test),
                                    cp.boot ? 0 : settle_check_mark(it, sl.first_test, last_test),
                                    cp.boot ? 0 : settle_sparse_check_gate(it, sl.first_test, last_test, sl.gate_start));
            SC_TRY(launch_check(h, tv[k], gs[k], method, skip, lanes[k], cp));
            if (set_phase && k + 1 < nl) {
                SC_HIP(hipEventRecord(h->ev_phase[k + 1], lanes[k]));
                SC_HIP(hipStreamWaitEvent(lanes[k + 1], h->ev_phase[k + 1], 0));
            }
        }
        if (!no_check) set_phase = false;  // (a first iteration without check passes leaves the offset to the second)
        if (!settle_has_var(it, K)) continue;  // (the closing variable pass takes this one's place: settle_horizon_usable)
        for (int k = 0; k < nl; k++) {
            VarPass vp;
            vp.write_out = (early || last) ? 1 : 0;
            vp.tile0 = t0[k];
            vp.first_synd = first_fuse && it == 1;
            // (the record form starts with iteration 2: an iteration 1 that has a check pass ran it in the message form)
            vp.rec = it > 1 && recf;
            vp.light = it > 1;
            vp.final_pass = last;
            vp.keep_hard = keep_hard && !last;
            if (tracked && !last)
                vp.settle = sl.pass(g0 + t0[k], settle_var_done(it, sl.first_test, last_test),
                                    settle_var_mark(it, sl.first_test, last_test),
                                    boot_it[k] == it ? 0 : settle_sparse_var_gate(it, sl.first_test, last_test, sl.gate_start));  // (a bootstrap check pass stamped no row)
            else if (keep_hard)  // the closing pass: it comes behind the check pass that completes the group's last test
                vp.settle = Settle{sl.of(g0 + t0[k]), last_test, 0};
            SC_TRY(launch_var(h, tv[k], gs[k], skip, lanes[k], vp));
            if (ride && !last && !poll) {
                verdict_pending[k] = true;  // the next check pass of this lane carries the test
            } else if (early || last) {  // convergence test + latch, one launch
                const dim3 grid(parity_blocks(h->m), gs[k]);
                const FusedTest pf = fused_test(h, tv[k], rem + it, it, early);
                if (pw >= FT_WORDS && h->kn.fuse_test)  // sharded accumulators / counters (fused_commit)
                    hipLaunchKernelGGL(k_parity_fin_sharded, grid, dim3(256), 0, lanes[k], h->d_row_ptr, h->d_col_idx, h->m, tv[k].synd,
                                       pf);
                else
                    hipLaunchKernelGGL(k_parity_fin, grid, dim3(256), 0, lanes[k], h->d_row_ptr, h->d_col_idx, pf.hard, h->m, h->n,
                                       tv[k].synd, pf.unsat, pf.pw, pf.it_prev, pf.latch, pf.done, pf.conv, pf.iters, pf.remaining);
                LAUNCH_CHECK();
            }
        }
        if (!early || last || !poll) continue;
        // a poll drains the queue (the GPU idles while the host turns around): skip the poll
        // points at which the call's earlier groups saw no codeword finish yet (poll_point)
        if (it == defer_after && stops_unseen(defer_after, max_iter, ps)) {
            note_unseen(ps);  // stop here unseen, as the last groups did
            h->sched.w[SCHED_UNSEEN]++;
            *deferred = true;
            if (chain & 2) return 0;  // (the next group stops unseen too and continues these lanes: no host in between)
            return lanes.join();
        }
        SC_TRY(lanes.join());
        SC_HIP(hipMemcpyAsync(h->h_remaining + it, rem + it, sizeof(int), hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
        set_phase = true;
        h->sched.w[SCHED_POLLS]++;
        // nobody left: done.  From `defer_after` on, any poll point may hand the stragglers over (after_poll)
        const PollVerdict v = after_poll(ps, it, defer_after, max_iter, h->h_remaining[it], std::min(c.batch - g0 * TW, g * TW), g,
                                          el_limit(h, method));
        if (v == POLL_DONE) return 0;
        if (v == POLL_HAND_OVER) {
            *deferred = true;
            return 0;
        }
    }
    if (chain & 2) return 0;  // (the next group continues these lanes; the last one of the chain joins)
    return lanes.join();
}

// the state planes of a compact level, for T2 dense tiles of stragglers
int ensure_level(scaldpc_bp *h, scaldpc_bp::Level &L, int T2)
{
    if (T2 <= L.cap_tiles) return 0;
    L.synd.reset(); L.hard.reset(); L.done.reset(); L.conv.reset(); L.unsat.reset();
    L.iters.reset(); L.ids.reset();
    L.cap_tiles = 0;
    SC_TRY(L.synd.ensure((size_t)T2 * h->m));
    SC_TRY(L.hard.ensure((size_t)T2 * h->n));
    SC_TRY(L.done.ensure((size_t)T2));
    SC_TRY(L.conv.ensure((size_t)T2));
    SC_TRY(L.unsat.ensure((size_t)T2 * parity_waves(h)));
    SC_TRY(L.iters.ensure((size_t)T2 * TW));
    SC_TRY(L.ids.ensure((size_t)T2 * TW));
    L.cap_tiles = T2;
    return 0;
}

// Settled codewords: a fixed-iteration level on the record-form kernels tracks which tiles' message state has stopped
// changing (Settle), its passes return at once for those, and with a horizon K -- forced, or learned from the handle's
// last call (settle_next_horizon) -- what would return at once is not enqueued at all.  Plans level `lvl`, clears the words.
int plan_settle(scaldpc_bp *h, const DecodeCall &c, int lvl, const TileState &st, SettlePlan *sl)
{
    const int settle = settle_mode(h->kn.settle, h->identity_from >= 0);
    if (lvl != 0 || c.early || settle <= 0 || !rec_form(h, c.method)) return 0;
    // the first iteration from which alpha_for() is one float to the call's end (the schedule never decreases)
    int alpha_from = 1;
    while (alpha_from < c.max_iter && alpha_for(c.alpha, alpha_from) != alpha_for(c.alpha, c.max_iter)) alpha_from++;
    sl->first_test = settle_first_test(alpha_from);
    const int soft = st.pprior ? 1 : 0;
    if (h->settle_key_iter != c.max_iter || h->settle_key_alpha != c.alpha || h->settle_key_soft != soft) {
        h->settle_next = 0;  // another max_iter / alpha / kind of priors: learn again
        h->sparse_start_next = 0;
        h->settle_key_iter = c.max_iter;
        h->settle_key_alpha = c.alpha;
        h->settle_key_soft = soft;
    }
    if (sl->first_test > c.max_iter) return 0;
    SC_TRY(h->d_settle.ensure((size_t)c.T * SETTLE_WORDS));
    SC_HIP(hipMemsetAsync(h->d_settle, 0, sizeof(unsigned) * (size_t)c.T * SETTLE_WORDS, c.s));  // once per level, as unsat
    sl->words = h->d_settle;
    if (settle_sparse_mode(h->kn.settle_sparse, settle, h->identity_from >= 0)) {
        SC_TRY(h->d_rowf.ensure((size_t)c.T * h->m));
        SC_TRY(h->d_colf.ensure((size_t)c.T * h->n));
        SC_HIP(hipMemsetAsync(h->d_rowf, 0, sizeof(uint4) * (size_t)c.T * h->m, c.s));
        SC_HIP(hipMemsetAsync(h->d_colf, 0, sizeof(unsigned) * (size_t)c.T * h->n, c.s));
        sl->rowf = h->d_rowf;
        sl->colf = h->d_colf;
        sl->m = h->m;
        sl->n = h->n;
        h->sparse_m = h->m;
        h->sparse_n = h->n;
        h->sparse_T = c.T;
        sl->gate_start = h->sparse_start_next > sl->first_test ? h->sparse_start_next : sl->first_test;
        h->sparse_start = sl->gate_start;
    }
    if (settle >= 2 && !c.no_sync) {
        const int K = h->kn.settle_horizon > 0 ? h->kn.settle_horizon : h->settle_next;
        if (settle_horizon_usable(K, sl->first_test, c.max_iter)) sl->horizon = K;
    }
    return 0;
}

// After a tracked level's groups: the tiles' frozen-at numbers, read back once (one synchronise).  With a horizon, every
// tile that was not frozen by it is decoded again from its inputs, in place, with all its iterations: the syndrome planes
// are intact, a fixed-iteration pass overwrites every output of a real codeword, and BP is deterministic.  Leaves the
// handle's report (scaldpc_bp_last_settle) and the horizon of its next call.
int collect_settle(scaldpc_bp *h, const DecodeCall &c, Lanes &lanes, const TileState &st, const SettlePlan &sl)
{
    const int T = c.T, Gl = std::min(c.G, T);
    SC_TRY(h->h_settle.ensure((size_t)T * SETTLE_WORDS));
    auto read_back = [&](int t0, int cnt, int last_test) -> int {
        SC_HIP(hipMemcpyAsync(h->h_settle + (size_t)t0 * SETTLE_WORDS, sl.of(t0), sizeof(unsigned) * (size_t)cnt * SETTLE_WORDS,
                              hipMemcpyDeviceToHost, c.s));
        SC_HIP(hipStreamSynchronize(c.s));
        for (int t = t0; t < t0 + cnt; t++) {
            unsigned latest = 0;
            for (int i = 0; i < SETTLE_SHARDS; i++) latest = std::max(latest, h->h_settle[(size_t)t * SETTLE_WORDS + i]);
            h->settle_frozen_at[t] = settle_frozen_at((int)latest, sl.first_test, last_test);
        }
        return 0;
    };
    h->settle_frozen_at.assign(T, 0);
    h->settle_K = sl.horizon;
    SC_TRY(read_back(0, T, sl.horizon ? sl.horizon : c.max_iter));
    if (sl.horizon) {
        SettlePlan again = sl;
        again.horizon = 0;
        PollState poll;  // (a fixed-iteration level: no polls, no hand-over)
        for (int t = 0; t < T;) {
            if (h->settle_frozen_at[t]) { t++; continue; }
            int g = 1;
            while (g < Gl && t + g < T && !h->settle_frozen_at[t + g]) g++;
            SC_HIP(hipMemsetAsync(sl.of(t), 0, sizeof(unsigned) * (size_t)g * SETTLE_WORDS, c.s));
            if (sl.rowf) {  // (a stale stamp equal to a pass of the re-run would read as fresh)
                SC_HIP(hipMemsetAsync(sl.rowf + (size_t)t * sl.m, 0, sizeof(uint4) * (size_t)g * sl.m, c.s));
                SC_HIP(hipMemsetAsync(sl.colf + (size_t)t * sl.n, 0, sizeof(unsigned) * (size_t)g * sl.n, c.s));
            }
            bool d = false;
            SC_TRY(iterate_tiles(h, c, lanes, st, t, g, 0, &d, poll, 0, again));
            SC_TRY(read_back(t, g, c.max_iter));
            h->settle_rerun += g;
            t += g;
        }
    }
    int frozen = 0, max_at = 0;
    for (int t = 0; t < T; t++) {
        frozen += h->settle_frozen_at[t] > 0;
        max_at = std::max(max_at, h->settle_frozen_at[t]);
    }
    const bool learns = settle_mode(h->kn.settle, h->identity_from >= 0) >= 2;
    h->settle_next = learns ? settle_next_horizon(T, frozen, max_at, (int)h->settle_rerun, c.max_iter) : 0;
    int min_at = 0;
    for (int t = 0; t < T; t++)
        if (h->settle_frozen_at[t] > 0 && (min_at == 0 || h->settle_frozen_at[t] < min_at)) min_at = h->settle_frozen_at[t];
    h->sparse_start_next = settle_sparse_next_start(min_at, sl.first_test);
    return 0;
}

int hand_down(scaldpc_bp *h, const DecodeCall &c, int lvl, const TileState &st, const std::vector<char> &deferred_tile);

// One compaction level: the c.batch codewords of `st` (c.T tiles), all iterations of one
// cache-resident tile group after the other.  In early-exit runs the stragglers of
// mostly-converged groups are gathered into dense tiles of their own and re-decoded from their
// inputs one level down (codewords are independent and BP is deterministic: identical
// results), and that level may shed its own stragglers again -- on the config-5 sweep the
// second level drops the codewords that needed 5-7 iterations and leaves the ~0.5 % that never
// converge to run their 100 iterations in 3 tiles instead of 11.
int decode_level(scaldpc_bp *h, const DecodeCall &c, int lvl, const TileState &st)
{
    const int T = c.T, Gl = std::min(c.G, T), max_iter = c.max_iter;
    const bool early = c.early;
    const int el = (T == 1 && c.batch <= el_limit(h, c.method)) ? c.batch : 0;  // a handful of codewords: row-parallel kernels
    if (el)
        SC_TRY(ensure_el(h, el));
    else
        SC_TRY(ensure_msg(h, Gl, c.method));
    if (lvl == 0) {
        h->last_group = el ? 0 : Gl;
        h->last_early = early;
    }
    h->stat_levels = lvl;
    if (el) {
        h->stat_el = el;
        return iterate_el(h, c, st, el);
    }

    const int defer_after = defer_after_of(early, lvl, h->kn.compact_after, max_iter);
    // accumulators and block counters of the convergence tests: zero once, every launch leaves them zero
    SC_HIP(hipMemsetAsync(st.unsat, 0, sizeof(u64) * (size_t)T * parity_waves(h), c.s));
    std::vector<char> deferred_tile(T, 0);
    bool any = false;
    PollState poll;
    // fixed-iteration runs chain consecutive groups of the same geometry lane by lane (iterate_tiles): no host interaction,
    // every pass of a lane depends only on that lane's previous pass over the same slice of the message array
    // (A/B on the HQC-128 bench, best of five runs each: 60.43 against 61.12 ms per step; tanh rule 94.5 against 95.0-95.4:
    // profiles/r04/ab_chain_groups.log)
    const bool lanes2 = fused_init(h, c.method) && fixed_lanes(h, Gl) > 1;
    // Early-exit runs chain too where the host stays out: a group that will stop at the hand-over point UNSEEN and polls
    // nowhere before (runs_unseen, from the same PollState and rules iterate_tiles decides by) enqueues its launches
    // without ever synchronising.
    Lanes lanes(h, c.s);
    SettlePlan sl;
    SC_TRY(plan_settle(h, c, lvl, st, &sl));
    for (int g0 = 0; g0 < T; g0 += Gl) {
        const int g = std::min(Gl, T - g0);
        bool d = false;
        const bool next_full = g0 + Gl < T && std::min(Gl, T - (g0 + Gl)) == Gl;
        // (no chaining across the wrap of the "still running" counter rows, which clears them all: chain_bits)
        const int chain = chain_bits(early, lanes2, g == Gl, g0 == 0, next_full, lanes.open, defer_after, max_iter, poll, h->rem);
        h->sched.note_group(lvl, early, chain);
        SC_TRY(iterate_tiles(h, c, lanes, st, g0, g, defer_after, &d, poll, chain, sl));
        if (d) {
            any = true;
            for (int t = g0; t < g0 + g; t++) deferred_tile[t] = 1;
        }
    }
    if (sl.words && !c.no_sync) SC_TRY(collect_settle(h, c, lanes, st, sl));
    return any ? hand_down(h, c, lvl, st, deferred_tile) : 0;
}

// The stragglers of the tiles marked in deferred_tile, one level down: gathered into dense tiles of their own, decoded
// there from their inputs, and their results put back.
int hand_down(scaldpc_bp *h, const DecodeCall &c, int lvl, const TileState &st, const std::vector<char> &deferred_tile)
{
    const hipStream_t s = c.s;
    const int T = c.T;
    std::vector<u64> done_h(T);
    SC_HIP(hipMemcpyAsync(done_h.data(), st.done, sizeof(u64) * T, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    pvec<int> ids, slot_of((size_t)T * TW, -1);
    for (int t = 0; t < T; t++) {
        if (!deferred_tile[t]) continue;
        for (int w = 0; w < TW; w++) {
            const long b = (long)t * TW + w;
            if (b < c.batch && !((done_h[t] >> w) & 1)) {
                slot_of[b] = (int)ids.size();
                ids.push_back((int)b);
            }
        }
    }
    DecodeCall c2 = c;  // the level below: the stragglers alone, in dense tiles
    c2.batch = (int)ids.size();
    if (c2.batch == 0) return 0;
    if (lvl == 0) h->stat_deferred = c2.batch;
    h->sched.w[SCHED_HANDED + lvl] = c2.batch;
    const int T2 = c2.T = (c2.batch + TW - 1) / TW;
    ids.resize((size_t)T2 * TW, -1);
    scaldpc_bp::Level &L = h->lv[lvl + 1];
    SC_TRY(ensure_level(h, L, T2));
    SC_TRY(grow(L.slot_of, (size_t)T * TW));
    if (c.want_post) SC_TRY(grow(L.post, (size_t)T2 * h->n * TW));
    const int pcols = st.pprior ? h->n - st.first_col : 0;
    if (pcols) SC_TRY(grow(L.pprior, (size_t)T2 * pcols * TW));
    SC_HIP(hipMemcpyAsync(L.ids, ids.data(), sizeof(int) * ids.size(), hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(L.slot_of, slot_of.data(), sizeof(int) * slot_of.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_gather_planes, dim3((h->m + 63) / 64, T2), dim3(256), 0, s, st.synd, h->m, L.ids, L.synd);
    LAUNCH_CHECK();
    if (pcols) {  // the stragglers' priors go with them
        hipLaunchKernelGGL(k_gather_prior, dim3((pcols + 3) / 4, T2), dim3(256), 0, s, st.pprior, pcols, L.ids, L.pprior);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_init_state, dim3(T2), dim3(64), 0, s, c2.batch, c.max_iter, L.done, L.conv, L.iters);
    LAUNCH_CHECK();
    SC_HIP(hipMemsetAsync(L.hard, 0, sizeof(u64) * (size_t)T2 * h->n, s));
    SC_HIP(hipStreamSynchronize(s));  // ids / slot_of are locals, and the level below reuses the stream
    const TileState st2{L.synd, L.hard, L.done, L.conv, L.unsat, L.iters, c.want_post ? L.post : nullptr,
                        pcols ? L.pprior.get() : nullptr, st.first_col};
    SC_TRY(decode_level(h, c2, lvl + 1, st2));
    hipLaunchKernelGGL(k_scatter_planes, dim3((h->n + 63) / 64, T), dim3(256), 0, s, st.hard, h->n, L.slot_of, L.hard);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scatter_state, dim3(T), dim3(64), 0, s, st.iters, st.conv, L.slot_of, L.iters, L.conv);
    LAUNCH_CHECK();
    if (c.want_post) {
        hipLaunchKernelGGL(k_scatter_post, dim3(h->n, T), dim3(64), 0, s, st.post, h->n, L.slot_of, L.post);
        LAUNCH_CHECK();
    }
    return 0;
}

// The decode proper, on inputs already staged as planes (h->d_synd; h->d_recv when the
// caller wants e XOR v): state reset, then decode_level.
// Results stay on the device (h->d_hard / d_post / d_conv / d_iters).
// pprior / first_col: a soft call's prior plane (h->d_pprior) and its first column; null = the handle's shared priors.
int run_core(scaldpc_bp *h, const DecodeCall &c, const float *pprior = nullptr, int first_col = 0)
{
    if (!c.state_ready) {
        hipLaunchKernelGGL(k_init_state, dim3(c.T), dim3(64), 0, c.s, c.batch, c.max_iter, h->d_done, h->d_conv, h->d_iters);
        LAUNCH_CHECK();
        SC_HIP(hipMemsetAsync(h->d_hard, 0, sizeof(u64) * (size_t)c.T * h->n, c.s));
    }
    h->last_group = 0;
    h->stat_deferred = 0;
    h->stat_el = 0;
    h->stat_levels = 0;

    // small graph: the LDS-resident single-launch decoder, plane I/O (Monte-Carlo entry points)
    if (const size_t lds = small_lds(h)) {
        return launch_small<true>(h, lds, c.method, c.batch, h->d_synd, SCALDPC_IN_SYNDROME, c.max_iter, c.alpha, c.early, h->d_hard,
                                  c.want_post ? h->d_post.get() : nullptr, h->d_iters, h->d_conv, c.s, pprior, first_col);
    }
    const TileState st{h->d_synd, h->d_hard, h->d_done, h->d_conv, h->d_unsat, h->d_iters,
                       c.want_post ? h->d_post : nullptr, pprior, first_col};
    return decode_level(h, c, 0, st);
}

}  // namespace

#define TMARK(name)                                                                                   \
    do {                                                                                              \
        static const bool on__ = getenv("SCALDPC_TIMING") != nullptr;                                 \
        if (on__) {                                                                                   \
            auto now__ = std::chrono::steady_clock::now();                                            \
            fprintf(stderr, "[create] %-10s %8.1f us\n", name,                                        \
                    std::chrono::duration<double, std::micro>(now__ - tmark_last()).count());         \
            tmark_last() = now__;                                                                     \
        }                                                                                             \
    } while (0)
static std::chrono::steady_clock::time_point &tmark_last()
{
    static thread_local std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    return t;
}

namespace {

// Everything that depends on the WHOLE graph, from the host CSR and the node degrees: degree
// buckets, CSC permutation, identity block, and the device copy of the arrays every path needs --
// views into ONE allocation filled by ONE copy: the attack loop builds a new decoder per decode
// (hqc.py:694), so construction is on its critical path (a dozen hipMalloc + synchronous hipMemcpy
// pairs cost more than the decode).  The per-kernel-family tables follow on first use
// (ensure_tile_tables / ensure_el_tables).  Used by scaldpc_bp_create and, on a handle whose graph
// has grown, by refresh_full (there CSR and priors already live in buffers of their own).
// Consumes cdeg.
int finish_graph(scaldpc_bp *h, const int *row_ptr, const int *col_idx, const pvec<int> &rdeg, pvec<int> &cdeg)
{
    const int m = h->m, n = h->n;
    const long nnz = h->E;
    h->max_row_deg = m ? *std::max_element(rdeg.begin(), rdeg.end()) : 0;
    h->min_row_deg = m ? *std::min_element(rdeg.begin(), rdeg.end()) : 0;
    h->max_col_deg = *std::max_element(cdeg.begin(), cdeg.end());
    static const int vb[] = {1, 2, 4, 8, 16, 32, 64};
    static const int rb[] = {2, 4, 8, 16, 32, 64};
    HostBuckets hv, hr;
    build_buckets(cdeg, vb, 7, true, hv);
    build_buckets(rdeg, rb, 6, false, hr);
    TMARK("buckets");
    h->var_bk = hv.bk;
    h->row_bk = hr.bk;
    h->need_scratch = hv.has_generic || hr.has_generic;
    h->identity_from = -1;
    if (n > m) {  // H = [Hin | I_m]?  (what hqc.decode builds, hqc.py:680)
        bool ident = true;
        for (int r = 0; r < m && ident; r++) {
            const int j = n - m + r;
            ident = cdeg[j] == 1 && row_ptr[r + 1] > row_ptr[r] && col_idx[row_ptr[r + 1] - 1] == j;
        }
        h->identity_from = ident ? n - m : -1;
    }
    h->el_ok = nnz > 0 && h->max_row_deg <= ROW_CAP && h->max_col_deg <= 64;  // the row-parallel path can take this graph
    const bool own_csr = h->incremental;  // CSR and priors already live in growable buffers of their own
    size_t total = 0;
    auto reserve = [&](size_t cnt) {  // 256-byte aligned sections
        const size_t off = total;
        total += (cnt + 63) / 64 * 64;
        return off;
    };
    const size_t o_row_ptr = own_csr ? 0 : reserve((size_t)m + 1), o_col_idx = own_csr ? 0 : reserve((size_t)nnz);
    const size_t o_col_ptr = reserve((size_t)n + 1), o_csc_edge = reserve((size_t)nnz), o_var_list = reserve(hv.list.size());
    const size_t o_prior = own_csr ? 0 : reserve((size_t)n);
    int *const host = stage_buffer(total);  // not cleared: every word a kernel reads is written below
    if (!host) return fail(SCALDPC_ENOMEM, "out of host memory");
    TMARK("reserve");
    if (!own_csr) {
        std::copy(row_ptr, row_ptr + m + 1, host + o_row_ptr);
        std::copy(col_idx, col_idx + nnz, host + o_col_idx);
    }
    // CSC permutation: edges grouped by column, ascending row (row-major scan keeps rows ascending)
    int *col_ptr = host + o_col_ptr, *csc_edge = host + o_csc_edge;
    {
        col_ptr[0] = 0;
        for (int j = 0; j < n; j++) col_ptr[j + 1] = col_ptr[j] + cdeg[j];
        pvec<int> cursor(col_ptr, col_ptr + n);
        for (int e = 0; e < (int)nnz; e++) csc_edge[cursor[col_idx[e]]++] = e;
    }
    std::copy(hv.list.begin(), hv.list.end(), host + o_var_list);
    TMARK("csc");
    SC_TRY(h->d_graph.ensure(total));
    if (hipMemcpy(h->d_graph, host, total * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
        return fail(SCALDPC_EHIP, "graph upload failed");
    TMARK("upload");
    // what the lazy table builders need
    if (!own_csr) h->hg_row_ptr.assign(row_ptr, row_ptr + m + 1);
    h->hg_col_ptr.assign(col_ptr, col_ptr + n + 1);
    h->hg_csc_edge.assign(csc_edge, csc_edge + nnz);
    h->hg_cdeg.swap(cdeg);
    h->hg_var = std::move(hv);
    h->hg_row = std::move(hr);
    TMARK("keep");
    if (!own_csr) {
        h->d_row_ptr = h->d_graph + o_row_ptr;
        h->d_col_idx = h->d_graph + o_col_idx;
        h->d_prior = (float *)(h->d_graph + o_prior);
    }
    h->d_col_ptr = h->d_graph + o_col_ptr;
    h->d_csc_edge = h->d_graph + o_csc_edge;
    h->d_var_list = h->d_graph + o_var_list;
    return 0;
}

// ---- a graph that grows (scaldpc_bp_append_rows) -------------------------------------------------
// First append: CSR and priors leave the construction-time allocation for buffers with spare
// capacity; the host keeps the CSR (col_idx is recovered from the CSC mirror); the row-parallel
// tables are dropped and come back with free lanes on the next decode.
int make_incremental(scaldpc_bp *h)
{
    if (h->incremental) return 0;
    const size_t rows = (size_t)h->m + 1, edges = (size_t)h->E, cols = (size_t)h->n;
    SC_TRY(h->d_csr_rp.ensure(rows + rows / 2 + 256));
    SC_TRY(h->d_csr_ci.ensure(edges + edges / 2 + 4096));
    SC_TRY(h->d_prior_buf.ensure(cols + cols / 2 + 256));
    SC_HIP(hipMemcpy(h->d_csr_rp, h->d_row_ptr, rows * sizeof(int), hipMemcpyDeviceToDevice));
    if (edges) SC_HIP(hipMemcpy(h->d_csr_ci, h->d_col_idx, edges * sizeof(int), hipMemcpyDeviceToDevice));
    SC_HIP(hipMemcpy(h->d_prior_buf, h->d_prior, cols * sizeof(float), hipMemcpyDeviceToDevice));
    h->d_row_ptr = h->d_csr_rp;
    h->d_col_idx = h->d_csr_ci;
    h->d_prior = h->d_prior_buf;
    h->hg_col_idx.resize(edges);
    for (int j = 0; j < h->n; j++)
        for (int k = h->hg_col_ptr[j]; k < h->hg_col_ptr[j + 1]; k++) h->hg_col_idx[h->hg_csc_edge[k]] = j;
    h->incremental = true;
    h->d_el_tab.reset();  // rebuilt with free lanes per column on the next use
    h->d_el_slots = h->d_el_slot_col = nullptr;
    return 0;
}

// CSR and priors of a growing graph: room for `need` elements (and half as many again), the first `used` kept
template <typename T>
int grow_graph(Buf<T> &b, size_t used, size_t need)
{
    return b.grow_keep(used, need, need + need / 2 + 256);
}

// The tile / LDS kernels' view of a grown graph: CSC, degree buckets, identity block, device CSC
// arrays, and (lazily, on their first use) the tile tables.  O(E) on the host, as a construction.
int refresh_full(scaldpc_bp *h)
{
    if (!h->full_stale) return 0;
    pvec<int> rdeg(h->m), cdeg(h->hg_cdeg);
    for (int r = 0; r < h->m; r++) rdeg[r] = h->hg_row_ptr[r + 1] - h->hg_row_ptr[r];
    h->d_graph.reset();
    h->d_tile_tab.reset();
    h->d_var_meta = h->d_csc_list = h->d_row_list = nullptr;
    SC_TRY(finish_graph(h, h->hg_row_ptr.data(), h->hg_col_idx.data(), rdeg, cdeg));
    h->full_stale = false;
    return 0;
}

// ---- what the entry points share ------------------------------------------------------------------
int check_usable(const scaldpc_bp *h)
{
    if (!h->broken) return 0;
    return fail(SCALDPC_EHIP, "this decoder is unusable: an earlier scaldpc_bp_append_rows failed part-way; destroy it and build a new one");
}

// fp32 prior LLRs of `count` columns, the same expression as the oracle's f32 instantiation: log((1-p)/p).  Priors come
// in long runs of one value -- [w/N]*N ++ [1-certainty]*R, hqc.py:686-691 -- so the previous result is reused while p
// repeats.  `first` is the column of probs[0] (for the message).
int prior_llrs(const double *probs, int first, int count, pvec<float> &llr)
{
    float last_p = 0.0f, last_llr = 0.0f;
    for (int j = 0; j < count; j++) {
        if (!(probs[j] >= 0.0 && probs[j] <= 1.0))
            return fail(SCALDPC_EINVAL, "channel_probs[%d] = %g is not a probability", first + j, probs[j]);
        const float p = (float)probs[j];
        if (j == 0 || p != last_p) {
            last_p = p;
            last_llr = logf((1.0f - p) / p);
        }
        llr[j] = last_llr;
    }
    return 0;
}

// The preamble of the decoding entry points (decode_batch and the Monte-Carlo runs): priors set, and of the DecodeCall the
// batch, max_iter with its default, the stream, tiles of 64 codewords (at most 65535: a grid dimension) and tiles per group.
// What the entry decodes with (method, alpha, early, want_post, the two flags) it fills in itself.
// what scaldpc_bp_last_settle reports: cleared when a call starts, whatever path it takes
void settle_report_reset(scaldpc_bp *h)
{
    h->settle_frozen_at.clear();
    h->settle_saved = h->settle_rerun = 0;
    h->settle_K = 0;
    h->sparse_m = h->sparse_n = h->sparse_T = 0;
    h->sparse_start = 0;
}
int begin_call(scaldpc_bp *h, int batch, int max_iter, void *stream, DecodeCall *c)
{
    if (!h->have_prior || h->prior_n < h->n)
        return fail(SCALDPC_EINVAL, "channel probabilities not set (columns [%d, %d))", h->have_prior ? h->prior_n : 0, h->n);
    h->sched.reset();
    settle_report_reset(h);
    c->batch = batch;
    c->max_iter = max_iter > 0 ? max_iter : h->n;
    c->s = stream ? (hipStream_t)stream : h->own_stream;
    c->T = (batch + TW - 1) / TW;
    if (c->T > 65535) return fail(SCALDPC_EINVAL, "batch %d too large for one call (max %d)", batch, 65535 * TW);
    c->G = (h->tile_group > 0) ? std::min(h->tile_group, c->T) : auto_group(h, c->T);
    return 0;
}

// An entry point that fails after its preamble synchronises the call's stream before it returns: nothing it enqueued
// (on the stream, or on lanes decode_level has joined into it) is still in flight when a block it released is handed out
// again.  Its success paths keep their own synchronisation and say done().
struct SyncOnError {
    hipStream_t s;
    bool ok = false;
    ~SyncOnError() { if (!ok) (void)hipStreamSynchronize(s); }
    int done() { ok = true; return 0; }
};

// HIP events with timing (scaldpc_bp_time_kernels), destroyed with their owner
struct TimingEvents {
    std::vector<hipEvent_t> ev;
    TimingEvents() = default;
    TimingEvents(const TimingEvents &) = delete;
    TimingEvents &operator=(const TimingEvents &) = delete;
    ~TimingEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    int create(size_t count)
    {
        ev.assign(count, nullptr);
        for (hipEvent_t &e : ev) SC_HIP(hipEventCreate(&e));
        return 0;
    }
    hipEvent_t &operator[](size_t i) { return ev[i]; }
};

// `bytes` of input on the device: the caller's own with SCALDPC_F_DEVICE_IO, else a copy in the handle's staging block
int stage_input(scaldpc_bp *h, const uint8_t *in, size_t bytes, bool dev_io, hipStream_t s, const uint8_t **din)
{
    *din = in;
    if (dev_io) return 0;
    SC_TRY(grow(h->d_in, bytes));
    SC_HIP(hipMemcpyAsync(h->d_in, in, bytes, hipMemcpyHostToDevice, s));
    *din = h->d_in;
    return 0;
}

// A call's per-codeword outputs (null: not wanted).  With SCALDPC_F_DEVICE_IO the caller's arrays are device memory and the
// kernels write them directly; otherwise the handle's staging blocks stand in (stage_outputs) and copy_outputs brings them
// to the caller.
struct Outputs {
    uint8_t *bits = nullptr;
    float *llr = nullptr;
    int32_t *iters = nullptr;
    uint8_t *conv = nullptr;
};
// with_state: stage the iteration / convergence pair (one request each, always together) even where only one is wanted
int stage_outputs(scaldpc_bp *h, const Outputs &out, int batch, bool dev_io, bool with_state, Outputs *dev)
{
    *dev = out;
    if (dev_io) return 0;
    const size_t planes = (size_t)batch * h->n;
    if (out.bits) {
        SC_TRY(grow(h->d_out_bits, planes));
        dev->bits = h->d_out_bits;
    }
    if (out.llr) {
        SC_TRY(grow(h->d_out_llr, planes));
        dev->llr = h->d_out_llr;
    }
    if (with_state) {
        if ((size_t)batch > h->d_out_conv.cap()) {  // (d_out_conv is requested last: its capacity is the pair's)
            h->d_out_iters.reset();
            h->d_out_conv.reset();
            SC_TRY(h->d_out_iters.ensure((size_t)batch));
            SC_TRY(h->d_out_conv.ensure((size_t)batch));
        }
        dev->iters = out.iters ? h->d_out_iters.get() : nullptr;
        dev->conv = out.conv ? h->d_out_conv.get() : nullptr;
    }
    return 0;
}
int copy_outputs(const scaldpc_bp *h, const Outputs &out, const Outputs &dev, int batch, bool dev_io, hipStream_t s)
{
    if (dev_io) return 0;
    const size_t planes = (size_t)batch * h->n;
    if (out.bits) SC_HIP(hipMemcpyAsync(out.bits, dev.bits, planes, hipMemcpyDeviceToHost, s));
    if (out.llr) SC_HIP(hipMemcpyAsync(out.llr, dev.llr, sizeof(float) * planes, hipMemcpyDeviceToHost, s));
    if (out.iters) SC_HIP(hipMemcpyAsync(out.iters, dev.iters, sizeof(int) * (size_t)batch, hipMemcpyDeviceToHost, s));
    if (out.conv) SC_HIP(hipMemcpyAsync(out.conv, dev.conv, (size_t)batch, hipMemcpyDeviceToHost, s));
    return 0;
}

// The same for an optional per-trial output of the Monte-Carlo sweeps (out null: not wanted, *dev null): the caller's own array
// with SCALDPC_F_DEVICE_IO, else the handle's block, grown to `count` elements ...
template <typename T, bool P>
int mc_stage(Buf<T, P> &block, T *out, size_t count, bool dev_io, T **dev)
{
    *dev = out;
    if (!out || dev_io) return 0;
    SC_TRY(grow(block, count));
    *dev = block.get();
    return 0;
}
// ... from which `count` elements then go to the caller
template <typename T>
int mc_unstage(T *out, const T *dev, size_t count, bool dev_io, hipStream_t s)
{
    if (out && !dev_io) SC_HIP(hipMemcpyAsync(out, dev, sizeof(T) * count, hipMemcpyDeviceToHost, s));
    return 0;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================

extern "C" {

int scaldpc_bp_create(int32_t m, int32_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                      scaldpc_bp **out)
{
    if (!out) return fail(SCALDPC_EINVAL, "out is NULL");
    *out = nullptr;
    if (m <= 0 || n <= 0 || nnz < 0 || !row_ptr || (nnz && !col_idx))
        return fail(SCALDPC_EINVAL, "bad graph arguments (m=%d n=%d nnz=%lld)", m, n, (long long)nnz);
    if (nnz > 0x7fffffffLL) return fail(SCALDPC_EINVAL, "nnz too large");
    if (row_ptr[0] != 0 || row_ptr[m] != nnz) return fail(SCALDPC_EINVAL, "row_ptr does not span [0, nnz]");
    TMARK("start");
    pvec<int> rdeg(m), cdeg(n, 0);
    for (int r = 0; r < m; r++) {
        if (row_ptr[r + 1] < row_ptr[r]) return fail(SCALDPC_EINVAL, "row_ptr not monotone at row %d", r);
        rdeg[r] = row_ptr[r + 1] - row_ptr[r];
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; e++) {
            if (col_idx[e] < 0 || col_idx[e] >= n) return fail(SCALDPC_EINVAL, "col_idx out of range at edge %d", e);
            if (e > row_ptr[r] && col_idx[e] <= col_idx[e - 1])
                return fail(SCALDPC_EINVAL, "col_idx not strictly ascending in row %d", r);
            cdeg[col_idx[e]]++;
        }
    }
    scaldpc_bp *h = new (std::nothrow) scaldpc_bp();
    if (!h) return fail(SCALDPC_ENOMEM, "out of host memory");
    knobs_from_env(h->kn);
    h->m = m;
    h->n = n;
    h->E = nnz;
    TMARK("validate");
    int rc = finish_graph(h, row_ptr, col_idx, rdeg, cdeg);
    if (!rc) rc = stream_acquire(&h->own_stream, &h->device);
    TMARK("stream");
    if (rc) {
        scaldpc_bp_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int scaldpc_bp_set_channel_probs(scaldpc_bp *h, const double *probs)
{
    if (!h || !probs) return fail(SCALDPC_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    SC_TRY(check_usable(h));
    DeviceGuard dg(h->device);
    pvec<float> llr(h->n);
    SC_TRY(prior_llrs(probs, 0, h->n, llr));
    SC_HIP(hipMemcpy(h->d_prior, llr.data(), sizeof(float) * h->n, hipMemcpyHostToDevice));
    h->h_probs.assign(probs, probs + h->n);
    h->thr_valid = false;
    h->first_valid = false;
    h->settle_next = 0;  // (the settle horizon was learned on the priors and rows that were: learn again)
    h->sparse_start_next = 0;
    h->ratio_valid = false;
    h->have_prior = true;
    h->prior_n = h->n;
    return 0;
}

int scaldpc_bp_set_channel_probs_tail(scaldpc_bp *h, int32_t first, int32_t count, const double *probs)
{
    if (!h || (count > 0 && !probs)) return fail(SCALDPC_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    SC_TRY(check_usable(h));
    DeviceGuard dg(h->device);
    if (first < 0 || count < 0 || (long)first + count > h->n)
        return fail(SCALDPC_EINVAL, "columns [%d, %d) are outside the graph (n = %d)", first, first + count, h->n);
    if (first > h->prior_n) return fail(SCALDPC_EINVAL, "priors of columns [%d, %d) are still unset", h->prior_n, first);
    if (count == 0) return 0;
    if (h->async_used) SC_HIP(hipDeviceSynchronize());
    pvec<float> llr(count);
    SC_TRY(prior_llrs(probs, first, count, llr));
    SC_HIP(hipMemcpy(h->d_prior + first, llr.data(), sizeof(float) * count, hipMemcpyHostToDevice));
    h->h_probs.resize(h->n, 0.0);
    std::copy(probs, probs + count, h->h_probs.begin() + first);
    h->thr_valid = false;
    h->first_valid = false;
    h->settle_next = 0;  // (the settle horizon was learned on the priors and rows that were: learn again)
    h->sparse_start_next = 0;
    h->ratio_valid = false;
    h->prior_n = std::max(h->prior_n, first + count);
    h->have_prior = true;
    return 0;
}

int scaldpc_bp_append_rows(scaldpc_bp *h, int32_t nrows, const int32_t *row_ptr, const int32_t *col_idx, int32_t new_n)
{
    if (!h || nrows < 0 || (nrows > 0 && !row_ptr)) return fail(SCALDPC_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    SC_TRY(check_usable(h));
    DeviceGuard dg(h->device);
    CacheBypass guard(h->async_used);
    if (new_n < h->n) return fail(SCALDPC_EINVAL, "new_n = %d is smaller than the current block length %d", new_n, h->n);
    const long add = nrows ? row_ptr[nrows] : 0;
    if (nrows && (row_ptr[0] != 0 || add < 0 || (add && !col_idx))) return fail(SCALDPC_EINVAL, "row_ptr does not start at 0");
    if ((long)h->E + add > 0x7fffffffL) return fail(SCALDPC_EINVAL, "nnz too large");
    // only the NEW rows are validated; the old ones were when they came in
    for (int r = 0; r < nrows; r++) {
        if (row_ptr[r + 1] < row_ptr[r]) return fail(SCALDPC_EINVAL, "row_ptr not monotone at appended row %d", r);
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; e++) {
            if (col_idx[e] < 0 || col_idx[e] >= new_n) return fail(SCALDPC_EINVAL, "col_idx out of range at appended edge %d", e);
            if (e > row_ptr[r] && col_idx[e] <= col_idx[e - 1])
                return fail(SCALDPC_EINVAL, "col_idx not strictly ascending in appended row %d", r);
        }
    }
    if (nrows == 0 && new_n == h->n) return 0;
    if (h->async_used) SC_HIP(hipDeviceSynchronize());  // the tables below may still be read by work in flight
    TMARK("app:start");
    // From here on the handle is being rebuilt in place.  A failure below (an allocation, a copy) leaves host mirrors
    // and device arrays in disagreement: the handle is then marked broken and refuses every later call.
    struct Unfinished {
        scaldpc_bp *h;
        bool done = false;
        ~Unfinished() { if (!done) h->broken = true; }
    } unfinished{h};
    SC_TRY(make_incremental(h));
    hipStream_t s = h->own_stream;
    const int m0 = h->m, n0 = h->n;
    const long E0 = h->E;
    // (each view is re-pointed right after its own buffer moved: a later failure must not leave it dangling)
    SC_TRY(grow_graph(h->d_csr_rp, (size_t)m0 + 1, (size_t)m0 + 1 + nrows));
    h->d_row_ptr = h->d_csr_rp;
    SC_TRY(grow_graph(h->d_csr_ci, (size_t)E0, (size_t)E0 + add));
    h->d_col_idx = h->d_csr_ci;
    SC_TRY(grow_graph(h->d_prior_buf, (size_t)n0, (size_t)new_n));
    h->d_prior = h->d_prior_buf;

    // ---- host mirror: CSR, column degrees ------------------------------------------------------
    h->hg_row_ptr.reserve((size_t)m0 + 1 + nrows);
    for (int r = 0; r < nrows; r++) h->hg_row_ptr.push_back((int)(E0 + row_ptr[r + 1]));
    h->hg_col_idx.insert(h->hg_col_idx.end(), col_idx, col_idx + add);
    h->hg_cdeg.resize(new_n, 0);
    for (int r = 0; r < nrows; r++) h->max_row_deg = std::max(h->max_row_deg, row_ptr[r + 1] - row_ptr[r]);

    TMARK("app:mirror");
    // ---- row-parallel tables, in place: one slot word per new edge while its column has a free lane
    const bool had_tables = h->d_el_tab;
    pvec<int> &dirty_slot = h->el_dirty_slot, &dirty_col = h->el_dirty_col;  // words of h_el_slots / h_el_col that changed
    dirty_slot.clear();
    dirty_col.clear();
    bool el_alive = had_tables;
    if (had_tables) {
        h->seg_slot.resize(new_n, -1);
        h->seg_cap.resize(new_n, 0);
    }
    // A word may be listed more than once (filled in place, then moved with its column in the same call):
    // the pairs sent to the device carry the mirror's FINAL value of the word, so duplicates are harmless
    // in whatever order the scatter kernel applies them.
    auto set_slot = [&](size_t i, int v) {
        h->h_el_slots[i] = v;
        dirty_slot.push_back((int)i);
    };
    auto new_segment = [&](int c, int cap, const int *edges, int d) {  // writes a whole segment
        const int s0 = el_alloc_segment(h, cap), start = s0 & 63;
        for (int k = 0; k < cap; k++) {
            set_slot(2 * (size_t)(s0 + k), k < d ? edges[k] : -1);
            set_slot(2 * (size_t)(s0 + k) + 1, el_tag(start, k, cap, true));
        }
        h->h_el_col[s0] = c;
        dirty_col.push_back(s0);  // (a segment start is handed out once: no duplicates)
        h->seg_slot[c] = s0;
        h->seg_cap[c] = (unsigned char)cap;
    };
    int edges_tmp[64];
    for (long i = 0; i < add; i++) {
        const int c = col_idx[i], e = (int)(E0 + i);
        const int d_old = h->hg_cdeg[c]++;
        h->max_col_deg = std::max(h->max_col_deg, d_old + 1);
        if (!el_alive) continue;
        if (d_old + 1 > 64) {  // a column wider than a wave: the row-parallel path is gone for this graph
            el_alive = false;
            continue;
        }
        if (h->seg_slot[c] < 0) {  // a column that came with these rows
            edges_tmp[0] = e;
            new_segment(c, std::min(64, 1 + el_slack(h, c, 1)), edges_tmp, 1);
        } else if (d_old < h->seg_cap[c]) {
            set_slot(2 * (size_t)(h->seg_slot[c] + d_old), e);
        } else {  // the segment is full: the column moves to a larger one, its old lanes go dead
            const int s_old = h->seg_slot[c];
            for (int k = 0; k < d_old; k++) edges_tmp[k] = h->h_el_slots[2 * (size_t)(s_old + k)];
            edges_tmp[d_old] = e;
            for (int k = 0; k < d_old; k++) set_slot(2 * (size_t)(s_old + k), -1);  // (the free lanes hold -1 already)
            set_slot(2 * (size_t)s_old + 1, 0);  // no head, no column: the other lanes of the old segment just idle
            new_segment(c, std::min(64, d_old + 1 + std::max(el_slack(h, c, d_old + 1), (d_old + 1) / 2)), edges_tmp, d_old + 1);
        }
    }
    if (el_alive)
        for (int c = n0; c < new_n; c++)  // new columns no appended row touches: isolated variables still have a posterior
            if (h->seg_slot[c] < 0) new_segment(c, 1, edges_tmp, 0);

    h->m = m0 + nrows;
    h->n = new_n;
    h->E = E0 + add;
    h->el_ok = h->E > 0 && h->max_row_deg <= ROW_CAP && h->max_col_deg <= 64;
    if (had_tables && (!el_alive || !h->el_ok)) {
        h->d_el_tab.reset();
        h->d_el_slots = h->d_el_slot_col = nullptr;
        el_alive = false;
    }

    TMARK("app:tables");
    // ---- device: CSR tails, table words -----------------------------------------------------------
    const bool reupload = el_alive && h->el_waves > h->el_cap_bins;  // the bins outgrew the device table
    const size_t npairs = (el_alive && !reupload) ? dirty_slot.size() + dirty_col.size() : 0;
    const size_t stage_ints = (size_t)nrows + add + 2 * npairs;
    if (stage_ints > h->d_pairs.cap()) {  // (d_pairs is requested last: its capacity is the pair's)
        h->h_pairs.reset();
        h->d_pairs.reset();
        const size_t want = stage_ints + stage_ints / 2 + 1024;
        SC_TRY(h->h_pairs.ensure(want));
        SC_TRY(h->d_pairs.ensure(want));
    }
    int *st = h->h_pairs;
    for (int r = 0; r < nrows; r++) st[r] = (int)(E0 + row_ptr[r + 1]);
    std::copy(col_idx, col_idx + add, st + nrows);
    if (nrows) SC_HIP(hipMemcpyAsync(h->d_row_ptr + m0 + 1, st, sizeof(int) * nrows, hipMemcpyHostToDevice, s));
    if (add) SC_HIP(hipMemcpyAsync(h->d_col_idx + E0, st + nrows, sizeof(int) * add, hipMemcpyHostToDevice, s));
    if (reupload) {
        SC_TRY(el_upload(h));
    } else if (npairs) {
        int *pp = st + nrows + add;
        const int col_base = (int)el_col_off(h);
        size_t q = 0;
        for (int i : dirty_slot) {
            pp[2 * q] = i;
            pp[2 * q + 1] = h->h_el_slots[i];
            q++;
        }
        for (int i : dirty_col) {
            pp[2 * q] = col_base + i;
            pp[2 * q + 1] = h->h_el_col[i];
            q++;
        }
        SC_HIP(hipMemcpyAsync(h->d_pairs, pp, sizeof(int) * 2 * npairs, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_apply_pairs, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, s, h->d_el_tab,
                           (const int2 *)h->d_pairs.get(), (int)npairs);
        LAUNCH_CHECK();
    }
    SC_HIP(hipStreamSynchronize(s));
    TMARK("app:device");

    // ---- what was sized or derived for the old graph ------------------------------------------------
    h->full_stale = true;  // CSC, degree buckets, identity block, tile tables: rebuilt when the tile / LDS kernels are next needed
    h->h_probs.resize(new_n, 0.0);
    h->thr_valid = false;
    h->first_valid = false;
    h->settle_next = 0;  // (the settle horizon was learned on the priors and rows that were: learn again)
    h->sparse_start_next = 0;
    h->ratio_valid = false;
    h->d_x64.reset();
    h->d_c64.reset();
    h->d_post64.reset();
    h->d_thr.reset();
    h->d_msg.reset();
    h->d_scratch.reset();
    h->cap_group = 0;
    h->d_rec.reset();
    h->d_mask.reset();
    h->cap_rec_group = 0;
    for (auto &L : h->lv) {
        L.synd.reset(); L.hard.reset(); L.done.reset(); L.conv.reset(); L.unsat.reset();
        L.iters.reset(); L.ids.reset(); L.post.reset(); L.pprior.reset(); L.pratio64.reset();
        L.cap_tiles = 0;
    }
    h->last_group = 0;
    TMARK("app:tail");
    unfinished.done = true;
    return 0;
}

int scaldpc_bp_last_compacted(scaldpc_bp *h, int64_t *count)
{
    if (!h || !count) return fail(SCALDPC_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *count = h->stat_deferred;
    return 0;
}

int scaldpc_bp_last_stats(scaldpc_bp *h, int64_t *out)
{
    if (!h || !out) return fail(SCALDPC_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->stat_deferred;
    out[1] = h->stat_el;
    out[2] = h->stat_levels;
    out[3] = 0;
    return 0;
}

int scaldpc_bp_last_schedule(scaldpc_bp *h, int64_t *out)
{
    if (!h || !out) return fail(SCALDPC_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    for (int i = 0; i < SCHED_WORDS; i++) out[i] = h->sched.w[i];
    for (int i = SCHED_WORDS; i < SCALDPC_SCHEDULE_WORDS; i++) out[i] = 0;
    return 0;
}

int scaldpc_bp_last_settle(scaldpc_bp *h, int32_t *frozen_at, int32_t cap, int64_t *info)
{
    if (!h || !info || cap < 0 || (cap > 0 && !frozen_at)) return fail(SCALDPC_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t T = h->settle_frozen_at.size();
    for (size_t t = 0; t < T && t < (size_t)cap; t++) frozen_at[t] = h->settle_frozen_at[t];
    info[0] = (int64_t)T;
    info[1] = h->settle_saved;
    info[2] = h->settle_rerun;
    info[3] = h->settle_K;
    return 0;
}

int scaldpc_bp_debug_sparse_flags(scaldpc_bp *h, int32_t tile, uint32_t *row_stamp, uint64_t *row_dirty, uint32_t *col_flag, int64_t *info)
{
    if (!h || !info || tile < 0) return fail(SCALDPC_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    info[0] = h->sparse_T;
    info[1] = h->sparse_m;
    info[2] = h->sparse_n;
    info[3] = h->sparse_start;
    if (!row_stamp && !row_dirty && !col_flag) return 0;
    if (tile >= h->sparse_T || !row_stamp || !row_dirty || !col_flag) return fail(SCALDPC_EINVAL, "no sparse flags for that tile");
    DeviceGuard dev(h->device);
    const int m = h->sparse_m, n = h->sparse_n;
    std::vector<uint4> rows((size_t)m);
    // (a debug entry, after a synchronous call: blocking copies)
    if (m) SC_HIP(hipMemcpy(rows.data(), h->d_rowf + (size_t)tile * m, sizeof(uint4) * (size_t)m, hipMemcpyDeviceToHost));
    if (n) SC_HIP(hipMemcpy(col_flag, h->d_colf + (size_t)tile * n, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost));
    for (int r = 0; r < m; r++) {
        row_stamp[r] = rows[(size_t)r].x;
        row_dirty[r] = ((uint64_t)rows[(size_t)r].w << 32) | rows[(size_t)r].z;
    }
    return 0;
}

int scaldpc_bp_set_tile_group(scaldpc_bp *h, int32_t tiles)
{
    if (!h || tiles < 0) return fail(SCALDPC_EINVAL, "bad tile group");
    std::lock_guard<std::mutex> lk(h->mu);
    h->tile_group = tiles;
    return 0;
}

// Tile group (c.G) and workspace of a call on the tile path.  prob_cols > 0: the last prob_cols columns bring per-codeword priors
// (scaldpc_bp_decode_batch_soft, scaldpc_mc_hqc_run_soft), whose plane h->d_pprior is sized here too.
static int size_call(scaldpc_bp *h, DecodeCall &c, int prob_cols)
{
    if (prob_cols > 0 && h->tile_group <= 0) {
        // the plane's rows share the cache with the group's messages where its passes keep reading them: every pass of an
        // early-exit run and every message-form pass reads all of them, a record-form pass without output only the
        // columns of degree >= 2 (launch_var: `light`)
        int cols = prob_cols;
        if (!c.early && rec_form(h, c.method)) {
            cols = 0;
            for (int v = h->n - prob_cols; v < h->n; v++) cols += h->hg_cdeg[v] > 1;
        }
        c.G = auto_group(h, c.T, cols);
    }
    return ensure_workspace(h, c.T, c.G, c.want_post, c.max_iter, prob_cols);
}

// Both decode entry points.  probs / prob_cols: a soft call's per-codeword probabilities of the last prob_cols columns
// (float [batch][prob_cols], where `in` lives); prob_cols = 0: the handle's shared priors, the plain call.
static int decode_batch_impl(scaldpc_bp *h, const uint8_t *in, int32_t input_kind, int32_t batch, const float *probs,
                             int32_t prob_cols, int32_t max_iter_arg, int32_t method, float alpha, uint32_t flags, void *stream,
                             uint8_t *out_bits, float *out_llr, int32_t *out_iters, uint8_t *out_conv)
{
    if (!h || !in || !out_bits) return fail(SCALDPC_EINVAL, "NULL argument");
    if (batch <= 0) return fail(SCALDPC_EINVAL, "batch must be positive (got %d)", batch);
    if (input_kind != SCALDPC_IN_SYNDROME && input_kind != SCALDPC_IN_RECEIVED)
        return fail(SCALDPC_EINVAL, "unknown input kind %d", input_kind);
    if (method != SCALDPC_BP_PRODUCT_SUM && method != SCALDPC_BP_MIN_SUM)
        return fail(SCALDPC_EINVAL, "unknown bp method %d", method);
    if (!(alpha >= 0.0f)) return fail(SCALDPC_EINVAL, "ms_scaling_factor must be >= 0");
    std::lock_guard<std::mutex> lk(h->mu);
    SC_TRY(check_usable(h));
    if (prob_cols > h->n) return fail(SCALDPC_EINVAL, "prob_cols = %d exceeds the block length n = %d", prob_cols, h->n);
    DeviceGuard dg(h->device);
    DecodeCall c;
    SC_TRY(begin_call(h, batch, max_iter_arg, stream, &c));
    const bool dev_io = flags & SCALDPC_F_DEVICE_IO;
    const bool early = flags & SCALDPC_F_EARLY_EXIT;
    if ((flags & SCALDPC_F_ASYNC) && (!dev_io || early))
        return fail(SCALDPC_EINVAL, "SCALDPC_F_ASYNC needs DEVICE_IO and no EARLY_EXIT (early exit polls the device)");
    if (flags & SCALDPC_F_ASYNC) h->async_used = true;
    c.method = method;
    c.alpha = alpha;
    c.early = early;
    c.want_post = out_llr != nullptr;
    c.no_sync = (flags & SCALDPC_F_ASYNC) != 0;  // (such a call only enqueues: no read-back of settled tiles, no horizon)
    CacheBypass guard(h->async_used);
    const hipStream_t s = c.s;
    SyncOnError settle{s};
    const int T = c.T, max_iter = c.max_iter;
    const int len = input_kind == SCALDPC_IN_SYNDROME ? h->m : h->n;
    const Outputs out{out_bits, out_llr, out_iters, out_conv};
    Outputs dev;
    const bool soft = prob_cols > 0;
    const int first_col = h->n - prob_cols;
    // host probabilities are checked before anything is enqueued (device ones by the conversion kernel: soft_verdict)
    if (soft && !dev_io)
        for (size_t i = 0, cnt = (size_t)batch * prob_cols; i < cnt; i++)
            if (!(probs[i] >= 0.0f && probs[i] <= 1.0f))
                return fail(SCALDPC_EINVAL, "channel_probs[%zu][%zu] = %g is not a probability (codeword %zu, column %zu)",
                            i / prob_cols, i % prob_cols, (double)probs[i], i / prob_cols, first_col + i % prob_cols);

    // Small graph: the LDS-resident single-launch decoder (k_bp_small).
    const size_t lds = small_lds(h);
    if (h->full_stale && (lds || !(T == 1 && batch <= el_limit(h, method))))  // rows were appended: only the row-parallel path is up to date
        SC_TRY(refresh_full(h));
    if (h->kn.path == Knobs::LDS && !lds)  // "stream" / "edge" / "lds" pin a path (tests)
        return fail(SCALDPC_EINVAL, "SCALDPC_PATH=lds but the graph needs %zu B of LDS", small_lds_bytes(h));
    // a soft call: probabilities -> the LLR plane h->d_pprior (enqueued once the plane is allocated) ...
    auto soft_convert = [&]() -> int {
        const float *dp = probs;
        const size_t cnt = (size_t)batch * prob_cols;
        if (!dev_io) {
            SC_TRY(grow(h->d_probs_in, cnt));
            SC_HIP(hipMemcpyAsync(h->d_probs_in, probs, sizeof(float) * cnt, hipMemcpyHostToDevice, s));
            dp = h->d_probs_in;
        }
        SC_TRY(h->d_soft_bad.ensure(1));
        SC_HIP(hipMemsetAsync(h->d_soft_bad, 0xff, sizeof(u64), s));
        hipLaunchKernelGGL(k_soft_convert, dim3((prob_cols + 63) / 64, T), dim3(256), 0, s, dp, prob_cols, batch, h->d_pprior.get(),
                           h->d_soft_bad.get());
        LAUNCH_CHECK();
        return 0;
    };
    // ... and what the conversion kernel found, at the call's synchronise (an SCALDPC_F_ASYNC call does not look)
    auto soft_verdict = [&]() -> int {
        u64 bad = ~0ull;
        SC_HIP(hipMemcpyAsync(&bad, h->d_soft_bad, sizeof(u64), hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
        if (bad != ~0ull)
            return fail(SCALDPC_EINVAL, "channel_probs[%llu][%llu] is not a probability (codeword %llu, column %llu)", bad / prob_cols,
                        bad % prob_cols, bad / prob_cols, first_col + bad % prob_cols);
        return 0;
    };
    if (lds) {
        const uint8_t *din = in;
        SC_TRY(stage_input(h, in, (size_t)batch * len, dev_io, s, &din));
        SC_TRY(stage_outputs(h, out, batch, dev_io, true, &dev));
        if (soft) {
            SC_TRY(grow(h->d_pprior, (size_t)T * prob_cols * TW));
            SC_TRY(soft_convert());
        }
        SC_TRY(launch_small<false>(h, lds, method, batch, din, input_kind, max_iter, alpha, early, dev.bits, dev.llr, dev.iters,
                                   dev.conv, s, soft ? h->d_pprior.get() : nullptr, first_col));
        SC_TRY(copy_outputs(h, out, dev, batch, dev_io, s));
        h->stat_deferred = 0;
        if (soft && !(flags & SCALDPC_F_ASYNC)) SC_TRY(soft_verdict());
        if (!(flags & SCALDPC_F_ASYNC)) SC_HIP(hipStreamSynchronize(s));
        return settle.done();
    }
    SC_TRY(size_call(h, c, prob_cols));
    if (soft) SC_TRY(soft_convert());
    const float *const pprior = soft ? h->d_pprior.get() : nullptr;

    // ---- a handful of codewords from host buffers: fused reshaping, one copy each way ------------------
    if (!dev_io && T == 1 && batch <= 8 && max_iter <= 1024) {
        const size_t bits_bytes = ((size_t)batch * h->n + 3) / 4 * 4;
        const size_t out_bytes = bits_bytes + (out_llr ? sizeof(float) * (size_t)batch * h->n : 0) + sizeof(int) * batch + batch;
        const size_t in_bytes = (size_t)batch * len, io_bytes = std::max(in_bytes, out_bytes);
        SC_TRY(h->h_io.ensure(io_bytes, io_bytes + io_bytes / 2));
        SC_TRY(grow(h->d_in, in_bytes));
        SC_TRY(grow(h->d_out_all, out_bytes));
        SC_TRY(ensure_el_unsat(h, max_iter));
        memcpy(h->h_io, in, in_bytes);
        SC_HIP(hipMemcpyAsync(h->d_in, h->h_io, in_bytes, hipMemcpyHostToDevice, s));
        const bool recvd = input_kind == SCALDPC_IN_RECEIVED;
        hipLaunchKernelGGL(k_small_prepare, dim3((std::max(len, h->n) + 63) / 64), dim3(256), 0, s, h->d_in, len, batch,
                           recvd ? h->d_recv : h->d_synd, h->n, h->d_hard, max_iter, h->d_done, h->d_conv, h->d_iters,
                           h->d_remaining, max_iter + 2, h->d_el_unsat, (max_iter + 2) * TW);
        LAUNCH_CHECK();
        if (recvd) SC_TRY(launch_syndrome(h, h->d_recv, h->d_synd, 1, s));
        c.state_ready = true;  // (k_small_prepare has reset the state planes and both counter arrays)
        SC_TRY(run_core(h, c, pprior, first_col));
        hipLaunchKernelGGL(k_small_unpack, dim3((h->n + 255) / 256), dim3(256), 0, s, h->d_hard, recvd ? h->d_recv : (const u64 *)nullptr,
                           out_llr ? h->d_post : (const float *)nullptr, h->d_conv, h->d_iters, h->n, batch, h->d_out_all);
        LAUNCH_CHECK();
        SC_HIP(hipMemcpyAsync(h->h_io, h->d_out_all, out_bytes, hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
        const uint8_t *o = h->h_io;
        memcpy(out_bits, o, (size_t)batch * h->n);
        o += bits_bytes;
        if (out_llr) {
            memcpy(out_llr, o, sizeof(float) * (size_t)batch * h->n);
            o += sizeof(float) * (size_t)batch * h->n;
        }
        if (out_iters) memcpy(out_iters, o, sizeof(int) * batch);
        if (out_conv) memcpy(out_conv, o + sizeof(int) * batch, batch);
        return settle.done();
    }

    // ---- stage input --------------------------------------------------------
    const uint8_t *din = in;
    SC_TRY(stage_input(h, in, (size_t)batch * len, dev_io, s, &din));
    if (input_kind == SCALDPC_IN_SYNDROME) {
        hipLaunchKernelGGL(k_pack_bits, dim3((h->m + 63) / 64, T), dim3(256), 0, s, din, h->m, batch, h->d_synd);
        LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(k_pack_bits, dim3((h->n + 63) / 64, T), dim3(256), 0, s, din, h->n, batch, h->d_recv);
        LAUNCH_CHECK();
        SC_TRY(launch_syndrome(h, h->d_recv, h->d_synd, T, s));
    }
    SC_TRY(run_core(h, c, pprior, first_col));

    // ---- outputs --------------------------------------------------------------
    SC_TRY(stage_outputs(h, out, batch, dev_io, true, &dev));
    hipLaunchKernelGGL(k_unpack_bits, dim3((h->n + 255) / 256, T), dim3(256), 0, s, h->d_hard,
                       input_kind == SCALDPC_IN_RECEIVED ? h->d_recv : (const u64 *)nullptr, h->n, batch, dev.bits);
    LAUNCH_CHECK();
    if (out_llr) {
        hipLaunchKernelGGL(k_unpack_llr, dim3((h->n + 63) / 64, T), dim3(256), 0, s, h->d_post, h->n, batch, dev.llr);
        LAUNCH_CHECK();
    }
    if (dev.iters || dev.conv) {
        hipLaunchKernelGGL(k_unpack_state, dim3(T), dim3(64), 0, s, h->d_conv, h->d_iters, batch, dev.iters, dev.conv);
        LAUNCH_CHECK();
    }
    SC_TRY(copy_outputs(h, out, dev, batch, dev_io, s));
    if (soft && !(flags & SCALDPC_F_ASYNC)) SC_TRY(soft_verdict());
    if (!(flags & SCALDPC_F_ASYNC)) SC_HIP(hipStreamSynchronize(s));
    return settle.done();
}

int scaldpc_bp_decode_batch(scaldpc_bp *h, const uint8_t *in, int32_t input_kind, int32_t batch, int32_t max_iter,
                            int32_t method, float alpha, uint32_t flags, void *stream, uint8_t *out_bits,
                            float *out_llr, int32_t *out_iters, uint8_t *out_conv)
{
    return decode_batch_impl(h, in, input_kind, batch, nullptr, 0, max_iter, method, alpha, flags, stream, out_bits, out_llr,
                             out_iters, out_conv);
}

int scaldpc_bp_decode_batch_soft(scaldpc_bp *h, const uint8_t *in, int32_t input_kind, int32_t batch, const float *probs,
                                 int32_t prob_cols, int32_t max_iter, int32_t method, float alpha, uint32_t flags, void *stream,
                                 uint8_t *out_bits, float *out_llr, int32_t *out_iters, uint8_t *out_conv)
{
    if (!h || !probs) return fail(SCALDPC_EINVAL, "NULL argument");
    if (prob_cols < 1) return fail(SCALDPC_EINVAL, "prob_cols = %d: at least one column", prob_cols);
    return decode_batch_impl(h, in, input_kind, batch, probs, prob_cols, max_iter, method, alpha, flags, stream, out_bits, out_llr,
                             out_iters, out_conv);
}

// ---------------------------------------------------------------------------
// The reference's own arithmetic: product-sum in the probability-ratio domain, float64 (kernels: scaldpc_bp_ref64.h)
// ---------------------------------------------------------------------------
// every REF64_POLL-th iteration of an early-exit tile group the host reads "codewords still running" and stops the group
// at 0 (iterations enqueued for a group that has finished return at once: their tiles are frozen)
static constexpr int REF64_POLL = 4;

// tiles per group of the float64 loop: the handle's group_mb budget with 8-byte messages in two arrays, at least one tile
static int ref64_group(const scaldpc_bp *h, int T)
{
    if (h->tile_group > 0) return std::min(h->tile_group, T);
    const double per_tile = (double)h->E * TW * sizeof(double) * 2;
    const int g = per_tile > 0 ? (int)(h->kn.group_mb * 1e6 / per_tile) : T;
    return std::max(1, std::min(g, T));
}

// the shared priors as ratios r = p / (1 - p), in double from the handle's float64 mirror (p = 0 -> 0, p = 1 -> inf)
static int ensure_ratio64(scaldpc_bp *h)
{
    if (h->ratio_valid && h->d_ratio) return 0;
    h->ratio_valid = false;
    pvec<double> r(h->n);
    for (int j = 0; j < h->n; j++) {
        const double p = h->h_probs[j];
        r[j] = p / (1.0 - p);
    }
    SC_TRY(grow(h->d_ratio, (size_t)h->n));
    SC_HIP(hipMemcpy(h->d_ratio, r.data(), sizeof(double) * h->n, hipMemcpyHostToDevice));
    h->ratio_valid = true;
    return 0;
}

// What the float64 loop needs on the device for a call of T tiles in groups of G: the shared ratios, the state planes, both
// message arrays, the "still running" counters, and on request the posterior plane and the per-codeword ratio plane.
static int ref64_ensure(scaldpc_bp *h, int T, int G, int max_iter, bool want_post, int prob_cols)
{
    SC_TRY(ensure_ratio64(h));
    SC_TRY(ensure_workspace(h, T, G, false, max_iter));
    SC_TRY(h->d_x64.ensure((size_t)G * h->E * TW));
    SC_TRY(h->d_c64.ensure((size_t)G * h->E * TW));
    if (want_post) SC_TRY(h->d_post64.ensure((size_t)T * h->n * TW));
    SC_TRY(h->d_rem64.ensure((size_t)max_iter + 2));
    SC_TRY(h->h_rem64.ensure(1));
    if (prob_cols) SC_TRY(grow(h->d_pratio, (size_t)T * prob_cols * TW));
    return 0;
}

// The planes a float64 loop runs on: the call's own (h->d_synd ...), or the dense tiles of its stragglers (h->lv[1]).
//   synd [tile][m], hard [tile][n], done / conv [tile], unsat [tile][parity_waves], iters [tile][64]
//   post    double [tile][n][64] or null
//   pratio  double [tile][prob_cols][64]: the per-codeword ratios of the last prob_cols columns; null = the shared priors
struct Ref64Planes {
    const u64 *synd;
    u64 *hard, *done, *conv, *unsat;
    int *iters;
    double *post;
    const double *pratio;
    int prob_cols;
};

// T tiles, one tile group after the other; per iteration check pass, variable pass, test + latch.  Every group runs the
// iterations 1 .. stop_at of a decode of max_iter (stop_at = max_iter: the whole decode; less: an early-exit call that hands its
// stragglers over after stop_at, ref64_handover).
static int ref64_iterate(scaldpc_bp *h, const Ref64Planes &p, int T, int G, int max_iter, int stop_at, bool early, hipStream_t s)
{
    const int n = h->n, m = h->m, pw = parity_waves(h), first_col = n - p.prob_cols;
    const long E = h->E;
    for (int g0 = 0; g0 < T; g0 += G) {
        const int g = std::min(G, T - g0);
        const Ratio64 prior{h->d_ratio, p.pratio ? p.pratio + (size_t)g0 * p.prob_cols * TW : nullptr, first_col,
                            p.pratio ? p.prob_cols : 0};
        const u64 *synd = p.synd + (size_t)g0 * m, *done = p.done + g0;
        u64 *hard = p.hard + (size_t)g0 * n;
        double *post = p.post ? p.post + (size_t)g0 * n * TW : nullptr;
        if (E) {
            hipLaunchKernelGGL(k_init_ratio64, dim3((unsigned)((E + 3) / 4), g), dim3(256), 0, s, h->d_col_idx, h->d_x64.get(), E,
                               prior);
            LAUNCH_CHECK();
        }
        if (early) SC_HIP(hipMemsetAsync(h->d_rem64, 0, sizeof(int) * ((size_t)max_iter + 2), s));
        for (int it = 1; it <= stop_at; it++) {
            const bool last = it == max_iter;
            if (E) {
                // (the register-resident width the launch is built for: the smallest that holds the widest row)
                auto check = h->max_row_deg <= 16 ? k_check_ratio64<16> : h->max_row_deg <= 52 ? k_check_ratio64<52>
                                                                                              : k_check_ratio64<REF64_ROW_CAP>;
                hipLaunchKernelGGL(check, dim3((m + 3) / 4, g), dim3(256), 0, s, h->d_row_ptr, h->d_x64.get(), h->d_c64.get(), E, m,
                                   synd, done);
                LAUNCH_CHECK();
            }
            auto var = h->max_col_deg <= 16 ? k_var_ratio64<16> : k_var_ratio64<REF64_COL_CAP>;
            hipLaunchKernelGGL(var, dim3((n + 3) / 4, g), dim3(256), 0, s, h->d_col_ptr, h->d_csc_edge, h->d_c64.get(),
                               h->d_x64.get(), E, n, prior, done, (early || last) ? 1 : 0, hard, post);
            LAUNCH_CHECK();
            if (!early && !last) continue;
            hipLaunchKernelGGL(k_parity_fin, dim3(parity_blocks(m), g), dim3(256), 0, s, h->d_row_ptr, h->d_col_idx, hard, m, n,
                               synd, p.unsat + (size_t)g0 * pw, pw, it, early ? 1 : 0, p.done + g0, p.conv + g0,
                               p.iters + (size_t)g0 * TW, h->d_rem64 + it);
            LAUNCH_CHECK();
            if (early && it < stop_at && it % REF64_POLL == 0) {
                SC_HIP(hipMemcpyAsync(h->h_rem64, h->d_rem64 + it, sizeof(int), hipMemcpyDeviceToHost, s));
                SC_HIP(hipStreamSynchronize(s));
                if (h->h_rem64[0] == 0) break;
            }
        }
    }
    return 0;
}

// state of `batch` codewords in T tiles before their first iteration
static int ref64_reset(scaldpc_bp *h, const Ref64Planes &p, int batch, int T, int max_iter, hipStream_t s)
{
    hipLaunchKernelGGL(k_init_state, dim3(T), dim3(64), 0, s, batch, max_iter, p.done, p.conv, p.iters);
    LAUNCH_CHECK();
    SC_HIP(hipMemsetAsync(p.hard, 0, sizeof(u64) * (size_t)T * h->n, s));
    SC_HIP(hipMemsetAsync(p.unsat, 0, sizeof(u64) * (size_t)T * parity_waves(h), s));  // k_parity_fin leaves its words zero
    return 0;
}

// The hand-over of the float64 sweeps, ONE level and one rule: every group of the call has stopped after iteration k; all
// codewords not latched by then are gathered, over the whole call, into dense tiles of their own (h->lv[1]: syndromes, and the
// rows of the ratio plane that go with them), decoded there from iteration 1 for max_iter iterations by the same loop on the
// same message arrays, and their decisions, iteration counts and converged bits are scattered back.  Codewords are independent
// and the recursion is deterministic: the results are those of the loop without hand-over, bit for bit.
static int ref64_handover(scaldpc_bp *h, const Ref64Planes &p, int batch, int T, int G, int max_iter, hipStream_t s)
{
    std::vector<u64> done_h(T);
    SC_HIP(hipMemcpyAsync(done_h.data(), p.done, sizeof(u64) * T, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    pvec<int> ids, slot_of((size_t)T * TW, -1);
    for (long b = 0; b < batch; b++)
        if (!((done_h[b >> 6] >> (b & 63)) & 1)) {
            slot_of[b] = (int)ids.size();
            ids.push_back((int)b);
        }
    const int batch2 = (int)ids.size();
    if (batch2 == 0) return 0;
    h->stat_deferred = batch2;
    h->stat_levels = 1;
    const int T2 = (batch2 + TW - 1) / TW;
    ids.resize((size_t)T2 * TW, -1);
    scaldpc_bp::Level &L = h->lv[1];
    SC_TRY(ensure_level(h, L, T2));
    SC_TRY(grow(L.slot_of, (size_t)T * TW));
    if (p.pratio) SC_TRY(grow(L.pratio64, (size_t)T2 * p.prob_cols * TW));
    SC_HIP(hipMemcpyAsync(L.ids, ids.data(), sizeof(int) * ids.size(), hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(L.slot_of, slot_of.data(), sizeof(int) * slot_of.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_gather_planes, dim3((h->m + 63) / 64, T2), dim3(256), 0, s, p.synd, h->m, L.ids, L.synd);
    LAUNCH_CHECK();
    if (p.pratio) {  // the stragglers' ratios go with them
        SC_TRY(launch_gather_prior64(p.pratio, p.prob_cols, L.ids, L.pratio64, T2, s));
    }
    const Ref64Planes p2{L.synd, L.hard, L.done, L.conv, L.unsat, L.iters, nullptr, p.pratio ? L.pratio64.get() : nullptr,
                         p.prob_cols};
    SC_TRY(ref64_reset(h, p2, batch2, T2, max_iter, s));
    SC_HIP(hipStreamSynchronize(s));  // ids / slot_of are locals
    SC_TRY(ref64_iterate(h, p2, T2, std::min(G, T2), max_iter, max_iter, true, s));
    hipLaunchKernelGGL(k_scatter_planes, dim3((h->n + 63) / 64, T), dim3(256), 0, s, p.hard, h->n, L.slot_of, L.hard);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scatter_state, dim3(T), dim3(64), 0, s, p.iters, p.conv, L.slot_of, L.iters, L.conv);
    LAUNCH_CHECK();
    return 0;
}

// The float64 decode proper, on inputs already staged as planes (p.synd, p.pratio): state reset, then the loop.  Results stay on
// the device (p.hard / post / conv / iters).  handover_at = k > 0 (the sweeps, early exit, max_iter > k): every group stops after
// iteration k and the stragglers are re-decoded in dense tiles; 0: every group runs to its end (scaldpc_bp_decode_batch_f64
// always; fixed-iteration sweeps; the knob "compact_after" = 0).
static int ref64_run(scaldpc_bp *h, const Ref64Planes &p, int batch, int T, int G, int max_iter, bool early, int handover_at,
                     hipStream_t s)
{
    SC_TRY(ref64_reset(h, p, batch, T, max_iter, s));
    h->last_group = 0;
    h->stat_deferred = 0;
    h->stat_el = 0;
    h->stat_levels = 0;
    const bool hand = early && handover_at > 0 && max_iter > handover_at && !p.post;
    SC_TRY(ref64_iterate(h, p, T, G, max_iter, hand ? handover_at : max_iter, early, s));
    if (hand) SC_TRY(ref64_handover(h, p, batch, T, G, max_iter, s));
    return 0;
}

int scaldpc_bp_decode_batch_f64(scaldpc_bp *h, const uint8_t *in, int32_t input_kind, int32_t batch, const double *probs,
                                int32_t prob_cols, int32_t max_iter_arg, uint32_t flags, void *stream, uint8_t *out_bits,
                                double *out_llr, int32_t *out_iters, uint8_t *out_conv)
{
    if (!h || !in || !out_bits) return fail(SCALDPC_EINVAL, "NULL argument");
    if (batch <= 0) return fail(SCALDPC_EINVAL, "batch must be positive (got %d)", batch);
    if (input_kind != SCALDPC_IN_SYNDROME && input_kind != SCALDPC_IN_RECEIVED)
        return fail(SCALDPC_EINVAL, "unknown input kind %d", input_kind);
    if (flags & SCALDPC_F_ASYNC) return fail(SCALDPC_EINVAL, "SCALDPC_F_ASYNC: the float64 decode is synchronous");
    if (prob_cols < 0 || (probs != nullptr) != (prob_cols > 0))
        return fail(SCALDPC_EINVAL, "probs and prob_cols = %d go together (NULL and 0: the handle's shared priors)", prob_cols);
    std::lock_guard<std::mutex> lk(h->mu);
    SC_TRY(check_usable(h));
    if (prob_cols > h->n) return fail(SCALDPC_EINVAL, "prob_cols = %d exceeds the block length n = %d", prob_cols, h->n);
    DeviceGuard dg(h->device);
    DecodeCall c;
    SC_TRY(begin_call(h, batch, max_iter_arg, stream, &c));
    const bool dev_io = flags & SCALDPC_F_DEVICE_IO;
    const bool early = flags & SCALDPC_F_EARLY_EXIT;
    CacheBypass guard(h->async_used);
    const hipStream_t s = c.s;
    const int T = c.T, max_iter = c.max_iter, n = h->n, m = h->m;
    const int len = input_kind == SCALDPC_IN_SYNDROME ? m : n;
    const int first_col = n - prob_cols;
    // host probabilities are checked before anything is enqueued
    if (prob_cols && !dev_io)
        for (size_t i = 0, cnt = (size_t)batch * prob_cols; i < cnt; i++)
            if (!(probs[i] >= 0.0 && probs[i] <= 1.0))
                return fail(SCALDPC_EINVAL, "channel_probs[%zu][%zu] = %g is not a probability (codeword %zu, column %zu)",
                            i / prob_cols, i % prob_cols, probs[i], i / prob_cols, first_col + i % prob_cols);
    SyncOnError settle{s};
    SC_TRY(refresh_full(h));  // rows were appended: the CSC arrays follow
    const int G = ref64_group(h, T);
    SC_TRY(ref64_ensure(h, T, G, max_iter, out_llr != nullptr, prob_cols));
    const Outputs out{out_bits, nullptr, out_iters, out_conv};
    Outputs dev;
    SC_TRY(stage_outputs(h, out, batch, dev_io, true, &dev));
    double *dev_llr = out_llr;
    if (out_llr && !dev_io) {
        SC_TRY(grow(h->d_out_llr64, (size_t)batch * n));
        dev_llr = h->d_out_llr64;
    }

    // ---- per-codeword priors -> the ratio plane; a value that is no probability is refused before the decode starts ----
    if (prob_cols) {
        const double *dp = probs;
        const size_t cnt = (size_t)batch * prob_cols;
        if (!dev_io) {
            SC_TRY(grow(h->d_probs_in64, cnt));
            SC_HIP(hipMemcpyAsync(h->d_probs_in64, probs, sizeof(double) * cnt, hipMemcpyHostToDevice, s));
            dp = h->d_probs_in64;
        }
        SC_TRY(h->d_soft_bad.ensure(1));
        SC_HIP(hipMemsetAsync(h->d_soft_bad, 0xff, sizeof(u64), s));
        hipLaunchKernelGGL(k_ratio64_convert, dim3((prob_cols + 63) / 64, T), dim3(256), 0, s, dp, prob_cols, batch,
                           h->d_pratio.get(), h->d_soft_bad.get());
        LAUNCH_CHECK();
        if (dev_io) {  // (host values were checked above)
            u64 bad = ~0ull;
            SC_HIP(hipMemcpyAsync(&bad, h->d_soft_bad, sizeof(u64), hipMemcpyDeviceToHost, s));
            SC_HIP(hipStreamSynchronize(s));
            if (bad != ~0ull)
                return fail(SCALDPC_EINVAL, "channel_probs[%llu][%llu] is not a probability (codeword %llu, column %llu)",
                            bad / prob_cols, bad % prob_cols, bad / prob_cols, first_col + bad % prob_cols);
        }
    }

    // ---- input planes, state ----------------------------------------------------------------------------------------
    const uint8_t *din = in;
    SC_TRY(stage_input(h, in, (size_t)batch * len, dev_io, s, &din));
    if (input_kind == SCALDPC_IN_SYNDROME) {
        hipLaunchKernelGGL(k_pack_bits, dim3((m + 63) / 64, T), dim3(256), 0, s, din, m, batch, h->d_synd);
        LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(k_pack_bits, dim3((n + 63) / 64, T), dim3(256), 0, s, din, n, batch, h->d_recv);
        LAUNCH_CHECK();
        SC_TRY(launch_syndrome(h, h->d_recv, h->d_synd, T, s));
    }
    // ---- the loop: every tile group through all its iterations (no hand-over: the launches are the call's own) ----------
    const Ref64Planes pl{h->d_synd, h->d_hard, h->d_done, h->d_conv, h->d_unsat, h->d_iters, out_llr ? h->d_post64.get() : nullptr,
                         prob_cols ? h->d_pratio.get() : nullptr, prob_cols};
    SC_TRY(ref64_run(h, pl, batch, T, G, max_iter, early, 0, s));

    // ---- outputs ----------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL(k_unpack_bits, dim3((n + 255) / 256, T), dim3(256), 0, s, h->d_hard,
                       input_kind == SCALDPC_IN_RECEIVED ? h->d_recv : (const u64 *)nullptr, n, batch, dev.bits);
    LAUNCH_CHECK();
    if (out_llr) {
        hipLaunchKernelGGL(k_unpack_llr64, dim3((n + 63) / 64, T), dim3(256), 0, s, h->d_post64.get(), n, batch, dev_llr);
        LAUNCH_CHECK();
    }
    if (dev.iters || dev.conv) {
        hipLaunchKernelGGL(k_unpack_state, dim3(T), dim3(64), 0, s, h->d_conv, h->d_iters, batch, dev.iters, dev.conv);
        LAUNCH_CHECK();
    }
    SC_TRY(copy_outputs(h, out, dev, batch, dev_io, s));
    if (out_llr && !dev_io)
        SC_HIP(hipMemcpyAsync(out_llr, dev_llr, sizeof(double) * (size_t)batch * n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return settle.done();
}

// ---------------------------------------------------------------------------
// Monte-Carlo entry points (K6)
//
// Two sweeps, each written once.  mc_fer_body: draw an error, take its syndrome, decode, compare.  mc_hqc_body: draw a secret,
// take its syndrome, add noise to the checks, build the message, decode, then stats / bits / compare.  What the 13 entries
// differ in goes in as values: the trials (TrialSrc, scaldpc_trials.h: a range or a list), the decode (McDecode) and, for HQC,
// the noise (McHqcNoise) and the outputs (McHqcOut).  The trials are drawn by the same kernels whatever the decode -- precision
// is a property of the decode, not of the trial -- and it decides three things only: the order of the argument checks
// (mc_args), the sizing (mc_size) and the decode itself (mc_decode).
// ---------------------------------------------------------------------------
namespace {

// (bernoulli_threshold: scaldpc_mc_law.h)

// How a sweep's trials are decoded: by the fp32 kernels (run_core) with a method and its alpha, or in the reference's own
// arithmetic, the float64 ratio domain (ref64_run: product-sum only, so no method and no alpha).
struct McDecode {
    bool f64 = false;
    int32_t method = SCALDPC_BP_PRODUCT_SUM;
    float alpha = 0.0f;
    static McDecode fp32(int32_t method, float alpha) { return {false, method, alpha}; }
    static McDecode float64() { return {true}; }
};

// The noise on the checks of an HQC sweep.  table == false: every check is flipped with probability eps, and the decoder keeps
// the handle's shared priors.  table: every check draws an outcome of the caller's table (include/scaldpc.h states the law),
// which brings the reported bit, its prior into the call's plane, and -- with costs -- the oracle calls it spent.  probs is
// float [K] for an fp32 decode (mc_hqc_law), probs64 double [K] for a float64 one (mc_hqc_law64).
struct McHqcNoise {
    bool table = false;
    double eps = 0.0;
    const double *weights = nullptr;
    const uint8_t *flips = nullptr;
    const float *probs = nullptr;
    const double *probs64 = nullptr;
    const int32_t *costs = nullptr;
    int32_t K = 0;
    bool counted() const { return costs != nullptr; }
    static McHqcNoise flip(double eps) { return {false, eps}; }
    static McHqcNoise drawn(const double *weights, const uint8_t *flips, const float *probs, const int32_t *costs, int32_t K)
    {
        return {true, 0.0, weights, flips, probs, nullptr, costs, K};
    }
    static McHqcNoise drawn(const double *weights, const uint8_t *flips, const double *probs64, const int32_t *costs, int32_t K)
    {
        return {true, 0.0, weights, flips, nullptr, probs64, costs, K};
    }
};

// The outputs of an HQC sweep (null: not wanted; success is required).  The eps forms have the first four.
struct McHqcOut {
    uint8_t *success = nullptr;
    int32_t *iters = nullptr;
    uint8_t *msg = nullptr;
    int32_t *y = nullptr;
    uint8_t *outcome = nullptr;
    int32_t *flips = nullptr, *cost = nullptr, *stats = nullptr;
    uint8_t *bits = nullptr;
};

// the trial source's own refusals (scaldpc_trials.h); a list is looked at once batch is known to be positive
int mc_trials_arg(const TrialSrc &ts, int32_t batch)
{
    char why[96];
    if (!trials_ok(ts, batch, why, sizeof why)) return fail(SCALDPC_EINVAL, "%s", why);
    return 0;
}

// The refusals every sweep shares.  An fp32 entry looks at its pointers first and at method and alpha last; a float64 entry
// (no method, no alpha) looks at the handle last, so that every one of its refusals can be seen without a device.
int mc_args(const scaldpc_bp *h, const TrialSrc &ts, int32_t batch, const McDecode &d, uint32_t flags, const uint8_t *out_success)
{
    const bool null_arg = !h || !out_success;
    if (!d.f64 && null_arg) return fail(SCALDPC_EINVAL, "NULL argument");
    if (flags & ~(SCALDPC_F_EARLY_EXIT | SCALDPC_F_DEVICE_IO))
        return fail(SCALDPC_EINVAL, "flags: SCALDPC_F_EARLY_EXIT and SCALDPC_F_DEVICE_IO are taken");
    if (!ts.listed) SC_TRY(mc_trials_arg(ts, batch));
    if (batch <= 0) return fail(SCALDPC_EINVAL, "batch must be positive (got %d)", batch);
    if (ts.listed) SC_TRY(mc_trials_arg(ts, batch));
    if (null_arg) return fail(SCALDPC_EINVAL, "NULL argument");
    if (d.f64) return 0;
    if (d.method != SCALDPC_BP_PRODUCT_SUM && d.method != SCALDPC_BP_MIN_SUM)
        return fail(SCALDPC_EINVAL, "unknown bp method %d", d.method);
    if (!(d.alpha >= 0.0f)) return fail(SCALDPC_EINVAL, "ms_scaling_factor must be >= 0");
    return 0;
}

// the law of a table-form noise, in the decode's precision; every refusal of the table is here, and nothing touches the device
int mc_noise_law(const McHqcNoise &nz, bool f64, int R, bool want_cost, McHqcLaw *law, McHqcLaw64 *law64)
{
    char why[160];
    const int bad = f64 ? mc_hqc_law64(nz.weights, nz.flips, nz.probs64, nz.costs, nz.K, R, want_cost, law64, why, sizeof why)
                        : mc_hqc_law(nz.weights, nz.flips, nz.probs, nz.costs, nz.K, R, want_cost, law, why, sizeof why);
    return bad ? fail(SCALDPC_EINVAL, "%s", why) : 0;
}

// the Bernoulli thresholds of the shared priors (the FER sweeps' noise), built on first use
int ensure_thresholds(scaldpc_bp *h)
{
    if (h->thr_valid) return 0;
    if (!h->d_thr) SC_TRY(h->d_thr.ensure((size_t)h->n));
    pvec<u64> thr(h->n);
    for (int j = 0; j < h->n; j++) thr[j] = bernoulli_threshold(h->h_probs[j]);
    SC_HIP(hipMemcpy(h->d_thr, thr.data(), sizeof(u64) * h->n, hipMemcpyHostToDevice));
    h->thr_valid = true;
    return 0;
}

int mc_finish(scaldpc_bp *h, int batch, int T, int nv, bool dev_io, hipStream_t s, uint8_t *out_success,
              int32_t *out_iters)
{
    SC_TRY(grow(h->d_diff, (size_t)T));
    SC_HIP(hipMemsetAsync(h->d_diff, 0, sizeof(u64) * (size_t)T, s));
    hipLaunchKernelGGL(k_mc_compare, dim3((nv + 255) / 256, T), dim3(256), 0, s, h->d_hard, h->d_mc, h->n, nv,
                       h->d_diff);
    LAUNCH_CHECK();
    uint8_t *ds = out_success;
    if (!dev_io) {
        SC_TRY(grow(h->d_succ, (size_t)batch));
        ds = h->d_succ;
    }
    Outputs out, dev;
    out.iters = out_iters;
    SC_TRY(stage_outputs(h, out, batch, dev_io, out_iters != nullptr, &dev));
    hipLaunchKernelGGL(k_mc_result, dim3(T), dim3(64), 0, s, h->d_diff, h->d_iters, batch, ds, dev.iters);
    LAUNCH_CHECK();
    if (!dev_io) SC_HIP(hipMemcpyAsync(out_success, ds, (size_t)batch, hipMemcpyDeviceToHost, s));
    SC_TRY(copy_outputs(h, out, dev, batch, dev_io, s));
    SC_HIP(hipStreamSynchronize(s));
    return 0;
}

// planes (XOR xor_with, where given) -> uint8 [batch][n] for the caller.  last: no export of the call follows this one, so a
// host export need not wait for its copy before the staging block d_out_bits is used again (mc_finish synchronises).
int mc_export_bits(scaldpc_bp *h, const u64 *planes, const u64 *xor_with, int batch, int T, bool dev_io, bool last, hipStream_t s,
                   uint8_t *out)
{
    Outputs o, dev;
    o.bits = out;
    SC_TRY(stage_outputs(h, o, batch, dev_io, false, &dev));
    hipLaunchKernelGGL(k_unpack_bits, dim3((h->n + 255) / 256, T), dim3(256), 0, s, planes, xor_with, h->n, batch, dev.bits);
    LAUNCH_CHECK();
    SC_TRY(copy_outputs(h, o, dev, batch, dev_io, s));
    if (!dev_io && !last) SC_HIP(hipStreamSynchronize(s));  // d_out_bits is reused below
    return 0;
}

// The generators, from either source of trials (DeviceTrials, stage_trials: scaldpc_trials.h): a contiguous call enqueues the
// launch it always did.
int draw_bernoulli(bool xor_into, u64 *planes, int len, int batch, int T, const DeviceTrials &tr, unsigned k0, unsigned k1, const u64 *thr,
                   u64 thr0, hipStream_t s)
{
    if (tr.ids) return launch_mc_bernoulli_at(xor_into, planes, len, batch, T, tr.ids, 0u, k0, k1, thr, thr0, s);
    const dim3 grid((len + 63) / 64, T);
    if (xor_into)
        hipLaunchKernelGGL(k_mc_bernoulli<true>, grid, dim3(256), 0, s, planes, len, batch, tr.first, 0u, k0, k1, thr, thr0);
    else
        hipLaunchKernelGGL(k_mc_bernoulli<false>, grid, dim3(256), 0, s, planes, len, batch, tr.first, 0u, k0, k1, thr, thr0);
    LAUNCH_CHECK();
    return 0;
}
int draw_hqc_secret(scaldpc_bp *h, int N, int omega, int batch, int T, const DeviceTrials &tr, unsigned k0, unsigned k1, int *dy,
                    hipStream_t s)
{
    if (tr.ids) return launch_mc_hqc_secret_at(h->d_mc, h->n, N, omega, batch, T, tr.ids, k0, k1, dy, s);
    hipLaunchKernelGGL(k_mc_hqc_secret, dim3(T), dim3(64), (size_t)omega * 64 * sizeof(int), s, h->d_mc, h->n, N, omega, batch,
                       tr.first, k0, k1, dy);
    LAUNCH_CHECK();
    return 0;
}
// an outcome per check of the table's law: the reported bit into synd and its prior into the decode's plane -- the LLR into
// h->d_pprior (k_mc_hqc_outcome), or the ratio into h->d_pratio (k_mc_hqc_outcome64)
int draw_hqc_outcome(scaldpc_bp *h, bool f64, const McHqcLaw &law, const McHqcLaw64 &law64, int R, int batch, int T, const DeviceTrials &tr,
                     unsigned k0, unsigned k1, int *acc_flips, int *acc_cost, uint8_t *dout, hipStream_t s)
{
    if (f64 && tr.ids)
        return launch_mc_hqc_outcome64_at(law64, h->d_synd, h->d_pratio, R, batch, T, tr.ids, k0, k1, acc_flips, acc_cost, dout, s);
    if (f64) return launch_mc_hqc_outcome64(law64, h->d_synd, h->d_pratio, R, batch, T, tr.first, k0, k1, acc_flips, acc_cost, dout, s);
    if (tr.ids) return launch_mc_hqc_outcome_at(law, h->d_synd, h->d_pprior, R, batch, T, tr.ids, k0, k1, acc_flips, acc_cost, dout, s);
    hipLaunchKernelGGL(k_mc_hqc_outcome, dim3((R + 63) / 64, T), dim3(256), 0, s, law, h->d_synd.get(), h->d_pprior.get(), R, batch,
                       tr.first, k0, k1, acc_flips, acc_cost, dout);
    LAUNCH_CHECK();
    return 0;
}

// (mc_stage / mc_unstage, the staging of a sweep's optional outputs, are templates and stand with stage_outputs, ahead of the C ABI)

// the iteration after which an early-exit float64 sweep hands its stragglers over (0: never)
int mc_f64_handover_at(const scaldpc_bp *h) { return h->kn.compact_after < 0 ? 4 : h->kn.compact_after; }

// Tile group and workspace of a sweep whose last prob_cols columns bring per-trial priors (0: the handle's shared priors):
// size_call as decode_batch_impl sizes a soft call, or what scaldpc_bp_decode_batch_f64 sizes.
int mc_size(scaldpc_bp *h, DecodeCall &c, const McDecode &d, int prob_cols, bool early)
{
    c.method = d.method;  // (what the sweep decodes with; no posteriors)
    c.alpha = d.alpha;
    c.early = early;
    if (!d.f64) return size_call(h, c, prob_cols);
    c.G = ref64_group(h, c.T);
    return ref64_ensure(h, c.T, c.G, c.max_iter, false, prob_cols);
}

// The decode of a sweep on the planes its trial kernels have staged (h->d_synd, and with prob_cols the prior plane of the
// decode's precision): run_core, or scaldpc_bp_decode_batch_f64's loop (ref64_run), whose stragglers are handed over to dense
// tiles once, after iteration "compact_after" (ref64_handover).
int mc_decode(scaldpc_bp *h, const McDecode &d, const DecodeCall &c, int prob_cols)
{
    if (!d.f64) return run_core(h, c, prob_cols ? h->d_pprior.get() : nullptr, prob_cols ? h->n - prob_cols : 0);
    const Ref64Planes pl{h->d_synd, h->d_hard, h->d_done, h->d_conv, h->d_unsat, h->d_iters, nullptr,
                         prob_cols ? h->d_pratio.get() : nullptr, prob_cols};
    return ref64_run(h, pl, c.batch, c.T, c.G, c.max_iter, c.early, mc_f64_handover_at(h), c.s);
}

// Every FER entry: the trials from either source, decoded either way.
int mc_fer_body(scaldpc_bp *h, const TrialSrc &ts, int32_t batch, uint64_t seed, int32_t max_iter_arg, const McDecode &d, uint32_t flags,
                void *stream, uint8_t *out_success, int32_t *out_iters, uint8_t *out_error)
{
    SC_TRY(mc_args(h, ts, batch, d, flags, out_success));
    std::lock_guard<std::mutex> lk(h->mu);
    SC_TRY(check_usable(h));
    DeviceGuard dg(h->device);
    CacheBypass guard(h->async_used);
    DecodeCall c;
    SC_TRY(begin_call(h, batch, max_iter_arg, stream, &c));
    const hipStream_t s = c.s;
    SyncOnError settle{s};
    SC_TRY(refresh_full(h));
    const bool dev_io = flags & SCALDPC_F_DEVICE_IO, early = flags & SCALDPC_F_EARLY_EXIT;
    const int T = c.T;
    SC_TRY(mc_size(h, c, d, 0, early));
    SC_TRY(grow(h->d_mc, (size_t)T * h->n));
    SC_TRY(ensure_thresholds(h));
    DeviceTrials tr;
    SC_TRY(stage_trials(h->d_trial_ids, ts, batch, s, &tr));
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    // error ~ Bernoulli(p_i) per position (decode.py:166-167), syndrome = H error (decode.py:168)
    SC_TRY(draw_bernoulli(false, h->d_mc, h->n, batch, T, tr, k0, k1, (const u64 *)h->d_thr, 0ull, s));
    SC_TRY(launch_syndrome(h, h->d_mc, h->d_synd, T, s));
    if (out_error) SC_TRY(mc_export_bits(h, h->d_mc, nullptr, batch, T, dev_io, false, s, out_error));
    SC_TRY(mc_decode(h, d, c, 0));
    // success iff decoding == error everywhere (decode.py:173-175)
    SC_TRY(mc_finish(h, batch, T, h->n, dev_io, s, out_success, out_iters));
    return settle.done();
}

// Every HQC entry.  The eps form flips each check with probability eps (k_mc_bernoulli<true>) and decodes on the handle's shared
// priors; the table form draws an outcome per check conditional on its true bit (draw_hqc_outcome), which also fills the prior
// plane of the check columns, and the decode is the soft call's, on that plane from column N on.  o.stats / o.bits: what
// scaldpc_mc_hqc_run_stats adds (k_mc_hqc_stats on the planes the decode leaves; the decoded word as decode_batch_impl unpacks
// it).  With an output null, nothing is launched, cleared or allocated for it; the eps form has no flip / cost accumulators.
int mc_hqc_body(scaldpc_bp *h, const TrialSrc &ts, int32_t omega, const McHqcNoise &nz, int32_t batch, uint64_t seed, int32_t max_iter_arg,
                const McDecode &d, uint32_t flags, void *stream, const McHqcOut &o)
{
    SC_TRY(mc_args(h, ts, batch, d, flags, o.success));
    std::lock_guard<std::mutex> lk(h->mu);
    SC_TRY(check_usable(h));
    McHqcLaw law;
    McHqcLaw64 law64;
    if (nz.table) SC_TRY(mc_noise_law(nz, d.f64, h->m, o.cost != nullptr, &law, &law64));
    DeviceGuard dg(h->device);
    CacheBypass guard(h->async_used);
    DecodeCall c;
    SC_TRY(begin_call(h, batch, max_iter_arg, stream, &c));
    const hipStream_t s = c.s;
    SyncOnError settle{s};
    SC_TRY(refresh_full(h));
    if (h->identity_from < 0) return fail(SCALDPC_EINVAL, "parity-check matrix is not of the form [Hin | I] (hqc.py:680)");
    const int N = h->identity_from, R = h->m;
    if (omega < 0 || omega > N) return fail(SCALDPC_EINVAL, "omega must be in [0, N]");
    if (!nz.table && !(nz.eps >= 0.0 && nz.eps <= 1.0)) return fail(SCALDPC_EINVAL, "eps must be a probability");
    if ((size_t)omega * 64 * 4 > 64 * 1024) return fail(SCALDPC_EDEGREE, "omega %d too large for the LDS-resident sampler", omega);
    const bool dev_io = flags & SCALDPC_F_DEVICE_IO, early = flags & SCALDPC_F_EARLY_EXIT;
    const int T = c.T, prob_cols = nz.table ? R : 0;
    SC_TRY(mc_size(h, c, d, prob_cols, early));
    SC_TRY(grow(h->d_mc, (size_t)T * h->n));
    if (nz.table) SC_TRY(grow(h->d_mc_acc, (size_t)2 * batch));
    int *dy, *dstats;
    uint8_t *dout;
    SC_TRY(mc_stage(h->d_ylist, o.y, (size_t)batch * std::max(omega, 1), dev_io, &dy));
    SC_TRY(mc_stage(h->d_mc_outcome, o.outcome, (size_t)batch * R, dev_io, &dout));
    SC_TRY(mc_stage(h->d_mc_stats, o.stats, (size_t)5 * batch, dev_io, &dstats));
    DeviceTrials tr;
    SC_TRY(stage_trials(h->d_trial_ids, ts, batch, s, &tr));
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    // x = [y | 0]: omega distinct positions;  true bits c = Hin y = H x  (hqc.py:1253-1257)
    SC_HIP(hipMemsetAsync(h->d_mc, 0, sizeof(u64) * (size_t)T * h->n, s));
    if (omega) SC_TRY(draw_hqc_secret(h, N, omega, batch, T, tr, k0, k1, dy, s));
    SC_TRY(launch_syndrome(h, h->d_mc, h->d_synd, T, s));
    int *const acc_flips = h->d_mc_acc, *const acc_cost = nz.counted() ? acc_flips + batch : nullptr;
    if (nz.table) {
        // each check: an outcome of the (wrapped) oracle given its true bit -> the reported bit and its certainty (hqc.py:782-871)
        SC_HIP(hipMemsetAsync(acc_flips, 0, sizeof(int) * (size_t)2 * batch, s));
        SC_TRY(draw_hqc_outcome(h, d.f64, law, law64, R, batch, T, tr, k0, k1, acc_flips, acc_cost, dout, s));
    } else {  // each oracle answer wrong with probability eps
        SC_TRY(draw_bernoulli(true, h->d_synd, R, batch, T, tr, k0, k1, (const u64 *)nullptr, bernoulli_threshold(nz.eps), s));
    }
    // msg = [0]*N ++ reported (hqc.py:703-705); its syndrome under H = [Hin | I] is `reported` itself
    SC_HIP(hipMemsetAsync(h->d_recv, 0, sizeof(u64) * (size_t)T * h->n, s));
    SC_HIP(hipMemcpy2DAsync(h->d_recv + N, sizeof(u64) * h->n, h->d_synd, sizeof(u64) * h->m, sizeof(u64) * h->m, T,
                            hipMemcpyDeviceToDevice, s));
    if (o.msg) SC_TRY(mc_export_bits(h, h->d_recv, nullptr, batch, T, dev_io, false, s, o.msg));
    SC_TRY(mc_decode(h, d, c, prob_cols));
    const hipMemcpyKind back = dev_io ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    SC_TRY(mc_unstage(o.y, dy, (size_t)batch * omega, dev_io, s));
    SC_TRY(mc_unstage(o.outcome, dout, (size_t)batch * R, dev_io, s));
    if (o.flips) SC_HIP(hipMemcpyAsync(o.flips, acc_flips, sizeof(int) * (size_t)batch, back, s));
    if (o.cost) SC_HIP(hipMemcpyAsync(o.cost, acc_cost, sizeof(int) * (size_t)batch, back, s));
    if (o.stats) {
        // the counters of hqc.py:709-758, from the decisions every path (compact passes, the hand-over) has left in d_hard
        SC_HIP(hipMemsetAsync(dstats, 0, sizeof(int) * (size_t)5 * batch, s));
        hipLaunchKernelGGL(k_mc_hqc_stats, dim3((h->n + 4 * MC_STATS_RUN - 1) / (4 * MC_STATS_RUN), T), dim3(256), 0, s,
                           h->d_hard.get(), h->d_mc.get(), h->d_recv.get(), h->n, N, batch, dstats);
        LAUNCH_CHECK();
        SC_TRY(mc_unstage(o.stats, dstats, (size_t)5 * batch, dev_io, s));
    }
    // decoded = e XOR msg, as the decode entry of the same precision returns it for out_msg
    if (o.bits) SC_TRY(mc_export_bits(h, h->d_hard, h->d_recv, batch, T, dev_io, true, s, o.bits));
    // decoded[:N] = e[:N] XOR msg[:N] = e[:N] must equal the indicator of y (hqc.py:742-749)
    SC_TRY(mc_finish(h, batch, T, N, dev_io, s, o.success, o.iters));
    return settle.done();
}

}  // namespace

int scaldpc_mc_fer_run(scaldpc_bp *h, int64_t first_trial, int32_t batch, uint64_t seed, int32_t max_iter_arg,
                       int32_t method, float alpha, uint32_t flags, void *stream, uint8_t *out_success,
                       int32_t *out_iters, uint8_t *out_error)
{
    return mc_fer_body(h, TrialSrc::range(first_trial), batch, seed, max_iter_arg, McDecode::fp32(method, alpha), flags, stream,
                       out_success, out_iters, out_error);
}

int scaldpc_mc_fer_run_at(scaldpc_bp *h, const int64_t *trial_ids, int32_t batch, uint64_t seed, int32_t max_iter_arg,
                          int32_t method, float alpha, uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_iters,
                          uint8_t *out_error)
{
    return mc_fer_body(h, TrialSrc::list(trial_ids), batch, seed, max_iter_arg, McDecode::fp32(method, alpha), flags, stream,
                       out_success, out_iters, out_error);
}

int scaldpc_mc_hqc_run(scaldpc_bp *h, int32_t omega, double eps, int64_t first_trial, int32_t batch, uint64_t seed,
                       int32_t max_iter_arg, int32_t method, float alpha, uint32_t flags, void *stream,
                       uint8_t *out_success, int32_t *out_iters, uint8_t *out_msg, int32_t *out_y)
{
    return mc_hqc_body(h, TrialSrc::range(first_trial), omega, McHqcNoise::flip(eps), batch, seed, max_iter_arg,
                       McDecode::fp32(method, alpha), flags, stream, {out_success, out_iters, out_msg, out_y});
}

int scaldpc_mc_hqc_run_soft(scaldpc_bp *h, int32_t omega, const double *weights, const uint8_t *flips, const float *probs,
                            const int32_t *costs, int32_t K, int64_t first_trial, int32_t batch, uint64_t seed,
                            int32_t max_iter_arg, int32_t method, float alpha, uint32_t flags, void *stream,
                            uint8_t *out_success, int32_t *out_iters, uint8_t *out_msg, int32_t *out_y, uint8_t *out_outcome,
                            int32_t *out_flips, int32_t *out_cost)
{
    return mc_hqc_body(h, TrialSrc::range(first_trial), omega, McHqcNoise::drawn(weights, flips, probs, costs, K), batch, seed,
                       max_iter_arg, McDecode::fp32(method, alpha), flags, stream,
                       {out_success, out_iters, out_msg, out_y, out_outcome, out_flips, out_cost});
}

int scaldpc_mc_hqc_run_stats(scaldpc_bp *h, int32_t omega, const double *weights, const uint8_t *flips, const float *probs,
                             const int32_t *costs, int32_t K, int64_t first_trial, int32_t batch, uint64_t seed,
                             int32_t max_iter_arg, int32_t method, float alpha, uint32_t flags, void *stream,
                             uint8_t *out_success, int32_t *out_iters, uint8_t *out_msg, int32_t *out_y, uint8_t *out_outcome,
                             int32_t *out_flips, int32_t *out_cost, int32_t *out_stats, uint8_t *out_bits)
{
    if (!out_stats) return fail(SCALDPC_EINVAL, "out_stats is NULL");
    return mc_hqc_body(h, TrialSrc::range(first_trial), omega, McHqcNoise::drawn(weights, flips, probs, costs, K), batch, seed,
                       max_iter_arg, McDecode::fp32(method, alpha), flags, stream,
                       {out_success, out_iters, out_msg, out_y, out_outcome, out_flips, out_cost, out_stats, out_bits});
}

// (out_stats may be NULL here, as in the float64 entry: with it NULL this is scaldpc_mc_hqc_run_soft on chosen trials)
int scaldpc_mc_hqc_run_stats_at(scaldpc_bp *h, int32_t omega, const double *weights, const uint8_t *flips, const float *probs,
                                const int32_t *costs, int32_t K, const int64_t *trial_ids, int32_t batch, uint64_t seed,
                                int32_t max_iter_arg, int32_t method, float alpha, uint32_t flags, void *stream,
                                uint8_t *out_success, int32_t *out_iters, uint8_t *out_msg, int32_t *out_y, uint8_t *out_outcome,
                                int32_t *out_flips, int32_t *out_cost, int32_t *out_stats, uint8_t *out_bits)
{
    return mc_hqc_body(h, TrialSrc::list(trial_ids), omega, McHqcNoise::drawn(weights, flips, probs, costs, K), batch, seed,
                       max_iter_arg, McDecode::fp32(method, alpha), flags, stream,
                       {out_success, out_iters, out_msg, out_y, out_outcome, out_flips, out_cost, out_stats, out_bits});
}

// The same sweeps decoded in the reference's own arithmetic (McDecode::float64())

int scaldpc_mc_fer_run_f64(scaldpc_bp *h, int64_t first_trial, int32_t batch, uint64_t seed, int32_t max_iter_arg, uint32_t flags,
                           void *stream, uint8_t *out_success, int32_t *out_iters, uint8_t *out_error)
{
    return mc_fer_body(h, TrialSrc::range(first_trial), batch, seed, max_iter_arg, McDecode::float64(), flags, stream, out_success,
                       out_iters, out_error);
}

int scaldpc_mc_fer_run_at_f64(scaldpc_bp *h, const int64_t *trial_ids, int32_t batch, uint64_t seed, int32_t max_iter_arg,
                              uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_iters, uint8_t *out_error)
{
    return mc_fer_body(h, TrialSrc::list(trial_ids), batch, seed, max_iter_arg, McDecode::float64(), flags, stream, out_success,
                       out_iters, out_error);
}

int scaldpc_mc_hqc_run_f64(scaldpc_bp *h, int32_t omega, double eps, int64_t first_trial, int32_t batch, uint64_t seed,
                           int32_t max_iter_arg, uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_iters,
                           uint8_t *out_msg, int32_t *out_y)
{
    return mc_hqc_body(h, TrialSrc::range(first_trial), omega, McHqcNoise::flip(eps), batch, seed, max_iter_arg, McDecode::float64(),
                       flags, stream, {out_success, out_iters, out_msg, out_y});
}

int scaldpc_mc_hqc_run_stats_f64(scaldpc_bp *h, int32_t omega, const double *weights, const uint8_t *flips, const double *probs,
                                 const int32_t *costs, int32_t K, int64_t first_trial, int32_t batch, uint64_t seed,
                                 int32_t max_iter_arg, uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_iters,
                                 uint8_t *out_msg, int32_t *out_y, uint8_t *out_outcome, int32_t *out_flips, int32_t *out_cost,
                                 int32_t *out_stats, uint8_t *out_bits)
{
    return mc_hqc_body(h, TrialSrc::range(first_trial), omega, McHqcNoise::drawn(weights, flips, probs, costs, K), batch, seed,
                       max_iter_arg, McDecode::float64(), flags, stream,
                       {out_success, out_iters, out_msg, out_y, out_outcome, out_flips, out_cost, out_stats, out_bits});
}

int scaldpc_mc_hqc_run_stats_at_f64(scaldpc_bp *h, int32_t omega, const double *weights, const uint8_t *flips, const double *probs,
                                    const int32_t *costs, int32_t K, const int64_t *trial_ids, int32_t batch, uint64_t seed,
                                    int32_t max_iter_arg, uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_iters,
                                    uint8_t *out_msg, int32_t *out_y, uint8_t *out_outcome, int32_t *out_flips, int32_t *out_cost,
                                    int32_t *out_stats, uint8_t *out_bits)
{
    return mc_hqc_body(h, TrialSrc::list(trial_ids), omega, McHqcNoise::drawn(weights, flips, probs, costs, K), batch, seed,
                       max_iter_arg, McDecode::float64(), flags, stream,
                       {out_success, out_iters, out_msg, out_y, out_outcome, out_flips, out_cost, out_stats, out_bits});
}

int scaldpc_bp_configure(scaldpc_bp *h, const char *key, const char *value)
{
    if (!h || !key || !value) return fail(SCALDPC_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (!set_knob(h->kn, key, value)) return fail(SCALDPC_EINVAL, "unknown knob or bad value: %s=%s", key, value);
    return 0;
}

int scaldpc_bp_device_of(scaldpc_bp *h, int32_t *out)
{
    if (!h || !out) return fail(SCALDPC_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    auto where = [](const void *p) -> int {
        if (!p) return -1;
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) != hipSuccess) {
            (void)hipGetLastError();
            return -2;
        }
        return at.device;
    };
    out[0] = h->device;
    out[1] = where(h->d_graph);
    out[2] = where(h->d_msg ? h->d_msg.get() : h->d_emsg.get());
    out[3] = where(h->d_synd);
    return 0;
}

int scaldpc_bp_time_kernels(scaldpc_bp *h, int32_t iters, int32_t method, float alpha, void *stream, float *ms,
                            int32_t *launches)
{
    if (!h || !ms || !launches || iters <= 0) return fail(SCALDPC_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    SC_TRY(check_usable(h));
    DeviceGuard dg(h->device);
    if (h->last_group <= 0) return fail(SCALDPC_EINVAL, "no previous decode to time");
    hipStream_t s = stream ? (hipStream_t)stream : h->own_stream;
    const int g = h->last_group;
    SC_TRY(ensure_msg(h, g, method));  // (a method other than the last decode's may want the record arrays)
    const int nl = std::min(fixed_lanes(h, g), 2);
    SC_TRY(ensure_lanes(h, nl));
    // The variable pass is timed in the form the last decode launched it in: early-exit runs write decisions on EVERY
    // pass (all columns), fixed-iteration runs only on the last one (the passes before it leave out the columns of
    // degree <= 1 in the record form).  launches[5] says which.
    const int wo = h->last_early ? 1 : 0;
    const bool recf = rec_form(h, method);
    const int form_bits = (recf ? 1 : 0) | (wo ? 2 : 0) | (recf && !wo ? 4 : 0);
    TimingEvents ev;
    SyncOnError settle{s};
    Lanes lanes(h, s);
    int gs[2], t0[2];
    deal_tiles(g, nl, gs, t0);  // as iterate_tiles deals the tiles
    const TileState st{h->d_synd, h->d_hard, h->d_done, h->d_conv, h->d_unsat, h->d_iters, nullptr};  // (no posteriors)
    auto check = [&](int it, int k) {
        CheckPass cp;
        cp.alpha = alpha_for(alpha, it + 1);
        cp.tile0 = t0[k];
        return launch_check(h, st.at(h, t0[k]), gs[k], method, 0, lanes[k], cp);
    };
    auto var = [&](int k) {
        VarPass vp;
        vp.write_out = wo;
        vp.tile0 = t0[k];
        vp.rec = recf;
        vp.light = true;
        return launch_var(h, st.at(h, t0[k]), gs[k], 0, lanes[k], vp);
    };
    // `iters` back-to-back launches of each kernel between two events: the event
    // overhead (a few us, comparable to a 65 us launch) is amortised, what remains is
    // the kernel plus the ~1.5 us dependent-launch gap it also pays in a real decode.
    if (nl < 2) {
        SC_TRY(ev.create(4));
        SC_HIP(hipEventRecord(ev[0], s));
        for (int it = 0; it < iters; it++) SC_TRY(check(it, 0));
        SC_HIP(hipEventRecord(ev[1], s));
        SC_HIP(hipEventRecord(ev[2], s));
        for (int it = 0; it < iters; it++) SC_TRY(var(0));
        SC_HIP(hipEventRecord(ev[3], s));
        SC_HIP(hipStreamSynchronize(s));
        SC_HIP(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
        SC_HIP(hipEventElapsedTime(&ms[1], ev[2], ev[3]));
        launches[0] = launches[1] = iters;
        launches[2] = launches[4] = g * TW;  // codewords swept per launch
        launches[3] = 1;
        launches[5] = form_bits;
        return settle.done();
    }
    // Two-lane schedule (what a fixed-iteration decode runs): the decode's own launch pattern --
    // each lane alternates check and variable launches over its half of the group, the second
    // lane one kernel out of phase -- with an event after EVERY launch; a launch's duration is
    // the distance between its event and the previous one on the same lane (it includes the
    // dependent-launch gap, as the single-lane series do).  ms[] = sum over the measured
    // launches of both lanes, the first two iterations (phase settling) excluded.
    const int total = iters + 2;
    SC_TRY(ev.create((size_t)2 * (2 * total + 1)));  // per lane: start, then one per launch
    auto M = [&](int k, int i) -> hipEvent_t & { return ev[(size_t)k * (2 * total + 1) + i]; };
    auto phase = [&]() -> int {  // the second lane starts one kernel behind the first
        SC_HIP(hipEventRecord(h->ev_phase[1], lanes[0]));
        SC_HIP(hipStreamWaitEvent(lanes[1], h->ev_phase[1], 0));
        return 0;
    };
    SC_TRY(lanes.fork(2));
    for (int it = 0; it < total; it++) {
        for (int k = 0; k < 2; k++) {
            if (it == 0) SC_HIP(hipEventRecord(M(k, 0), lanes[k]));
            SC_TRY(check(it, k));
            SC_HIP(hipEventRecord(M(k, 2 * it + 1), lanes[k]));
            if (it == 0 && k == 0) SC_TRY(phase());
        }
        for (int k = 0; k < 2; k++) {
            SC_TRY(var(k));
            SC_HIP(hipEventRecord(M(k, 2 * it + 2), lanes[k]));
        }
    }
    SC_TRY(lanes.join());
    SC_HIP(hipStreamSynchronize(s));
    double tc = 0.0, tv = 0.0;
    int nc = 0, nv = 0;
    for (int k = 0; k < 2; k++)
        for (int it = 2; it < total; it++) {
            float d = 0.0f;
            SC_HIP(hipEventElapsedTime(&d, M(k, 2 * it), M(k, 2 * it + 1)));
            tc += d;
            nc++;
            SC_HIP(hipEventElapsedTime(&d, M(k, 2 * it + 1), M(k, 2 * it + 2)));
            tv += d;
            nv++;
        }
    // The event after every launch costs the schedule its back-to-back dispatch (~2.5 us per launch: with the 30-50
    // us launches of the record form the evented pair came out 6 % above rocprofv3's).  A second pass with the same
    // launch pattern and NO events in between gives the pair's true duration per lane; the evented series supply
    // only the check : variable ratio.
    hipEvent_t &b0 = M(0, 0), &e0 = M(0, 1), &b1 = M(1, 0), &e1 = M(1, 1);
    SC_TRY(lanes.fork(2));
    for (int it = 0; it < total; it++) {
        if (it == 2) {
            SC_HIP(hipEventRecord(b0, lanes[0]));
            SC_HIP(hipEventRecord(b1, lanes[1]));
        }
        for (int k = 0; k < 2; k++) {
            SC_TRY(check(it, k));
            if (it == 0 && k == 0) SC_TRY(phase());
        }
        for (int k = 0; k < 2; k++) SC_TRY(var(k));
    }
    SC_HIP(hipEventRecord(e0, lanes[0]));
    SC_HIP(hipEventRecord(e1, lanes[1]));
    SC_TRY(lanes.join());
    SC_HIP(hipStreamSynchronize(s));
    float d0 = 0.0f, d1 = 0.0f;
    SC_HIP(hipEventElapsedTime(&d0, b0, e0));
    SC_HIP(hipEventElapsedTime(&d1, b1, e1));
    const double pair_ms = 0.5 * ((double)d0 + (double)d1) / (total - 2);
    if (pair_ms > 0.0 && tc + tv > 0.0 && nc == nv && nc > 0) {
        const double evented_pair = (tc + tv) / nc, scale = pair_ms / evented_pair;
        tc *= scale;
        tv *= scale;
    }
    ms[0] = (float)tc;
    ms[1] = (float)tv;
    launches[0] = nc;
    launches[1] = nv;
    launches[2] = gs[0] * TW;
    launches[4] = gs[0] * TW;  // (odd groups: the second lane's launches are one tile smaller)
    launches[3] = 2;
    launches[5] = form_bits;
    return settle.done();
}

void scaldpc_bp_destroy(scaldpc_bp *h)
{
    if (!h) return;
    DeviceGuard dg(h->device);
    // A handle that took SCALDPC_F_ASYNC calls may still have work in flight, on the caller's stream and
    // on its own lanes: wait for the device, and send its blocks through hipFree instead of parking
    // them for the next handle.  The guard must be in place BEFORE the first block is released.
    CacheBypass guard(h->async_used);
    if (h->async_used) (void)hipDeviceSynchronize();
    delete h;  // the buffers, then the streams and events (HandleStreams)
}

}  // extern "C"
