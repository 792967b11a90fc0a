/*
 * scaldpc.h -- C ABI of libscaldpc: MI355X (gfx950) LDPC belief-propagation
 * decoders behind the decoder boundary of atneit/SCA-LDPC's Monte-Carlo drivers.
 *
 * Plain C types only (pointers, sizes, ints); opaque handles; every entry point
 * returns an int status (0 = ok) and never throws across the boundary;
 * scaldpc_last_error() gives the message of the calling thread's last failure.
 *
 * What each entry point replaces in the reference (paths relative to
 * simulate-with-python/):
 *
 *   scaldpc_bp_create            ldpc.bp_decoder.__init__ dense->sparse graph build,
 *                                call sites simulate/decode.py:155-161, simulate/hqc.py:694-699
 *   scaldpc_bp_set_channel_probs the `error_rate=` / `channel_probs=` constructor kwargs (same sites)
 *   scaldpc_bp_append_rows /     the attack loop's growing H: add_check's np.vstack (simulate/hqc.py:885-908) and the
 *     _set_channel_probs_tail    decoder rebuild of every decode (hqc.py:680,694) -> rows appended to a live decoder
 *   scaldpc_bp_decode_batch      ldpc.bp_decoder.decode(v), simulate/decode.py:171, simulate/hqc.py:708
 *                                (batched: one call = `batch` independent decode() calls)
 *   scaldpc_bp_decode_batch_soft the same with the priors of the last columns given PER CODEWORD: hqc.decode()'s
 *                                `channel_probs = [w/N]*N ++ [1 - certainty_i]`, simulate/hqc.py:684-699, whose check
 *                                certainties differ from trial to trial (hqc.py:782-806)
 *                                (entry point added under SCALDPC_VERSION 103: nothing that existed changed)
 *   scaldpc_bp_decode_batch_f64  the same decode() in the package's OWN arithmetic: product-sum in the probability-ratio
 *                                domain, float64 -- decisions, iteration counts and converged flags are
 *                                the package's exactly, posteriors to the last ulps of one log()
 *                                (entry point added under SCALDPC_VERSION 104: nothing that existed changed)
 *   scaldpc_bp_destroy           object lifetime
 *   scaldpc_mc_fer_run           the per-trial body of simulate_frame_error_rate,
 *                                simulate/decode.py:36-40,165-175 (noise, syndrome, decode, compare)
 *   scaldpc_mc_hqc_run           hqc.decode() input assembly + success test for synthetic trials,
 *                                simulate/hqc.py:684-705,742-749
 *   scaldpc_mc_hqc_run_soft      the same trials with the answers of the oracles the attack really asks: per check an outcome of
 *                                wrapped_hqc_decoding_oracle / inner_hqc_decoding_oracle, simulate/hqc.py:782-871, drawn
 *                                conditional on the check's true value -- the reported bit, its certainty (the check's own
 *                                prior, hqc.py:689) and the oracle calls it spent -- on the device
 *                                (entry point added under SCALDPC_VERSION 103: nothing that existed changed)
 *   scaldpc_mc_fer_run_f64 / scaldpc_mc_hqc_run_f64 / scaldpc_mc_hqc_run_stats_f64
 *                                the same three sweeps decoded by scaldpc_bp_decode_batch_f64's recursion: the reference's
 *                                success rates in its own arithmetic, trial for trial
 *                                (entry points added under SCALDPC_VERSION 104: nothing that existed changed)
 *   scaldpc_mc_fer_run_at / scaldpc_mc_hqc_run_stats_at / scaldpc_mc_fer_run_at_f64 / scaldpc_mc_hqc_run_stats_at_f64 /
 *   scaldpc_mc_qary_run_at / scaldpc_mc_qary_run_secret_at
 *                                the sweeps above on CHOSEN trials: a list of global trial indices where the sibling takes a
 *                                contiguous range -- the post-mortem of a sweep's failures, the attack loop that stops at a
 *                                key's first success (simulate/hqc.py:980-982), a subset picked on the host
 *                                (entry points added under SCALDPC_VERSION 104: nothing that existed changed)
 *   scaldpc_qary_create          simulate_rs Decoder::new via PyO3 `#[new]`,
 *                                simulate_rs/src/pydecoder.rs:24-45 -> simulate_rs/src/decoder.rs:494-553
 *   scaldpc_qary_min_sum_batch   PyO3 `min_sum`, simulate_rs/src/pydecoder.rs:53-65
 *                                -> decoder.rs:668-692 (into_llr) + decoder.rs:560-666 (min_sum)
 *   scaldpc_qary_into_llr        Decoder::into_llr, simulate_rs/src/decoder.rs:668-692 (== decoder_special.rs:619-643),
 *                                the conversion alone (its known-answer test: decoder.rs:744-768)
 *   scaldpc_qary_special_create / _min_sum_batch
 *                                simulate_rs/src/pydecoder.rs:96-117,125-145
 *                                -> simulate_rs/src/decoder_special.rs:387-464, 471-617
 *   scaldpc_qary_min_sum_batch_soft / scaldpc_qary_special_min_sum_batch_soft
 *                                the same decodes, with what the last variable update (decoder.rs:634-658 /
 *                                decoder_special.rs:566-609) computes and the reference drops at its arg-min
 *                                (decoder.rs:654-657): the per-symbol totals, the margin of every decision, and the
 *                                number of checks the decided word leaves unmet (the reference has no convergence test)
 *                                (entry points added under SCALDPC_VERSION 103: nothing that existed changed)
 *   scaldpc_mc_qary_run          the per-trial body of simulate_frame_error_rate_rust, simulate/decode.py:246-257,273-277:
 *                                every symbol of an all-zero word gets the "good" or the "bad" pmf row, min_sum, is the
 *                                decision all zero -- trials drawn on the device
 *                                (entry point added under SCALDPC_VERSION 103: nothing that existed changed)
 *   scaldpc_mc_qary_run_secret   the trial the Kyber decoders exist for, simulate/kyber.py: a secret drawn from the centred
 *                                binomial (kyber.py:60-64,95-105), the row sums that follow from it and H (compute_ssum,
 *                                kyber.py:85-92), every variable measured by an oracle whose answer depends on the TRUE symbol,
 *                                the posterior pmf of that answer handed to the decoder
 *                                (max_likelihood.s_distribution_from_hard_y, kyber.py:362-376) -- is the key recovered?
 *                                (entry point added under SCALDPC_VERSION 103: nothing that existed changed)
 *
 * Threading: calls on distinct handles are independent; calls on one handle are
 * serialised internally, so one decoder object may be shared by many host
 * threads as the reference's thread pool does (simulate/decode.py:247-262).
 *
 * Device / host buffers: unless SCALDPC_F_DEVICE_IO is set, `in`/`out_*` are host
 * pointers and are staged through device memory by the call.  With
 * SCALDPC_F_DEVICE_IO they are device pointers (e.g. torch tensors' data_ptr())
 * and nothing crosses PCIe.  `stream` is a hipStream_t passed as void* (NULL =
 * the handle's own non-blocking stream); the call returns after the stream work is
 * complete unless SCALDPC_F_ASYNC is set (device I/O only).  With device pointers the
 * caller owns the ordering: pass the stream the inputs were produced on (or
 * synchronise first), and do not touch the handle's priors or buffers while an
 * SCALDPC_F_ASYNC call is still in flight.
 */
#ifndef SCALDPC_H
#define SCALDPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCALDPC_VERSION 104

/* status codes */
#define SCALDPC_OK 0
#define SCALDPC_EINVAL 1   /* bad argument (shape, mode, method, NULL) -> Python ValueError */
#define SCALDPC_EHIP 2     /* HIP runtime failure */
#define SCALDPC_ENOMEM 3
#define SCALDPC_EPMF 4     /* pmf row does not sum to 1 +- 1e-3 (decoder.rs:683-684 assert) */
#define SCALDPC_ENOCONF 5  /* a check admits no finite configuration (decoder.rs:618 assert) */
#define SCALDPC_EDEGREE 6  /* degree/alphabet outside what the kernels are built for */

/* bp methods (ldpc.bp_decoder `bp_method`) */
#define SCALDPC_BP_PRODUCT_SUM 0 /* "product_sum"/"ps"(+_log): tanh rule, LLR domain, fp32 */
#define SCALDPC_BP_MIN_SUM 1     /* "min_sum"/"ms"(+_log): scaling `alpha` (0 => 1 - 2^-iter) */

/* decode input convention (ldpc.bp_decoder.decode) */
#define SCALDPC_IN_SYNDROME 0 /* in: uint8 [batch][m]; result = error estimate e */
#define SCALDPC_IN_RECEIVED 1 /* in: uint8 [batch][n]; s = H v mod 2; result = e XOR v */

/* flags */
#define SCALDPC_F_EARLY_EXIT 1u /* per-codeword stop at H e == s (reference behaviour) */
#define SCALDPC_F_DEVICE_IO 2u  /* in/out pointers are device pointers */
#define SCALDPC_F_ASYNC 4u      /* with DEVICE_IO: enqueue only, caller synchronises `stream` */

const char *scaldpc_last_error(void);
int scaldpc_version(void);
int scaldpc_device_count(int *count);
int scaldpc_set_device(int device);
/* Device and pinned-host blocks (up to 64 MiB each, 512 MiB in total) released by destroyed
 * handles are parked for the next handle instead of going through hipFree: the reference builds
 * a new decoder per decode (simulate/hqc.py:694), and allocation would otherwise cost several
 * times the decode.  scaldpc_trim() returns the parked blocks to the driver;
 * SCALDPC_NO_CACHE=1 in the environment disables parking.  The host-side graph mirrors and tables of a handle
 * (a few multi-megabyte vectors) are recycled the same way (blocks >= 32 KiB, at most 256 MiB parked, also returned
 * by scaldpc_trim()): left to malloc they are unmapped and page-faulted in again per decoder, at a cost that depends
 * on the state of the host process's heap (0.45 ms or 2-8 ms per construction, measured). */
int scaldpc_trim(void);
/* Leak accounting (tests, profiles/microbench/leak_check.py): blocks the library's allocator has handed
 * out and that a live handle still owns.  out[6] = { device blocks, device bytes, pinned-host blocks,
 * pinned-host bytes, parked (idle) blocks, parked bytes }.  A create / decode / destroy cycle must leave
 * out[0..3] where it found them -- the reference builds a decoder per decode (simulate/hqc.py:694-708). */
int scaldpc_debug_live_blocks(int64_t *out);
/* Fault injection (tests): the `countdown`-th allocation the library makes from now on (device or pinned host,
 * any handle, any thread) fails with SCALDPC_ENOMEM; 0 disarms.  Every entry point must then return an error
 * code, leave the handle either intact or refusing further calls (never decoding on half-updated state), and
 * scaldpc_*_destroy must still release everything (scaldpc_debug_live_blocks back at its starting value).
 * Opt-in: the injector exists only in a process started with SCALDPC_DEBUG=1 (read once); otherwise arming it
 * returns SCALDPC_EINVAL and the allocator never consults the countdown. */
int scaldpc_debug_fail_alloc(int32_t countdown);
/* Measurement aid for bench.py (`roofline.cache_ceiling_GBps`): an in-place read-all / write-all stream over
 * `bytes` of scratch device memory -- every wave reads `rows_per_wave` consecutive 256-B rows and writes them back,
 * the access shape of an in-place BP pass -- `reps` launches between two HIP events on the NULL stream of the
 * current device.  *gbps = read + written bytes per second.  At the size of a cache-resident tile group (209 MB on
 * the HQC-128 graph) this is what the Infinity Cache sustains for this shape; far beyond 256 MiB, what HBM does.
 * No reference counterpart (measurement only). */
int scaldpc_measure_rmw_stream(int64_t bytes, int32_t rows_per_wave, int32_t reps, double *gbps);

/* ------------------------------------------------------------------ binary BP */
typedef struct scaldpc_bp scaldpc_bp;

/* Graph in CSR: row_ptr[m+1], col_idx[nnz] ascending inside each row (host pointers). */
int scaldpc_bp_create(int32_t m, int32_t n, int64_t nnz, const int32_t *row_ptr,
                      const int32_t *col_idx, scaldpc_bp **out);
/* Per-bit prior error probabilities, float64 [n] (host). p = 0 / p = 1 are legal
 * (LLR = +-inf), as the reference's certainty-1.0 checks produce (hqc.py:689). */
int scaldpc_bp_set_channel_probs(scaldpc_bp *h, const double *probs);
/*
 * A graph that GROWS: the attack loop adds one parity check per oracle answer (hqc.py:885-908,
 * `H = np.vstack([H, row])`) and decodes every DECODE_EVERY answers on [H | I] (hqc.py:972-980, 680),
 * where the reference rebuilds the decoder from the dense matrix each time.  Here the decoder lives on:
 *   scaldpc_bp_append_rows(h, nrows, row_ptr, col_idx, new_n)
 *       appends `nrows` checks (CSR of the new rows only: row_ptr[0] = 0, columns strictly ascending,
 *       < new_n) and grows the block length to new_n >= n (the new columns come last -- for [Hin | I]
 *       each appended row brings its identity column).  Only the new rows are validated; device CSR
 *       and priors have spare capacity and are appended to; the tables of the row-parallel kernels
 *       (the single decode() of the attack loop) are updated in place -- one word per new edge while
 *       the edge's column has a free lane, a moved segment otherwise; what only the 64-codeword-tile
 *       and LDS kernels need (CSC, degree buckets, their tables) is rebuilt when one of them is next
 *       used.  Results are those of a decoder freshly built on the grown graph, bit for bit.
 *   scaldpc_bp_set_channel_probs_tail(h, first, count, probs)
 *       priors of columns [first, first + count) (float64, as scaldpc_bp_set_channel_probs); the
 *       columns an append added must be given theirs before the next decode.
 */
int scaldpc_bp_append_rows(scaldpc_bp *h, int32_t nrows, const int32_t *row_ptr, const int32_t *col_idx, int32_t new_n);
int scaldpc_bp_set_channel_probs_tail(scaldpc_bp *h, int32_t first, int32_t count, const double *probs);
/*
 * Decode `batch` independent inputs, flooding schedule, fp32 messages.
 *   max_iter <= 0 -> n (ldpc convention)
 *   out_bits  uint8 [batch][n]   required
 *   out_llr   float [batch][n]   optional (NULL): posterior log(p0/p1) of the error estimate
 *   out_iters int32 [batch]      optional: iteration at which H e == s first held (else max_iter)
 *   out_conv  uint8 [batch]      optional: 1 iff the returned decision satisfies H e == s
 */
int scaldpc_bp_decode_batch(scaldpc_bp *h, const uint8_t *in, int32_t input_kind, int32_t batch,
                            int32_t max_iter, int32_t method, float alpha, uint32_t flags,
                            void *stream, uint8_t *out_bits, float *out_llr, int32_t *out_iters,
                            uint8_t *out_conv);
/*
 * scaldpc_bp_decode_batch with per-codeword priors for the LAST prob_cols columns, [n - prob_cols, n):
 *   probs  float32 [batch][prob_cols]: prior error probabilities of those columns for each codeword, 1 <= prob_cols <= n;
 *          the columns below keep the handle's shared priors (scaldpc_bp_set_channel_probs).  For H = [Hin | I_R],
 *          prob_cols = R is the `check_part` of hqc.py:689; prob_cols = n is a fully soft input.
 *          `probs` lives where `in` lives: host memory, or device memory with SCALDPC_F_DEVICE_IO.
 * Everything else means what it means in scaldpc_bp_decode_batch.  The handle's own priors are not changed: a plain call
 * afterwards behaves as before.  The prior LLRs are logf((1.0f - p) / p) in float32, computed on the device with glibc's
 * logf algorithm and the correctly rounded division: value for value what scaldpc_bp_set_channel_probs computes on the
 * host for the same float32 p (p = 0 / p = 1 are legal: LLR = +-inf).
 * Validation: a value outside [0, 1] or a NaN returns SCALDPC_EINVAL and names the codeword and the column.  Host input is
 * checked before anything is enqueued; device input is checked by the conversion kernel and reported when the call
 * synchronises (the outputs are then not to be used).  Under SCALDPC_F_ASYNC device input is NOT checked: the caller
 * answers for it (a bad value decodes as p = 1/2).
 */
int scaldpc_bp_decode_batch_soft(scaldpc_bp *h, const uint8_t *in, int32_t input_kind, int32_t batch,
                                 const float *probs, int32_t prob_cols,
                                 int32_t max_iter, int32_t method, float alpha, uint32_t flags, void *stream,
                                 uint8_t *out_bits, float *out_llr, int32_t *out_iters, uint8_t *out_conv);
/*
 * The reference's own arithmetic on the device: ldpc.bp_decoder(..., bp_method="product_sum") is the probability-ratio
 * recursion in float64, and this entry point runs it operation for operation (no fused multiply-add, IEEE division):
 *   init      every edge of column j carries r_j = p_j / (1 - p_j), formed in double (p = 0 -> 0, p = 1 -> inf)
 *   check i   t = +-1 by the syndrome bit; forward over the row in ascending column: c[e] = t, t *= 2 / (1 + x[e]) - 1;
 *             backward with s = 1: c[e] *= s, c[e] = (1 - c[e]) / (1 + c[e]), s *= 2 / (1 + x[e]) - 1
 *   variable  t = r_j; forward over the column in ascending row: x[e] = t, t *= c[e], a NaN t becomes 1;
 *             posterior L = log(1 / t), decision t >= 1; backward with s = 1: x[e] *= s, s *= c[e], a NaN s becomes 1
 *   test      H e == s after every iteration; with SCALDPC_F_EARLY_EXIT a converged codeword's decision, posterior and
 *             iteration count are latched
 * out_bits, out_iters and out_conv equal the float64 CPU recursion's on EVERY codeword, settled or not; out_llr differs from
 * it by the last log() alone (a few ulp; +-inf and NaN in the same places).  It is the form to ask for when the reference's
 * numbers must be reproduced, and the full-batch float64 key the fp32 tanh kernels are audited against.  It is NOT the
 * throughput path: 8-byte messages in two arrays, two to three IEEE divisions per edge and iteration, one stream, no
 * compaction -- about a third of the fp32 tanh rule's rate.
 *   in, input_kind, batch, max_iter (<= 0 -> n), out_bits, out_iters, out_conv, SCALDPC_F_EARLY_EXIT, SCALDPC_F_DEVICE_IO
 *             mean what they mean in scaldpc_bp_decode_batch; SCALDPC_F_ASYNC is refused (SCALDPC_EINVAL)
 *   out_llr   double [batch][n], optional (NULL): log(1 / T) of the posterior ratio T
 *   probs     NULL with prob_cols = 0: the handle's shared priors (scaldpc_bp_set_channel_probs, taken from its float64
 *             values).  Otherwise double [batch][prob_cols], 1 <= prob_cols <= n: prior error probabilities PER CODEWORD of
 *             the last prob_cols columns (hqc.decode()'s `1 - certainty`, simulate/hqc.py:684-699), where `in` lives; the
 *             ratios are formed on the device by the same IEEE division.  One without the other is SCALDPC_EINVAL.
 * Validation as scaldpc_bp_decode_batch_soft's: a value outside [0, 1] or a NaN returns SCALDPC_EINVAL and names the codeword
 * and the column -- host values before anything is enqueued, device values after the conversion kernel and before the
 * decode starts.  No refusal writes to an output, and the handle stays usable.
 * Works on a handle grown by scaldpc_bp_append_rows.  Tile groups follow the "group_mb" budget with 16 bytes per edge and
 * codeword (scaldpc_bp_set_tile_group overrides); results never depend on the group size.
 * (entry point added under SCALDPC_VERSION 104: nothing that existed changed)
 */
int scaldpc_bp_decode_batch_f64(scaldpc_bp *h, const uint8_t *in, int32_t input_kind, int32_t batch,
                                const double *probs, int32_t prob_cols, int32_t max_iter, uint32_t flags, void *stream,
                                uint8_t *out_bits, double *out_llr, int32_t *out_iters, uint8_t *out_conv);
/*
 * Measurement aid for bench.py: on the message state left by the last (fixed-iteration)
 * decode -- in the min-sum record form the messages and sign masks of the pass BEFORE the decode's last one, which stores
 * neither: a consistent pair, one iteration behind the decisions -- run `iters` back-to-back launches of the check kernel and of the variable kernel of
 * `method`, each series bracketed by HIP events on its launch stream.
 *   ms[0] / ms[1]   total ms of the check / variable series          (float[2])
 *   launches[0..1]  launches in each series                           (int32[6])
 *   launches[2]     codewords swept per check launch
 *   launches[3]     lanes: 1 = the series ran one after the other over the whole tile group;
 *                   2 = the decode's two-stream schedule: the check series over the first
 *                   lane's tiles and the variable series over the second lane's tiles ran
 *                   concurrently, as they do in a decode's steady state.  There every launch is followed by an
 *                   event (its duration = the distance to the previous event on its lane); because those events
 *                   cost the schedule its back-to-back dispatch, the same launch pattern is run once more WITHOUT
 *                   them, bracketed per lane, and ms[0] / ms[1] are scaled so that check + variable = the true pair
 *   launches[4]     codewords swept per variable launch
 *   launches[5]     bit 0: min-sum ran in its record form (k_check_minsum_rec / k_var_rec; knob "minsum_rec");
 *                   bit 1: the variable pass was timed WITH its decision output -- the form every pass of an
 *                   early-exit decode launches; the timing follows the last decode (fixed iterations: no output);
 *                   bit 2: record form and no output: the timed variable launch leaves out the columns of degree <= 1
 */
int scaldpc_bp_time_kernels(scaldpc_bp *h, int32_t iters, int32_t method, float alpha, void *stream,
                            float *ms, int32_t *launches);
/* Tuning knob: codeword tiles (64 codewords each) per cache-resident group; 0 = auto
 * (largest group whose in-place message array stays within ~200 MB of Infinity Cache). */
int scaldpc_bp_set_tile_group(scaldpc_bp *h, int32_t tiles);
/* Number of codewords the last early-exit call re-decoded in its compact second pass
 * (stragglers of mostly-converged tile groups; results are identical either way;
 * environment SCALDPC_COMPACT_AFTER=0 disables the pass, =k moves the decision point). */
int scaldpc_bp_last_compacted(scaldpc_bp *h, int64_t *count);
/* Path statistics of the last call, out[4]:
 *   out[0] = scaldpc_bp_last_compacted
 *   out[1] = codewords decoded with the row-parallel kernels (wave = one row of one codeword,
 *            lane = edge; taken for calls -- or compact passes -- of at most 6 (min-sum) / 4
 *            (tanh rule) codewords on graphs too large for LDS: the single decode() of
 *            hqc.py:708).  Results are identical to the 64-codeword-tile kernels;
 *            SCALDPC_PATH=stream disables the path, =edge extends it to 64 codewords
 *   out[2] = deepest compaction level reached (0 = none; stragglers of a compact pass are
 *            compacted again, up to 3 levels)
 *   out[3] = reserved (0) */
int scaldpc_bp_last_stats(scaldpc_bp *h, int64_t *out);
/* The schedule the last decode or Monte-Carlo call ran on the tile kernels, out[SCALDPC_SCHEDULE_WORDS]: counters kept
 * on the host (no device work), reset when a call starts.  Results never depend on any of this; the words say which way
 * the early-exit scheduler went (scaldpc_bp_sched.h holds its rules):
 *   out[0..3]  tile groups run at compaction level 0 .. 3
 *   out[4..6]  codewords handed down FROM level 0 .. 2 (out[4] = scaldpc_bp_last_compacted)
 *   out[7]     host polls of the tile loop (a synchronise plus a read of a "still running" counter)
 *   out[8]     groups that stopped at the hand-over point UNSEEN (no poll: as the groups before them did)
 *   out[9]     early-exit groups that continued the stream lanes of the group before them (no fork)
 *   out[10]    early-exit groups whose lanes were left un-joined for the group after them
 *   out[11]    fixed-iteration groups that continued the lanes of the group before them
 *   out[12]    clears of the ring of counter rows after the call's first (the ring wrapped)
 *   out[13]    clears that met un-joined lanes (always 0: no group is left open into a clear)
 *   out[14]    rows of the ring during the call
 *   out[15]    host polls of the row-parallel loop
 *   out[16]    rows of the ring handed out
 *   further words reserved (0)
 * (entry point added under SCALDPC_VERSION 104: nothing that existed changed) */
#define SCALDPC_SCHEDULE_WORDS 24
int scaldpc_bp_last_schedule(scaldpc_bp *h, int64_t *out);
/* Settled codewords in the last decode or Monte-Carlo call (knob "settle"; host values, no device work).  A fixed-iteration
 * call on the record-form min-sum kernels tracks, per 64-codeword tile, the first iteration t >= 3 at which the tile is
 * FROZEN: check pass t stored the records and arg-min bytes it overwrote and variable pass t - 1 the sign masks it
 * overwrote, bit for bit, for every real codeword of the tile -- from there on every pass repeats the one before.
 *   frozen_at[min(cap, tiles)]  the frozen-at number of every tile, 0 = it never froze
 *   info[0]  tiles of the call (0 = the call did not track: early exit, another path or form, "settle" 0 -- which is
 *            also what the default means on a graph that is not [Hin | I] --, max_iter below the first test, an
 *            SCALDPC_F_ASYNC call)
 *   info[1]  kernel launches the settle horizon kept from being enqueued
 *   info[2]  tiles decoded again because they were not frozen by the horizon
 *   info[3]  the horizon K the call ran with (0 = none: device-side skipping only)
 * Results never depend on any of this. */
int scaldpc_bp_last_settle(scaldpc_bp *h, int32_t *frozen_at, int32_t cap, int64_t *info);
/* Debug: the sparse gate's tables (knob "settle_sparse") of one tile as the last call left them -- a blocking copy, to be
 * called after a synchronous call only.  info[4] = {tiles, rows, columns} the tables were laid out for (all 0 = the last
 * call did not use them) and the variable pass from which that call gated (its check passes one later: the first test in a
 * call that learns, then two passes before the smallest frozen-at number of the handle's last call on the same priors,
 * max_iter and alpha); with the three arrays NULL only info is filled.  row_stamp[rows] = the last tracked check pass in
 * which the row ran, row_dirty[rows] = the mask of its edges (by index in the row) whose message may have changed in that
 * pass, col_flag[columns] = (last tracked variable pass in which the column ran) << 1 | (its sign masks changed there). */
int scaldpc_bp_debug_sparse_flags(scaldpc_bp *h, int32_t tile, uint32_t *row_stamp, uint64_t *row_dirty, uint32_t *col_flag,
                                  int64_t *info);
/* Tuning / test knobs of one handle.  A new handle takes its defaults from the environment ONCE, at
 * creation (SCALDPC_PATH, SCALDPC_SPLIT, SCALDPC_GROUP_MB, SCALDPC_EL_MAX, SCALDPC_COMPACT_AFTER,
 * SCALDPC_FIRST_FUSED, SCALDPC_FUSE_TEST, SCALDPC_MINSUM_REC, SCALDPC_SETTLE, SCALDPC_SETTLE_HORIZON, SCALDPC_SETTLE_SPARSE); the decode entry points never read the environment.
 * Every knob selects a path, a size or a form that some graph or call still falls back to; the switches of variants
 * that were measured and rejected (round 3's test_overlap, var_form, rec_maskpos, rec_xmap, rec_sc1, fuse_finalize,
 * speculate, minsum_loop) are gone with their code (round 4; numbers in profiles/HISTORY.md), and so are the A/B-only
 * el_fuse, var_order and rec_skip1 (what their defaults chose is what runs): all are refused as unknown keys.
 * key / value (text):
 *   "path"          "auto" | "stream" (64-codeword tiles) | "edge" (row-parallel up to 64) | "lds"
 *   "split"         stream lanes per tile group (default 2)
 *   "group_mb"      budget of a cache-resident tile group in MB (default 215; large = stream from HBM)
 *   "el_max"        largest call the row-parallel kernels take (default 6 min-sum / 4 tanh)
 *   "compact_after" iteration from which stragglers may be handed to a compact pass (default 4, 0 = never); for the
 *                   float64 sweeps (scaldpc_mc_*_f64) it is the iteration AT which the one hand-over happens
 *   "fuse_test"     1 (default) = in the early-exit tile loop the convergence test of an iteration rides on the check
 *                   pass of the next one (except where the host polls or stops), with sharded accumulators;
 *                   0 = a stand-alone launch after every variable pass (what poll iterations use anyway).
 *   "minsum_rec"    1 (default) = min-sum on the 64-codeword-tile kernels in its RECORD form: the check pass writes, per
 *                   row and codeword, the two magnitudes a min-sum check sends (8 B) and, per edge and tile, two lane
 *                   masks (sign, arg-min: 0.25 B per codeword) instead of 4 B per edge and codeword; the variable pass
 *                   rebuilds every message from them, bit for bit.  0 = messages both ways (what graphs with a row
 *                   wider than 64 or a column wider than 32 use anyway).
 *                   2 = 1, and columns of 33 ... 64 edges stay in the record form: a second variable launch takes
 *                   them (k_var<64, ..> in a record mode, over the widest degree bucket), the narrower columns run the kernels they
 *                   run under 1.  Opt-in: on a graph without such a column 2 is 1, launch for launch; any value other
 *                   than 0 and 2 means 1.  Results never depend on it.
 *   "first_fused"   1 (default) = iteration 1 of the tile kernels runs without its check pass: the first variable
 *                   pass takes the first check-to-variable messages from a per-edge table (the message of a
 *                   zero-syndrome codeword) and the row's syndrome bit; 0 = check pass (reading the priors) + plain
 *                   variable pass, both in the message form (what graphs with a row or column wider than 64 use anyway,
 *                   and every scaldpc_bp_decode_batch_soft call: the table is a function of the shared priors).
 *   "settle"        fixed-iteration calls on the record-form min-sum kernels, whose message state reaches a bit-exact
 *                   fixed point on graphs with degree-1 columns: 0 = every pass runs; 1 = check and variable passes
 *                   return at once for tiles that are frozen (scaldpc_bp_last_settle), the last variable pass and the
 *                   final test run as ever (the skipping needs no host; for the query the tiles' words are read back
 *                   with one synchronise at the end of the call, except in an SCALDPC_F_ASYNC call); 2 = and from a handle's second call on the same priors, max_iter
 *                   and alpha a tile group enqueues only iterations 1 ... K, K = largest frozen-at number of the last
 *                   call + 2, and its closing passes -- while at least 7/8 of the tiles freeze by K and 2 K < max_iter.
 *                   Tiles not frozen by K are decoded again with all their iterations.
 *                   -1 (default) = 2 on a graph H = [Hin | I] (every row has an edge into a column of degree 1, which
 *                   is what bounds the messages), 0 on any other graph: it has no reason to settle and would only pay
 *                   for the compares.
 *   "settle_horizon" K > 0: that horizon, forced (0 = learned)
 *   "settle_sparse" tracked calls ("settle" 1 or 2): 1 = from the first test on, a check pass returns for every row none of
 *                   whose columns ran in the variable pass before, and a variable pass for every column of 2 ... 32 edges
 *                   none of whose messages changed in the check pass before (two small per-tile tables say which;
 *                   scaldpc_bp_debug_sparse_flags); 0 = every row and column of a tile that is not frozen runs;
 *                   -1 (default) = 1 where "settle" is 2 in force on a graph [Hin | I], else 0: where nothing freezes the
 *                   gate saves nothing and a tracked call costs about 18 % more with it (a (3,6)-regular graph).
 *   Results never depend on any of these. */
int scaldpc_bp_configure(scaldpc_bp *h, const char *key, const char *value);
/* Where a handle lives, out[4]: the device it was created on; the device (hipPointerGetAttributes)
 * of its graph allocation, of its message workspace and of its state planes (-1 = not allocated yet).
 * Every entry point switches to the handle's device for the call and restores the caller's. */
int scaldpc_bp_device_of(scaldpc_bp *h, int32_t *out);
void scaldpc_bp_destroy(scaldpc_bp *h);

/* ------------------------------------------- Monte-Carlo helpers on the device (K6) */
/*
 * The per-trial helpers of the reference's drivers -- draw the noise, form the syndrome,
 * decode, compare -- without a host round trip per trial.  Random numbers: Philox4x32-10,
 * key = seed, counter = (block, stream, GLOBAL trial index): a trial's inputs depend only
 * on (seed, first_trial + i), not on batch size or GPU count.
 *
 * scaldpc_mc_fer_run  = the body of simulate_frame_error_rate (simulate/decode.py:165-175):
 *   error_i ~ Bernoulli(channel_probs[i]) (flip iff stream-0 word i < floor(p_i 2^32)),
 *   syndrome = H error, decode, success = (decoding == error everywhere).
 *   out_error (optional) uint8 [batch][n]: the sampled error vectors.
 * scaldpc_mc_hqc_run  = synthetic hqc.decode() trials (simulate/hqc.py:684-705,742-749) on
 *   H = [Hin | I_R]: y = omega distinct positions in [0, N) (stream-1 candidates
 *   mulhi(word, N), duplicates skipped), checks = Hin y with each bit flipped with
 *   probability eps (stream 0), msg = [0]*N ++ checks, decode in received-vector mode,
 *   success = (decoded[:N] == indicator(y)).
 *   out_msg (optional) uint8 [batch][n]; out_y (optional) int32 [batch][omega], in draw order.
 * out_success uint8 [batch] required; out_iters int32 [batch] optional.
 * flags: SCALDPC_F_EARLY_EXIT, SCALDPC_F_DEVICE_IO (outputs are device pointers).
 * Refused with SCALDPC_EINVAL before anything is queued (as scaldpc_mc_qary_run and scaldpc_mc_hqc_run_soft refuse them):
 * first_trial < 0, and any flag other than these two; so are batch <= 0, an unknown method, alpha that is negative or NaN and
 * out_success = NULL.  scaldpc_mc_hqc_run also refuses omega outside [0, N], eps outside [0, 1] or NaN and a graph that does
 * not end in an identity block (SCALDPC_EINVAL), and omega > 256 (SCALDPC_EDEGREE: the sampler keeps a trial's positions in
 * LDS).  No refusal writes to an output, and the handle stays usable.
 */
int scaldpc_mc_fer_run(scaldpc_bp *h, int64_t first_trial, int32_t batch, uint64_t seed, int32_t max_iter,
                       int32_t method, float alpha, uint32_t flags, void *stream, uint8_t *out_success,
                       int32_t *out_iters, uint8_t *out_error);
int scaldpc_mc_hqc_run(scaldpc_bp *h, int32_t omega, double eps, int64_t first_trial, int32_t batch, uint64_t seed,
                       int32_t max_iter, int32_t method, float alpha, uint32_t flags, void *stream,
                       uint8_t *out_success, int32_t *out_iters, uint8_t *out_msg, int32_t *out_y);

/*
 * scaldpc_mc_hqc_run_soft = scaldpc_mc_hqc_run's trials under the law of the oracles of simulate/hqc.py:782-871: a check does
 * not arrive with one shared error rate but with a certainty of its own, and the distribution of (answer wrong?, certainty,
 * oracle calls spent) depends on the check's TRUE value.  The law is a table of K outcomes (HOST pointers whatever the flags):
 *   weights double [2][K]  row b = the probabilities of the K outcomes when the true check bit is b
 *   flips   uint8  [K]     1 = the reported bit is the complement of the true one
 *   probs   float  [K]     the prior error probability the decoder is given with the outcome (1 - certainty, hqc.py:689)
 *   costs   int32  [K]     the oracle calls the outcome spent; NULL = not counted
 *
 * Trial law (next to K6's above; a trial depends on (seed, first_trial + i) alone, not on batch, split or GPU count):
 *   secret      y exactly as scaldpc_mc_hqc_run draws it (stream 1); the true bits are c = Hin y
 *   generator   check r takes stream-0 word r of the trial: Philox counter (r >> 2, 0, trial_lo, trial_hi), word r & 3 -- the
 *               word scaldpc_mc_hqc_run uses for the flip of check r
 *   thresholds  T^b_k = thr(w[b][0] + ... + w[b][k]), the sum accumulated left to right in float64, thr(p) = floor(p 2^32), 0 for
 *               p <= 0, 2^32 for p >= 1; T^b_k is forced to 2^32 from row b's last outcome of nonzero weight on, so that an
 *               outcome of weight 0 is never drawn (the rule of scaldpc_mc_qary_run)
 *   outcome     the smallest k with word < T^b_k, b = c_r
 *   reported    c_r ^ flips[k]; column N + r of THAT trial carries the prior LLR logf((1.0f - probs[k]) / probs[k]), computed on
 *               the host in float32 as scaldpc_bp_set_channel_probs computes the handle's (p = 0 / p = 1: +-inf); the columns
 *               below N keep the handle's shared priors
 *   decode      msg = [0]*N ++ reported in received-vector mode; success = (decoded[:N] == indicator(y))
 *
 * Defining property: for every trial, out_success and out_iters are what scaldpc_bp_decode_batch_soft gives on the exported
 * out_msg with probs[out_outcome] as its last R columns (prob_cols = R) -- iterations bit for bit, for both methods and on every
 * path (LDS-resident, 64-codeword tiles, row-parallel, compact passes): the same kernels run on the same planes.
 * Reductions: K = 2, flips = (1, 0), probs = (eps, eps) and both weight rows (eps, 1 - eps) give scaldpc_mc_hqc_run(eps) exactly
 * (outcome 0 is drawn where the word is below floor(eps 2^32); the handle's priors of the check columns being eps); K = 1,
 * probs = (0) gives its eps = 0 case.
 *
 *   out_success / out_iters / out_msg / out_y   as scaldpc_mc_hqc_run's
 *   out_outcome uint8 [batch][R]  optional: the outcome drawn for every check
 *   out_flips   int32 [batch]     optional: checks reported wrong
 *   out_cost    int32 [batch]     optional: the sum of costs[outcome] over the trial's checks; needs costs
 * Validation (SCALDPC_EINVAL, nothing queued): 1 <= K <= 32; every weight finite and in [0, 1], each row summing to 1 +- 1e-6;
 * probs in [0, 1]; flips 0 or 1; costs in [0, 65535] and R * max cost < 2^31; out_cost without costs; first_trial >= 0; omega and
 * the [Hin | I] requirement as scaldpc_mc_hqc_run's.
 * flags: SCALDPC_F_EARLY_EXIT, SCALDPC_F_DEVICE_IO (the seven outputs are device pointers); anything else is refused.
 */
int scaldpc_mc_hqc_run_soft(scaldpc_bp *h, int32_t omega, const double *weights, const uint8_t *flips, const float *probs,
                            const int32_t *costs, int32_t K, int64_t first_trial, int32_t batch, uint64_t seed,
                            int32_t max_iter, int32_t method, float alpha, uint32_t flags, void *stream,
                            uint8_t *out_success, int32_t *out_iters, uint8_t *out_msg, int32_t *out_y, uint8_t *out_outcome,
                            int32_t *out_flips, int32_t *out_cost);

/*
 * scaldpc_mc_hqc_run_stats = scaldpc_mc_hqc_run_soft -- the same arguments, law, validation, refusals and flags -- that also
 * returns, per trial, the counters tracking.add_decoder_stats records after every decode (simulate/hqc.py:709-758) and,
 * optionally, the decoded word they are counted on.  Two more outputs follow scaldpc_mc_hqc_run_soft's:
 *   out_stats int32 [batch][5]  required (NULL: SCALDPC_EINVAL, nothing queued), per trial in this order:
 *               unsatisfied                   sum over checks r of reported_r
 *               good_flips                    sum over v < N of hard_v & truth_v        (truth = indicator(y))
 *               bad_flips                     sum over v < N of hard_v & ~truth_v
 *               found_bad_satisfied_checks    sum over r of hard_{N+r} & ~reported_r
 *               found_bad_unsatisfied_checks  sum over r of hard_{N+r} & reported_r
 *             hard = the error estimate of the decode; the decoded check bit is hard_{N+r} ^ reported_r (received-vector mode),
 *             so the last two are "reported 0, decoded 1" and "reported 1, decoded 0" (hqc.py:724-741).  `checks` is R and
 *             `success` is out_success: with them the row is the reference's decoder_stats row.
 *   out_bits  uint8 [batch][n]  optional: the decoded word, exactly what scaldpc_bp_decode_batch returns as out_bits for out_msg
 * The counters are a column count over three bit planes the call holds anyway (k_mc_hqc_stats): one launch after the decode; no
 * message, posterior or prior is read again.
 *
 * Defining property: for every trial i, out_stats[i] and out_success[i] are the counters and the success of the decoded word
 * bits_i = scaldpc_bp_decode_batch_soft(out_msg, probs[out_outcome], prob_cols = R) of the same handle, counted on the host from
 * (bits_i, the check part of out_msg_i, out_y_i) -- integer equality, for both methods and on every path (LDS-resident,
 * 64-codeword tiles, row-parallel, compact passes: the counters are read after the stragglers' decisions are back in place) --
 * and out_bits is bits.  Everything scaldpc_mc_hqc_run_soft returns is returned unchanged.
 * Reduction: the K = 2 table weights = ((eps, 1 - eps), (eps, 1 - eps)), flips = (1, 0), probs = (eps, eps) IS
 * scaldpc_mc_hqc_run(eps): this entry with that table returns the counters of scaldpc_mc_hqc_run's trials.
 * Growing graphs: a trial's secret does not depend on R and check r always takes stream-0 word r, so the trials of a graph of R
 * rows are the first R answers of the same trials on that graph with more rows appended (scaldpc_bp_append_rows): one seed, run
 * again after every append, follows the same keys through the attack's loop (hqc.py:953-984).
 * flags: SCALDPC_F_EARLY_EXIT, SCALDPC_F_DEVICE_IO (the nine outputs are device pointers, written on the caller's stream).
 */
int scaldpc_mc_hqc_run_stats(scaldpc_bp *h, int32_t omega, const double *weights, const uint8_t *flips, const float *probs,
                             const int32_t *costs, int32_t K, int64_t first_trial, int32_t batch, uint64_t seed,
                             int32_t max_iter, int32_t method, float alpha, uint32_t flags, void *stream,
                             uint8_t *out_success, int32_t *out_iters, uint8_t *out_msg, int32_t *out_y, uint8_t *out_outcome,
                             int32_t *out_flips, int32_t *out_cost, int32_t *out_stats, uint8_t *out_bits);

/*
 * The three sweep families decoded in the reference's own arithmetic: scaldpc_bp_decode_batch_f64's ratio-domain float64
 * recursion -- the same kernels, the same order of operations, the same test and latch -- on trials drawn on the device.  For
 * reproducing a success rate of the reference over 10^5 .. 10^6 trials, and for counting the trials on which the fp32 sweeps and
 * the reference's arithmetic disagree (driver.hqc_precision_audit), without moving a trial's inputs over PCIe.
 *   scaldpc_mc_fer_run_f64        scaldpc_mc_fer_run's trials
 *   scaldpc_mc_hqc_run_f64        scaldpc_mc_hqc_run's trials
 *   scaldpc_mc_hqc_run_stats_f64  scaldpc_mc_hqc_run_stats's trials; with out_stats = NULL it is scaldpc_mc_hqc_run_soft's sweep
 * There is no method and no alpha argument: the form is product-sum only.
 *
 * Trial law: that of the fp32 entries, word for word -- the same Philox words, thresholds, secret sampler and outcome rule.  For
 * the same (seed, first_trial + i) every exported input (out_error, out_msg, out_y, out_outcome, out_flips, out_cost) equals the
 * fp32 entry's bit for bit: precision is a property of the decode, not of the trial.
 * Decode: scaldpc_mc_fer_run_f64 and scaldpc_mc_hqc_run_f64 use the handle's shared float64 priors as ratios p / (1 - p).  In
 * scaldpc_mc_hqc_run_stats_f64 column N + r of each trial carries the ratio probs[k] / (1 - probs[k]) of its drawn outcome k, formed
 * in double by the IEEE division the per-codeword priors of scaldpc_bp_decode_batch_f64 go through; probs is DOUBLE [K] here, not
 * float: the table's certainties are taken as they are.
 *
 * Defining properties:
 *   - for every trial, out_success and out_iters are what scaldpc_bp_decode_batch_f64 gives on the exported inputs of the same
 *     handle with the same flags and max_iter (scaldpc_mc_hqc_run_stats_f64: with probs[out_outcome] as its last R columns,
 *     prob_cols = R), and out_bits is that call's out_bits -- integer equality;
 *   - out_stats is the five counters of scaldpc_mc_hqc_run_stats, counted on the decoded word of the float64 decode;
 *   - reduction: weights = ((eps, 1 - eps), (eps, 1 - eps)), flips = (1, 0), probs = (eps, eps) is scaldpc_mc_hqc_run_f64(eps) on a
 *     handle whose check columns carry eps -- exactly, because the table's probabilities are doubles.
 *
 * Stragglers: with SCALDPC_F_EARLY_EXIT, the knob "compact_after" = k > 0 and max_iter > k, every tile group stops after
 * iteration k; all codewords not latched by then are gathered over the whole call into dense tiles (syndromes, and for
 * scaldpc_mc_hqc_run_stats_f64 their rows of the ratio plane), decoded there from iteration 1 for max_iter iterations, and their
 * decisions and state are put back: one level, bit-identical (codewords are independent).  scaldpc_bp_last_compacted returns the
 * number handed over, scaldpc_bp_last_stats out[2] is 1 when any were; fixed-iteration calls never hand over.  Results never
 * depend on k, on the tile group size or on how a sweep is cut into calls.
 *
 * Refused as the fp32 entries refuse (SCALDPC_EINVAL, nothing queued, no output written, the handle usable afterwards):
 * first_trial < 0, batch <= 0, out_success = NULL, any flag other than SCALDPC_F_EARLY_EXIT | SCALDPC_F_DEVICE_IO; omega, eps and
 * the [Hin | I] requirement as scaldpc_mc_hqc_run's (omega > 256: SCALDPC_EDEGREE); K, weights, flips and costs as
 * scaldpc_mc_hqc_run_soft's, out_cost needing costs; probs outside [0, 1] or NaN.
 * Outputs as the fp32 entries'; in scaldpc_mc_hqc_run_stats_f64 out_stats is optional.
 * (entry points added under SCALDPC_VERSION 104: nothing that existed changed)
 */
int scaldpc_mc_fer_run_f64(scaldpc_bp *h, int64_t first_trial, int32_t batch, uint64_t seed, int32_t max_iter,
                           uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_iters, uint8_t *out_error);
int scaldpc_mc_hqc_run_f64(scaldpc_bp *h, int32_t omega, double eps, int64_t first_trial, int32_t batch, uint64_t seed,
                           int32_t max_iter, uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_iters,
                           uint8_t *out_msg, int32_t *out_y);
int scaldpc_mc_hqc_run_stats_f64(scaldpc_bp *h, int32_t omega, const double *weights, const uint8_t *flips,
                                 const double *probs, const int32_t *costs, int32_t K, int64_t first_trial,
                                 int32_t batch, uint64_t seed, int32_t max_iter, uint32_t flags, void *stream,
                                 uint8_t *out_success, int32_t *out_iters, uint8_t *out_msg, int32_t *out_y,
                                 uint8_t *out_outcome, int32_t *out_flips, int32_t *out_cost,
                                 int32_t *out_stats /* optional here */, uint8_t *out_bits);

/* Monte-Carlo sweeps on chosen trials: any list of global trial indices.
 *
 * Every sweep above draws trial i from (seed, first_trial + i) alone, so a trial is a pure function of its global index.  Each
 * entry below is its sibling -- the entry of the same name without "_at" -- with `const int64_t *trial_ids, int32_t batch` where
 * the sibling takes `int64_t first_trial, int32_t batch`; every other argument, the trial law, the validation, the flags and the
 * outputs are word for word the sibling's.  One difference: in scaldpc_mc_hqc_run_stats_at out_stats is OPTIONAL (as in the float64
 * entry), so that with the K = 2 table of scaldpc_mc_hqc_run_soft's reduction it covers scaldpc_mc_hqc_run(eps), and with
 * out_stats = NULL scaldpc_mc_hqc_run_soft.
 *
 * Law: slot i of the call is trial trial_ids[i] -- its Philox counter carries trial_ids[i] where the sibling's carries
 * first_trial + i.  Nothing else in any trial law changes.
 *
 * trial_ids: int64 [batch], a HOST pointer whatever the flags say (as the tables are); the call copies it to a device block the
 * handle owns (released by destroy, counted by scaldpc_debug_live_blocks).  Any order is legal; duplicates are legal (two slots
 * with the same index give the same row); indices up to 2^63 - 1 are legal.
 *
 * Defining property: for every i, every output row i of an _at call equals row trial_ids[i] - f of the sibling called with
 * first_trial = f on any range that contains the index, with the same handle, flags, max_iter, method and tables: out_success and
 * out_iters, out_flips and out_cost, out_stats, every exported input (out_error, out_msg, out_y, out_outcome, levels, secrets) and
 * out_bits / out_symbols -- integer equality, on every path (LDS-resident, 64-codeword tiles, row-parallel, every compaction
 * level, the float64 hand-over) and in every q-ary kernel form.  Only the generator kernels know trial indices; the decode,
 * compaction, compare and statistics kernels work on the slots of the call.
 *
 * Refused with SCALDPC_EINVAL before anything is queued (no output is written, the handle stays usable): trial_ids = NULL; a
 * negative index (the message names its position and its value); everything the sibling refuses.  The f64 entries (as all binary
 * sweeps) and the q-ary entries refuse SCALDPC_F_ASYNC.
 * (entry points added under SCALDPC_VERSION 104: nothing that existed changed)
 */
int scaldpc_mc_fer_run_at(scaldpc_bp *h, const int64_t *trial_ids, int32_t batch, uint64_t seed, int32_t max_iter,
                          int32_t method, float alpha, uint32_t flags, void *stream, uint8_t *out_success,
                          int32_t *out_iters, uint8_t *out_error);
int scaldpc_mc_hqc_run_stats_at(scaldpc_bp *h, int32_t omega, const double *weights, const uint8_t *flips, const float *probs,
                                const int32_t *costs, int32_t K, const int64_t *trial_ids, int32_t batch, uint64_t seed,
                                int32_t max_iter, int32_t method, float alpha, uint32_t flags, void *stream,
                                uint8_t *out_success, int32_t *out_iters, uint8_t *out_msg, int32_t *out_y,
                                uint8_t *out_outcome, int32_t *out_flips, int32_t *out_cost,
                                int32_t *out_stats /* optional here */, uint8_t *out_bits);
int scaldpc_mc_fer_run_at_f64(scaldpc_bp *h, const int64_t *trial_ids, int32_t batch, uint64_t seed, int32_t max_iter,
                              uint32_t flags, void *stream, uint8_t *out_success, int32_t *out_iters, uint8_t *out_error);
int scaldpc_mc_hqc_run_stats_at_f64(scaldpc_bp *h, int32_t omega, const double *weights, const uint8_t *flips,
                                    const double *probs, const int32_t *costs, int32_t K, const int64_t *trial_ids,
                                    int32_t batch, uint64_t seed, int32_t max_iter, uint32_t flags, void *stream,
                                    uint8_t *out_success, int32_t *out_iters, uint8_t *out_msg, int32_t *out_y,
                                    uint8_t *out_outcome, int32_t *out_flips, int32_t *out_cost,
                                    int32_t *out_stats /* optional */, uint8_t *out_bits);

/* ------------------------------------------------------------ q-ary min-sum */
typedef struct scaldpc_qary scaldpc_qary;

/* H: int8 [R][N] dense row-major with entries in {-1,0,+1} (what pydecoder.rs:24
 * receives), Q = 2B+1 symbols, `iterations` fixed (no early exit, decoder.rs:660). */
int scaldpc_qary_create(int32_t R, int32_t N, int32_t B, const int8_t *H, int32_t iterations,
                        scaldpc_qary **out);
/* pmf: float [batch][N][Q] probabilities (LLR conversion inside, as pydecoder.rs:60);
 * out: int8 [batch][N] hard decisions in [-B, B]. */
int scaldpc_qary_min_sum_batch(scaldpc_qary *h, const float *pmf, int32_t batch, uint32_t flags,
                               void *stream, int8_t *out);
void scaldpc_qary_destroy(scaldpc_qary *h);
/* The probability -> LLR conversion both decoders apply to their inputs, on its own:
 * llr[r][q] = ln(max_q' pmf[r][q'] / pmf[r][q]) in f32 (+inf where pmf = 0); pmf, llr: float [rows][Q].
 * Runs on the device with glibc's logf algorithm and the correctly rounded f32 division, so the values
 * are bit for bit those of the host's logf (what the reference's f32::ln calls).  A row that does not
 * sum to 1 +- 1e-3 returns SCALDPC_EPMF (the reference asserts).  flags: SCALDPC_F_DEVICE_IO. */
int scaldpc_qary_into_llr(const float *pmf, int64_t rows, int32_t Q, uint32_t flags, void *stream, float *llr);
/* Test / tuning knobs of one q-ary handle (defaults from SCALDPC_QARY_WAVE / SCALDPC_QARY_NO_UNROLL / SCALDPC_QARY_NO_TREE,
 * read once at creation):
 *   "wave"       -1 auto | 0 codeword per lane | 1 wave per (check, codeword)
 *   "unroll"     1 register-resident unrolled enumeration for small alphabets | 0 off
 *   "tree"       1 tree-walk check kernel for the Kyber shape (B = 2, six coefficient edges per check) | 0 off
 *   "dp"         1 (default) the same shape's check update as a min-plus recursion over the edges in the reference's order
 *                of additions -- no enumeration, the reference's messages bit for bit (scaldpc_qary_special.h) | 0 off
 *   "dp_min"     ... for calls of at least this many codewords (default 5; below, the tree walk)
 *   "dp_split"   ... the row's edges split over four waves up to this many codewords (default 64)
 *   "dp_split2"  ... and over two up to this many (default 192)
 *   "dp_any"     DecoderSpecial, B = 1, 2, 3: the min-plus recursion for rows of ANY number of coefficient edges, tables in LDS
 *                (k_q_special_check_dp_any, one launch for every row of the graph).  -1 (default) for graphs with a check of more
 *                than 8 edges, which no other kernel takes | 1 for every such decoder | 0 never (a call on a graph with a check
 *                of more than 8 edges then returns SCALDPC_EDEGREE before anything is queued)
 *   "llr_tiled", "var_small"  forms of the conversion / variable kernels
 *   "timing"     1: bracket the launches of a call with HIP events (scaldpc_qary_last_timing)
 * LDS limits (no launch of a call asks for more than 64 KB of dynamic LDS; the plan is made before anything is queued):
 *   enumeration, codeword per lane: maxdc * Q * 9 B per codeword (DecoderSpecial: 2 * ((maxdc - 1) * Q + QS) * 4 B); a block
 *                takes 64 codewords, halved down to 8 while that exceeds 64 KB; what does not fit at 8 returns SCALDPC_EDEGREE
 *   enumeration, wave per (check, codeword): used where its tables fit 64 KB (and the check has at most 8 edges), else the above
 *   variable update, generic kernel (k_q_var): two rows of W = max(Q, QS) floats per codeword, 2 * W * 4 B; a block takes 64
 *                codewords, halved while that exceeds 64 KB: 64 up to W = 128, 32 beyond (W = 255: 65 280 B) */
int scaldpc_qary_configure(scaldpc_qary *h, const char *key, const char *value);
/* Measurement aid for bench.py (the q-ary counterpart of scaldpc_bp_time_kernels): after
 * scaldpc_qary_configure(h, "timing", "1"), every check-node and variable-node launch of a call is bracketed by
 * HIP events on the launch stream (off by default -- the product path records nothing).  For the last call:
 *   ms[0] / ms[1]  total ms of its check / variable launches;  ms[2]  from the first check launch to the last
 *                  variable launch (the iteration loop, without the probability -> LLR conversion and the copies)
 *   info[0] iterations run;  info[1] check kernel: 0 k_q_check_unrolled<3,7>, 1 k_q_check_unrolled<5,5>,
 *           2 k_q_special_check_tree<5,6> (+ wave kernel for other row degrees), 3 k_q_special_check_wave,
 *           4 k_q_check_wave, 5 k_q_special_check, 6 k_q_check, 7 k_q_special_check_dp<5,6> (either form), 8 k_q_check_dp<3,7>,
 *           9 k_q_special_check_dp_any;  info[2] batch;  info[3] largest check degree */
int scaldpc_qary_last_timing(scaldpc_qary *h, float *ms, int32_t *info);

/* DecoderSpecial: H = [H' | I_R]; first N-R variables over [-B,B], last R over [-BSUM,BSUM].
 * Checks of up to 8 edges (7 coefficient edges + the row-sum edge): any B, the enumeration kernels.  Longer checks: B = 1, 2, 3
 * with 2 B (degree - 1) + 1 <= 85 (three LDS tables of that many entries x 64 codewords within 64 KB: 42 / 21 / 14 coefficient
 * edges at B = 1 / 2 / 3), on the min-plus recursion for rows of any length; anything else returns SCALDPC_EDEGREE. */
int scaldpc_qary_special_create(int32_t R, int32_t N, int32_t B, int32_t BSUM, const int8_t *H,
                                int32_t iterations, scaldpc_qary **out);
/* pmf_b: float [batch][N-R][2B+1]; pmf_sum: float [batch][R][2BSUM+1]; out int8 [batch][N]. */
int scaldpc_qary_special_min_sum_batch(scaldpc_qary *h, const float *pmf_b, const float *pmf_sum,
                                       int32_t batch, uint32_t flags, void *stream, int8_t *out);

/* Soft output of both q-ary decoders.  `out` is required and is byte for byte what the plain call returns; each of the
 * other outputs is optional (NULL), and with all of them NULL the call IS the plain call.
 *   out_cost    float [batch][N][Q]: the raw totals of the LAST variable update (decoder.rs:634-658), sum[q] = channel LLR +
 *               the incoming check messages added in the reference's order (the column's checks in ascending row), the very
 *               numbers whose first minimum (decoder.rs:694-704) is the symbol.  Index q stands for the value q - B.  Not
 *               normalised: on a cycle-free graph a row minus its minimum is the exact min-marginal cost difference.  +inf
 *               (zero-probability symbols, decoder.rs:688) and NaN entries come out as the arithmetic makes them.
 *               DecoderSpecial (decoder_special.rs:566-609): two arrays shaped like its two inputs, out_cost_b float
 *               [batch][N-R][2B+1] and out_cost_sum float [batch][R][2BSUM+1] (index q: the value q - BSUM); pass both or
 *               neither (else SCALDPC_EINVAL).
 *   out_margin  float [batch][N]: fl(m2 - m1), m1 the total at the decided symbol, m2 the smallest total over the OTHER
 *               symbols by the reference's own scan rule (strict <, NaN never selected, +inf if there is no candidate):
 *               two equal minima give 0.  The q-ary counterpart of |LLR|, N floats per codeword instead of N * Q.
 *   out_unmet   int32 [batch]: the number of checks whose sum of h_e * x_e over the row's edges, OVER THE INTEGERS (the
 *               constraint the check updates enumerate, decoder.rs:336-337; DecoderSpecial: the row-sum variable's edge
 *               included, decoder_special.rs:507-522), is nonzero on the returned symbols.  0: the decision is a valid word.
 * flags: SCALDPC_F_DEVICE_IO applies to the input and to every output alike; SCALDPC_F_ASYNC is refused (SCALDPC_EINVAL):
 * a q-ary call is synchronous.  SCALDPC_EPMF / SCALDPC_ENOCONF / SCALDPC_EINVAL are reported as by the plain calls.  The
 * staging buffers of an output are allocated by the first call that asks for it. */
int scaldpc_qary_min_sum_batch_soft(scaldpc_qary *h, const float *pmf, int32_t batch, uint32_t flags, void *stream,
                                    int8_t *out, float *out_cost, float *out_margin, int32_t *out_unmet);
int scaldpc_qary_special_min_sum_batch_soft(scaldpc_qary *h, const float *pmf_b, const float *pmf_sum, int32_t batch,
                                            uint32_t flags, void *stream, int8_t *out,
                                            float *out_cost_b, float *out_cost_sum, float *out_margin, int32_t *out_unmet);

/* ------------------------------------------- Monte-Carlo trials of the q-ary decoders on the device */
/*
 * `batch` trials of the reference's q-ary sweep (simulate/decode.py:246-257: an all-zero word whose symbols each carry one of a
 * few pmf rows) without a [batch][N][Q] input and without a [batch][N] output.  Every variable draws a LEVEL of its table:
 *   levels_b  float  [k_b][2B+1]     the pmf rows of the coefficient variables (the plain decoder: of every variable)
 *   weights_b double [k_b]           the probability of each row
 *   levels_s / weights_s / k_s       the same for DecoderSpecial's row-sum variables, [k_s][2BSUM+1]; a plain handle takes
 *                                    NULL, NULL, 0 and nothing else
 * and the call decodes the word so made.  Tables and weights are HOST pointers whatever the flags say.
 *
 * Trial law (next to K6's above; a trial depends on (seed, first_trial + i) alone, not on batch, split or GPU count):
 *   generator   Philox4x32-10, key = seed, counter = (x >> 2, 0, trial_lo, trial_hi): stream 0, word x & 3, with x the graph
 *               variable index 0 .. N-1 (DecoderSpecial's row-sum variables continue at N-R) and the GLOBAL trial index
 *   thresholds  T_k = thr(w_0 + ... + w_k), the sum accumulated left to right in float64, thr(p) = floor(p 2^32), 0 for p <= 0,
 *               2^32 for p >= 1 (the rule of scaldpc_mc_fer_run); T_{K-1} is forced to 2^32 -- and so is every T_k from the last
 *               level of nonzero weight on, so that a level of weight 0 is never drawn
 *   level       the smallest k with word < T_k
 * With K = 2, rows (bad, good) and weights (error_rate, 1 - error_rate), "bad" is drawn exactly where stream-0 word x of the
 * trial is below floor(error_rate 2^32) -- the Bernoulli draw of scaldpc_mc_fer_run -- and out_errs is the reference's `errs`.
 *
 * Defining property: for every trial, out_symbols is what scaldpc_qary_min_sum_batch / scaldpc_qary_special_min_sum_batch
 * returns for the materialised input pmf[i][v] = levels[out_levels[i][v]], bit for bit, in every kernel form and at any split of
 * the trials into calls.  (The K (+ K_s) rows are converted to LLRs by the conversion of scaldpc_qary_into_llr, once: a call
 * whose tables are bit for bit those of the handle's last finished call -- every chunk of a sweep -- reuses the converted rows.)
 *
 *   out_success uint8 [batch]     required: 1 iff every decided symbol is 0
 *   out_errs    int32 [batch]     optional: variables drawn at a level other than the LAST of their table
 *   out_wrong   int32 [batch]     optional: decided symbols != 0
 *   out_levels  uint8 [batch][N]  optional: the level drawn for every variable
 *   out_symbols int8  [batch][N]  optional: the decisions
 * Validation (SCALDPC_EINVAL, nothing queued): 1 <= K <= 16 per table; every weight finite and in [0, 1]; |sum w - 1| <= 1e-6;
 * first_trial >= 0; a plain handle refuses levels_s, a special handle requires it.  A table row that fails the reference's pmf
 * test (decoder.rs:683-684) returns SCALDPC_EPMF and names the table and the level.
 * flags: SCALDPC_F_DEVICE_IO: the five outputs are device pointers; SCALDPC_F_ASYNC is refused (SCALDPC_EINVAL).
 * SCALDPC_ENOCONF is reported as by the plain call.
 */
int scaldpc_mc_qary_run(scaldpc_qary *h, const float *levels_b, const double *weights_b, int32_t k_b,
                        const float *levels_s, const double *weights_s, int32_t k_s,
                        int64_t first_trial, int32_t batch, uint64_t seed, uint32_t flags, void *stream,
                        uint8_t *out_success, int32_t *out_errs, int32_t *out_wrong, uint8_t *out_levels,
                        int8_t *out_symbols);

/* ------------------------------------------- Monte-Carlo trials of DecoderSpecial on drawn secrets under an oracle's law */
/*
 * `batch` trials of the Kyber attack's decode on the device (special handles only): a SECRET is drawn, every variable is
 * answered by an oracle outcome drawn CONDITIONAL on the variable's true symbol, the outcome's pmf row goes to the decoder,
 * and the decision is compared with the secret.  Tables and prior are HOST pointers whatever the flags say.
 *   prior_b   double [Q]        Q = 2B+1: the law of a coefficient's true symbol, index q = value q - B
 *   levels_b  float  [k_b][Q]   the pmf row outcome k hands the decoder (the posterior given that answer)
 *   weights_b double [Q][k_b]   row s: the law of the outcome of a coefficient variable whose TRUE symbol is s
 *   levels_s  float  [k_s][QS]  QS = 2BSUM+1: the same for the row-sum variables (index q = value q - BSUM)
 *   weights_s double [QS][k_s]  row s: TRUE row-sum symbol s
 *
 * Trial law (next to the others; a trial depends on (seed, first_trial + i) alone, not on batch, split or GPU count):
 *   generator   Philox4x32-10, key = seed, the GLOBAL trial index, as scaldpc_mc_qary_run
 *   secret      coefficient variable v < N-R: stream 1 word v, i.e. counter (v >> 2, 1, trial_lo, trial_hi), word v & 3; the symbol
 *               is the smallest q with word < T_q, T the cumulative thresholds of prior_b by the rule of scaldpc_mc_qary_run
 *               (left-to-right float64 sum, thr, 2^32 from the last nonzero entry on)
 *               row-sum variable N-R+r: the one value that makes check r hold over the integers,
 *               t_r = -h_{r,id} * sum_j h_{r,j} s_j  (h_{r,id} = +-1 the row's identity entry, j over its coefficient edges);
 *               creation guarantees (degree - 1) B <= BSUM, so t_r lies inside the alphabet: every drawn word is a valid word
 *   outcome     variable x: stream 0 word x, the word scaldpc_mc_qary_run draws x's level from; the outcome is the
 *               smallest k with word < T^s_k, s the index of the variable's TRUE symbol: row s of weights_b (x < N-R) or of weights_s, every
 *               row through the threshold rule on its own -- an outcome of weight 0 in that row is never drawn under that symbol
 *   decode      outcome k hands the decoder levels[k]; the rows are converted once per table by the conversion of
 *               scaldpc_qary_into_llr (and kept over the chunks of a sweep, as scaldpc_mc_qary_run keeps them)
 *
 * Defining property: out_symbols is bit for bit what scaldpc_qary_special_min_sum_batch returns for
 * pmf_b[i][v] = levels_b[out_levels[i][v]] and pmf_sum[i][r] = levels_s[out_levels[i][N-R+r]], in every kernel form and at any
 * split of the trials into calls.
 * Reduction: with prior_b a point mass on the value 0, all rows of weights_b equal and all rows of weights_s equal, the call draws
 * the levels and the symbols of scaldpc_mc_qary_run with those weights, trial for trial; that call's out_wrong is
 * out_wrong[i][0] + out_wrong[i][1] here, and its out_success says whether that sum is 0.
 *
 *   out_success       uint8 [batch]     required: out_wrong[i][0] == 0 -- the key is recovered
 *   out_wrong         int32 [batch][2]  optional: decided != secret over the coefficient variables, over the row-sum variables
 *   out_channel_wrong int32 [batch][2]  optional: variables whose drawn row ALONE decides wrong -- the first maximum of the pmf
 *                                       row (the arg-min rule of decoder.rs:694-704 on its LLR row) is not the secret
 *   out_secret        int8  [batch][N]  optional: the secret values (row-sum variables last)
 *   out_levels        uint8 [batch][N]  optional: the outcome drawn for every variable
 *   out_symbols       int8  [batch][N]  optional: the decisions
 * Refused before anything is queued (the handle keeps working, no output is written):
 *   SCALDPC_EINVAL   NULL prior_b, table or out_success; a plain (non-special) handle: without row-sum variables a drawn secret
 *                    is no code word; k outside 1 .. 32 per table; the prior or a row of weights with an entry that is no
 *                    probability or a sum outside 1 +- 1e-6 (the message names the table and the row); first_trial < 0;
 *                    batch <= 0; SCALDPC_F_ASYNC
 *   SCALDPC_EPMF     a level that fails the reference's pmf test (decoder.rs:683-684; the message names table and level)
 *   SCALDPC_EDEGREE  a table of K levels over Q symbols with 4 (2 K Q + Q) > 65536: a launch keeps the table's LLR rows, its
 *                    thresholds per true symbol and their counts in dynamic LDS, 64 KB at the most (k_s = 32 with QS >= 253)
 * flags: SCALDPC_F_DEVICE_IO: the six outputs are device pointers.  SCALDPC_ENOCONF is reported as by the plain call.
 */
int scaldpc_mc_qary_run_secret(scaldpc_qary *h, const double *prior_b,
                               const float *levels_b, const double *weights_b, int32_t k_b,
                               const float *levels_s, const double *weights_s, int32_t k_s,
                               int64_t first_trial, int32_t batch, uint64_t seed, uint32_t flags, void *stream,
                               uint8_t *out_success, int32_t *out_wrong, int32_t *out_channel_wrong,
                               int8_t *out_secret, uint8_t *out_levels, int8_t *out_symbols);

/* The two q-ary sweeps on chosen trials: scaldpc_mc_qary_run and scaldpc_mc_qary_run_secret with `const int64_t *trial_ids`
 * (int64 [batch], a HOST pointer whatever the flags say, copied to a device block the handle owns) where they take
 * `int64_t first_trial`; everything else is word for word the sibling's.  Slot i of the call is trial trial_ids[i]: its Philox
 * counters carry trial_ids[i] where the sibling's carry first_trial + i.  Any order, duplicates and indices up to 2^63 - 1 are legal.
 * Defining property: for every i, every output row i (success, errs / wrong / channel_wrong, levels, secret, symbols) equals row
 * trial_ids[i] - f of the sibling called with first_trial = f on any range that contains the index, with the same handle, flags
 * and tables, in every kernel form -- integer equality.
 * Refused with SCALDPC_EINVAL before anything is queued (no output written, the handle usable): trial_ids = NULL, a negative index
 * (the message names its position and its value), and everything the sibling refuses, SCALDPC_F_ASYNC included.
 * (entry points added under SCALDPC_VERSION 104: nothing that existed changed)
 */
int scaldpc_mc_qary_run_at(scaldpc_qary *h, const float *levels_b, const double *weights_b, int32_t k_b,
                           const float *levels_s, const double *weights_s, int32_t k_s,
                           const int64_t *trial_ids, int32_t batch, uint64_t seed, uint32_t flags, void *stream,
                           uint8_t *out_success, int32_t *out_errs, int32_t *out_wrong, uint8_t *out_levels,
                           int8_t *out_symbols);
int scaldpc_mc_qary_run_secret_at(scaldpc_qary *h, const double *prior_b,
                                  const float *levels_b, const double *weights_b, int32_t k_b,
                                  const float *levels_s, const double *weights_s, int32_t k_s,
                                  const int64_t *trial_ids, int32_t batch, uint64_t seed, uint32_t flags, void *stream,
                                  uint8_t *out_success, int32_t *out_wrong, int32_t *out_channel_wrong,
                                  int8_t *out_secret, uint8_t *out_levels, int8_t *out_symbols);

#ifdef __cplusplus
}
#endif
#endif /* SCALDPC_H */
