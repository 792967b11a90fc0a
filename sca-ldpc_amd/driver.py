"""Batched counterparts of the reference's Monte-Carlo drivers -- the callers either
side of the decode path.  Same inputs, same RNG consumption, same
success criteria and statistics as the reference, but every trial of a run goes to the
decoder in ONE batched call.

  ErrorsProvider                  simulate/decode.py:9-127
  simulate_frame_error_rate       simulate/decode.py:130-177  (binary FER loop)
  simulate_frame_error_rate_rust  simulate/decode.py:180-286  (q-ary FER loop)
  qary_fer_sweep                  the same loop, its trials drawn on the device (Philox, sharded by global trial index)
  hqc_decode                      simulate/hqc.py:661-759      (input assembly + 7 stats fields)
  hqc_decode_batch                the same for many trials with their own certainties, one soft call
  hqc_oracle_sweep                such trials at a fixed number of checks, answered by the wrapped oracle's law
                                  (simulate/hqc.py:782-871) on the device: successes, iterations, oracle calls spent
  hqc_attack_curve                the same trials followed through the attack loop (simulate/hqc.py:953-984) on ONE growing
                                  decoder: checks needed per key, and the reference's decoder_stats table, counted on the device
  regular_ldpc_code & co          main.py:189-276              (the four FER commands, as functions)

The decoder classes are parameters (default: the HIP decoders) so that the host logic
can be exercised without a GPU by injecting any object with the same surface.
"""
from __future__ import annotations

import itertools
import re

import numpy as np

from . import codes
from .graph import TannerGraph


class ErrorsProvider:
    """simulate/decode.py:9-127.  `get_error(pos)` consumes exactly one `rng.rand()`;
    `get_errors(runs, n)` draws `runs*n` uniforms in the same order (row-major) and is
    therefore stream-identical to the reference's nested loops (decode.py:165-167)."""

    def __init__(self, error_rate, error_file, rng):
        self.error_rate = error_rate
        self.error_distribution = None
        self.rng = rng
        if error_file is not None:
            dist = []
            with open(error_file, "rt") as f:
                for line in f:
                    line = line.strip()
                    if line:
                        dist.append([float(x) for x in re.split("[, ]+", line)])
            self.error_distribution = dist

    @classmethod
    def from_distribution(cls, distribution, rng, error_rate=None):
        self = cls(error_rate, None, rng)
        self.error_distribution = [list(map(float, row)) for row in distribution]
        return self

    def get_error(self, pos):
        if self.error_distribution is None:
            return 1 if self.rng.rand() < self.error_rate else 0
        pr = self.error_distribution[pos % len(self.error_distribution)]
        if len(pr) == 1:
            return 1 if self.rng.rand() < pr[0] else 0
        rand = self.rng.rand()
        res = -(len(pr) // 2)
        threshold = 0
        for p in pr:
            threshold += p
            if threshold > rand:
                return res
            res += 1
        return None  # the reference falls off the loop the same way when rand >= sum(pr)

    def get_errors(self, runs, n):
        """[runs, n] errors, same uniforms in the same order as runs*n get_error calls."""
        u = self.rng.rand(runs, n)
        if self.error_distribution is None:
            return (u < self.error_rate).astype(np.int64)
        L = len(self.error_distribution)
        widths = {len(r) for r in self.error_distribution}
        if widths == {1}:
            thr = np.array([self.error_distribution[i % L][0] for i in range(n)])
            return (u < thr[None, :]).astype(np.int64)
        out = np.empty((runs, n), dtype=np.int64)
        for i in range(n):
            pr = self.error_distribution[i % L]
            if len(pr) == 1:
                out[:, i] = u[:, i] < pr[0]
            else:
                cum = np.cumsum(np.asarray(pr))  # threshold += p, `threshold > rand`
                out[:, i] = (cum[None, :] > u[:, i : i + 1]).argmax(axis=1) - len(pr) // 2
        return out

    def get_error_rate(self):
        return self.error_rate if self.error_distribution is None else None

    def get_binary_channel_probs(self, n=None):
        if self.error_distribution is None:
            return [None]
        if len(self.error_distribution[0]) != 1:
            raise ValueError("Distribution from the file isn't binary")
        if n is None:
            return [x[0] for x in self.error_distribution]
        it = itertools.cycle(self.error_distribution)
        return [next(it)[0] for _ in range(n)]


def _default_bp():
    from .bp import bp_decoder

    return bp_decoder


def simulate_frame_error_rate(H, errors_provider, runs, rng, bp_decoder=None):
    """simulate/decode.py:130-177: number of frames decoded exactly.  `rng` is the one
    held by `errors_provider` (the reference passes it twice as well)."""
    g = TannerGraph.coerce(H)
    n = g.n
    bpd = (bp_decoder or _default_bp())(
        g,
        error_rate=errors_provider.get_error_rate(),
        max_iter=n,
        bp_method="product_sum",
        channel_probs=errors_provider.get_binary_channel_probs(n),
    )
    error = errors_provider.get_errors(runs, n)
    syndrome = g.syndrome(error.astype(np.uint8))
    decoding = bpd.decode_batch(syndrome, early_exit=True, input_vector_type="syndrome")["bits"]
    return int((decoding == error).all(axis=1).sum())


def simulate_frame_error_rate_rust(H, B, error_rate, runs, rng, threads=1, decoder_class=None):
    """simulate/decode.py:180-286: all-zero codeword with noisy symbols; frames without a
    bad symbol are skipped (but their draws are consumed), success = all-zero decoding.
    `threads` is accepted for signature parity; the batch replaces the thread pool."""
    Hd = H.to_dense(np.int8) if isinstance(H, TannerGraph) else np.asarray(H)
    r, n = Hd.shape
    v = int(np.count_nonzero(Hd, axis=0).max())
    c = int(np.count_nonzero(Hd, axis=1).max())
    B = 1  # decode.py:222 overrides the argument
    BB = 2 * B + 1
    iterations = 5
    name = f"DecoderN{n}R{r}V{v}C{c}B{B}"
    if decoder_class is None:
        from .qary import decoder_class as _dc

        decoder_class = _dc
    decoder = decoder_class(name)(Hd.astype(np.int8), iterations)
    p = 1 / BB
    good = np.full(BB, p)
    bad = np.full(BB, p)
    good[[B, -1]] = [1.75 * p, 0.25 * p]
    bad[[-1, B]] = [1.75 * p, 0.25 * p]
    frames = []
    while len(frames) < runs:
        mask = rng.rand(n) < error_rate
        if not mask.any():
            continue
        frames.append(np.where(mask[:, None], bad, good).astype(np.float32))
    decoding = decoder.min_sum_batch(np.stack(frames))
    return int((decoding == 0).all(axis=1).sum())


def qary_fer_sweep(H, B, error_rate, runs, seed, chunk=4096, decoder_class=None):
    """The loop of simulate/decode.py:246-277 with its trials drawn on the device (`mc_run`; the generator is Philox keyed by
    (seed, global trial index), not the reference's MT19937 stream: `simulate_frame_error_rate_rust` keeps that one).
    Global trial indices 0, 1, ... are scanned `chunk` at a time; frames without a bad symbol are skipped as the reference
    skips them (decode.py:258-259), and the FIRST `runs` frames with one are counted.  Returns dict(successes,
    max_errs_success, min_errs_fail (None: nothing failed) -- the three numbers of decode.py:265-286 -- and trials_drawn, the
    index behind the last counted frame).  The result does not depend on `chunk`."""
    Hd = H.to_dense(np.int8) if isinstance(H, TannerGraph) else np.asarray(H)
    r, n = Hd.shape
    v = int(np.count_nonzero(Hd, axis=0).max())
    c = int(np.count_nonzero(Hd, axis=1).max())
    B = 1  # decode.py:222 overrides the argument
    BB = 2 * B + 1
    if not 0.0 < error_rate <= 1.0:
        raise ValueError("error_rate must be in (0, 1]: a frame without a bad symbol is never counted")
    if runs < 0 or chunk < 1:
        raise ValueError("runs must not be negative and chunk must be positive")
    if decoder_class is None:
        from .qary import decoder_class as _dc

        decoder_class = _dc
    decoder = decoder_class(f"DecoderN{n}R{r}V{v}C{c}B{B}")(Hd.astype(np.int8), 5)
    p = 1 / BB
    good = np.full(BB, p)
    bad = np.full(BB, p)
    good[[B, -1]] = [1.75 * p, 0.25 * p]
    bad[[-1, B]] = [1.75 * p, 0.25 * p]
    levels = np.stack([bad, good]).astype(np.float32)  # the last level is the good row: `errs` counts the bad symbols
    weights = np.array([error_rate, 1.0 - error_rate])
    res = dict(successes=0, max_errs_success=0, min_errs_fail=None, trials_drawn=0)
    counted, first = 0, 0
    try:
        while counted < runs:
            out = decoder.mc_run(chunk, seed, levels, weights, first_trial=first)
            errs, ok = np.asarray(out["errs"]), np.asarray(out["success"]).astype(bool)
            framed = np.flatnonzero(errs > 0)[: runs - counted]
            if framed.size:
                e, s = errs[framed], ok[framed]
                res["successes"] += int(s.sum())
                if s.any():
                    res["max_errs_success"] = max(res["max_errs_success"], int(e[s].max()))
                if (~s).any():
                    low = int(e[~s].min())
                    res["min_errs_fail"] = low if res["min_errs_fail"] is None else min(res["min_errs_fail"], low)
                counted += framed.size
                res["trials_drawn"] = first + int(framed[-1]) + 1
            first += chunk
    finally:
        if hasattr(decoder, "close"):
            decoder.close()
    return res


def kyber_fer_sweep(H, name, iterations, prior, table_b, table_s, runs, seed, chunk=4096, decoder_class=None):
    """A sweep of the Kyber attack's decode (simulate/kyber.py) on drawn secrets: per trial a secret from `prior`
    (`trials.centered_binomial`), the row sums that follow from it and H, every variable answered by an outcome of its table
    (`trials.oracle_posterior_table`: table_b for the coefficients, table_s -- built with reverse=True -- for the row sums)
    drawn on the device conditional on the variable's true value (`QarySpecialDecoder.mc_run_secret`).  `name` is the decoder's
    (e.g. "DecoderN1280R512SW6").  Global trial indices 0 .. runs - 1 are scanned `chunk` at a time; the result does not depend
    on `chunk`.  Returns dict(
      runs, successes       trials, and those whose every coefficient was decided as drawn (the key is recovered),
      wrong_hist            int64 [N - R + 1]: trials by their number of wrong coefficients after decoding,
      channel_wrong, wrong  wrong coefficients over all trials: from the drawn rows alone, and after decoding)."""
    Hd = H.to_dense(np.int8) if isinstance(H, TannerGraph) else np.asarray(H)
    r, n = Hd.shape
    if runs < 0 or chunk < 1:
        raise ValueError("runs must not be negative and chunk must be positive")
    if decoder_class is None:
        from .qary import decoder_class as _dc

        decoder_class = _dc
    decoder = decoder_class(name)(Hd.astype(np.int8), iterations)
    hist = np.zeros(n - r + 1, dtype=np.int64)
    successes = channel_wrong = wrong = 0
    try:
        for first in range(0, runs, chunk):
            out = decoder.mc_run_secret(min(chunk, runs - first), seed, prior, table_b["levels"], table_b["weights"], table_s["levels"],
                                        table_s["weights"], first_trial=first)
            w = np.asarray(out["wrong"], dtype=np.int64)[:, 0]
            successes += int(np.asarray(out["success"]).astype(bool).sum())
            hist += np.bincount(w, minlength=n - r + 1)
            wrong += int(w.sum())
            channel_wrong += int(np.asarray(out["channel_wrong"], dtype=np.int64)[:, 0].sum())
    finally:
        if hasattr(decoder, "close"):
            decoder.close()
    return dict(runs=int(runs), successes=successes, wrong_hist=hist, channel_wrong=channel_wrong, wrong=wrong)


def hqc_oracle_sweep(Hin, N, omega, table, runs, seed, chunk=4096, bp_method="product_sum", max_iter=100, bp_decoder=None,
                     want_stats=False, precision=None):
    """A sweep of synthetic hqc.decode() trials at a FIXED number of checks (the rows of Hin) under the law of the attack's
    oracle: every check is answered by an outcome of `table` (`trials.wrapped_oracle_table`: the repeated measurements of
    wrapped_hqc_decoding_oracle, simulate/hqc.py:782-871), drawn on the device conditional on the check's true value, and
    brings its own certainty into the decode (`BpDecoder.mc_hqc_run_soft`).  Global trial indices 0 .. runs - 1 are scanned
    `chunk` at a time; the result does not depend on `chunk`.  Returns dict(
      runs, successes,
      iter_hist           int64 [max_iter + 1]: trials by the iteration count of their decode,
      flips               checks reported wrong, over all trials,
      oracle_calls, oracle_calls_mean                  total and per trial, over all trials,
      oracle_calls_success, oracle_calls_success_mean  the same over the successful trials (mean None: none succeeded);
    the four oracle-call fields are None when the table has no costs).  What the paper's plots report -- oracle calls per
    recovered key -- is oracle_calls / successes.
    want_stats: the sweep also counts, on the device, what tracking.add_decoder_stats records per decode (hqc.py:709-758); the
    result gains `stats` and `stats_success`: {counter: total} over all trials and over the successful ones, the counters
    being HQC_STATS_COLUMNS.
    precision: None (the call as it always was: the fp32 kernels), "float32" or "float64" -- handed to
    `BpDecoder.mc_hqc_run_soft`: the same trials decoded by the reference's float64 recursion, product-sum only."""
    g = TannerGraph.coerce(Hin)
    if g.n != N:
        raise ValueError(f"Hin has {g.n} columns, N = {N}")
    if runs < 0 or chunk < 1:
        raise ValueError("runs must not be negative and chunk must be positive")
    # the check columns' shared priors are replaced per trial: any probability does
    shared = np.concatenate([np.full(N, omega / N, dtype=np.float64), np.full(g.m, 0.5, dtype=np.float64)])
    bpd = (bp_decoder or _default_bp())(g.with_identity(), max_iter=max_iter, bp_method=bp_method, channel_probs=shared)
    counted = table.get("costs") is not None
    hist = np.zeros(max_iter + 1, dtype=np.int64)
    successes = flips = calls = calls_ok = 0
    sums = np.zeros((2, len(HQC_STATS_COLUMNS)), dtype=np.int64)  # all trials / the successful ones
    extra = dict(dict(want_stats=True) if want_stats else {}, **_precision_kw(precision))
    try:
        for first in range(0, runs, chunk):
            out = bpd.mc_hqc_run_soft(min(chunk, runs - first), omega, table, seed, first_trial=first, max_iter=max_iter, **extra)
            ok = np.asarray(out["success"]).astype(bool)
            if want_stats:
                st = np.asarray(out["stats"], dtype=np.int64)
                sums += [st.sum(axis=0), st[ok].sum(axis=0)]
            successes += int(ok.sum())
            hist += np.bincount(np.asarray(out["iters"]), minlength=max_iter + 1)[: max_iter + 1]
            flips += int(np.asarray(out["flips"], dtype=np.int64).sum())
            if counted:
                cost = np.asarray(out["cost"], dtype=np.int64)
                calls += int(cost.sum())
                calls_ok += int(cost[ok].sum())
    finally:
        if hasattr(bpd, "close"):
            bpd.close()
    res = dict(runs=int(runs), successes=successes, iter_hist=hist, flips=flips, oracle_calls=None, oracle_calls_mean=None,
               oracle_calls_success=None, oracle_calls_success_mean=None)
    if counted:
        res.update(oracle_calls=calls, oracle_calls_mean=calls / runs if runs else None, oracle_calls_success=calls_ok,
                   oracle_calls_success_mean=calls_ok / successes if successes else None)
    if want_stats:
        res.update(stats={k: int(v) for k, v in zip(HQC_STATS_COLUMNS, sums[0])},
                   stats_success={k: int(v) for k, v in zip(HQC_STATS_COLUMNS, sums[1])})
    return res


def hqc_replay(Hin, N, omega, table, trial_ids, seed, bp_method="product_sum", max_iter=100, bp_decoder=None, precision=None):
    """The post-mortem of a sweep: decode CHOSEN trials of `hqc_oracle_sweep` (the failures of a sweep, the indices on which
    `hqc_precision_audit` finds fp32 and float64 to disagree) again and look at everything, in two calls on one decoder:
      1. `mc_hqc_run_soft_at(trial_ids, ..., want_inputs=True, want_stats=True, want_bits=True)`: the trials as the sweep
         drew and decoded them -- nothing but the listed trials is drawn, decoded or copied;
      2. `decode_batch(msg, channel_probs=probs[outcome], want_llr=True)` on what it exported: the posteriors.
    precision: "float32" or "float64" -- handed to both calls; None: the sweeps' own default (the fp32 kernels; `precision` of a
    `sweeps_in(precision)` class), so that both halves always decode in one arithmetic.
    Returns dict(trial_ids int64 [T], sweep = the first call's dict (success, iters, flips, cost, msg, y, outcome, stats, bits),
    decode = the second's (bits, iters, converged, llr)).  `decode` reproduces `sweep`: the same bits and iteration counts."""
    g = TannerGraph.coerce(Hin)
    if g.n != N:
        raise ValueError(f"Hin has {g.n} columns, N = {N}")
    # the check columns' shared priors are replaced per trial: any probability does
    shared = np.concatenate([np.full(N, omega / N, dtype=np.float64), np.full(g.m, 0.5, dtype=np.float64)])
    bpd = (bp_decoder or _default_bp())(g.with_identity(), max_iter=max_iter, bp_method=bp_method, channel_probs=shared)
    if precision is None:
        precision = getattr(bpd, "sweep_precision", None)
    f64 = precision is not None and str(precision).lower() == "float64"
    try:
        sweep = bpd.mc_hqc_run_soft_at(trial_ids, omega, table, seed, max_iter=max_iter, want_inputs=True, want_stats=True,
                                       want_bits=True, **_precision_kw(precision))
        probs = np.asarray(table["probs"], dtype=np.float64 if f64 else np.float32)[np.asarray(sweep["outcome"])]
        decode = bpd.decode_batch(sweep["msg"], max_iter=max_iter, want_llr=True, channel_probs=probs, **_precision_kw(precision))
    finally:
        if hasattr(bpd, "close"):
            bpd.close()
    return dict(trial_ids=np.asarray(trial_ids, dtype=np.int64), sweep=sweep, decode=decode)


def hqc_attack_curve(first_row_support, N, rows, omega, table, runs, seed, decode_every, max_checks=None, chunk=4096,
                     bp_method="product_sum", max_iter=100, bp_decoder=None):
    """How many checks does a key need?  The reference's attack loop (`add_checks`, simulate/hqc.py:953-984: add rows, decode
    every DECODE_EVERY, stop at the first success) for `runs` keys at once, every decode on the device.

    A trial of `BpDecoder.mc_hqc_run_soft` depends on (seed, global trial index) alone: its secret does not depend on the
    number of rows, and check r always takes the same random word.  So the trials of a graph of R rows are the first R answers
    of the SAME trials on that graph with more rows appended, and re-running one sweep with one seed on a growing decoder
    follows `runs` keys through the loop.  ONE live decoder is kept: it starts on the first `decode_every` rows of
    circulant(first_row_support)[rows] (sparse, each row with its identity column, as `HqcCheckAccumulator` builds them), grows
    by `decode_every` rows per step (`append_rows`) up to `max_checks` (default: all of `rows`; a last partial step is not
    taken), and at every step decodes trials 0 .. runs - 1, `chunk` at a time, with the per-trial counters of
    tracking.add_decoder_stats counted on the device (`want_stats`).  Trials that already succeeded are decoded again at
    the later steps -- this function decodes contiguous ranges of trial indices -- and converge within a few iterations; their
    later results are not recorded (`hqc_attack_curve_retiring` stops decoding a key at its first success, as the reference's
    loop does).  The result does not depend on `chunk`.
    The curve in the reference's own arithmetic: `bp_decoder=sweeps_in("float64")` -- a decoder class whose sweeps decode in
    float64 (the float64 form works on a decoder grown by `append_rows`); this function's own parameters are what they were.

    Returns dict(
      steps                int32 [S]: the numbers of checks R decoded at,
      successes            int64 [S]: trials whose decode at that step succeeded (already-recovered keys included),
      checks_needed        int32 [runs]: R at the trial's FIRST success, -1 if it never succeeded,
      oracle_calls_needed  int64 [runs]: the oracle calls the trial had spent at that step (its `cost`), -1 where
                           checks_needed is; None when the table has no costs,
      decoder_stats        one row per (trial, step) up to and including the trial's first success -- the reference's attack
                           stops there (hqc.py:980-982) -- ordered by trial, then step: dicts with the keys
                           `write_decoder_stats_csv` takes (checks, oracle_calls (None without costs), HQC_STATS_COLUMNS,
                           success) and `trial`)."""
    return _hqc_attack_curve(first_row_support, N, rows, omega, table, runs, seed, decode_every, max_checks, chunk, bp_method, max_iter,
                             bp_decoder, retiring=False)


def hqc_attack_curve_retiring(first_row_support, N, rows, omega, table, runs, seed, decode_every, max_checks=None, chunk=4096,
                              bp_method="product_sum", max_iter=100, bp_decoder=None):
    """`hqc_attack_curve` with the reference's stopping rule (hqc.py:980-982): a key is decoded until its FIRST success and
    never again.  The loop, the decoder and the trials are `hqc_attack_curve`'s; at every step only the trial indices not yet
    recovered are decoded, `chunk` at a time, through `BpDecoder.mc_hqc_run_soft_at` (a sweep on a list of trial indices).
    Works with `bp_decoder=sweeps_in("float64")` as that function does.  The result does not depend on `chunk`.

    Returns `hqc_attack_curve`'s dict: `steps`, `checks_needed`, `oracle_calls_needed` and `decoder_stats` are equal to that
    function's (it records nothing about a key after its first success either), and
      successes            int64 [S]: the keys whose FIRST success is that step (not: every key that succeeds there),
      decoded              int64 [S]: the trials decoded at that step = the keys not recovered before it."""
    return _hqc_attack_curve(first_row_support, N, rows, omega, table, runs, seed, decode_every, max_checks, chunk, bp_method, max_iter,
                             bp_decoder, retiring=True)


def _hqc_attack_curve(first_row_support, N, rows, omega, table, runs, seed, decode_every, max_checks, chunk, bp_method, max_iter,
                      bp_decoder, retiring):
    # the loop of hqc_attack_curve (every step decodes trials 0 .. runs - 1 in contiguous chunks) and of
    # hqc_attack_curve_retiring (every step decodes the list of trials with no success yet)
    k = np.sort(np.asarray(first_row_support, dtype=np.int64))
    rows = np.asarray(rows, dtype=np.int64)
    step = int(decode_every)
    top = rows.size if max_checks is None else min(int(max_checks), rows.size)
    if step < 1 or runs < 0 or chunk < 1:
        raise ValueError("decode_every and chunk must be positive and runs must not be negative")
    if top < step:
        raise ValueError(f"{top} rows do not make one step of decode_every = {step}")
    W = k.size
    # row i: the sorted support of row rows[i] of the circulant, then its identity column N + i -- CSR as it stands
    cols = np.concatenate([np.sort((rows[:top, None] - k[None, :]) % N, axis=1), N + np.arange(top)[:, None]], axis=1).astype(np.int32)
    ptr = np.arange(step + 1, dtype=np.int32) * (W + 1)
    steps = np.arange(step, top + 1, step, dtype=np.int32)
    counted = table.get("costs") is not None
    successes = np.zeros(steps.size, dtype=np.int64)
    decoded = np.zeros(steps.size, dtype=np.int64)
    needed = np.full(runs, -1, dtype=np.int32)
    calls = np.full(runs, -1, dtype=np.int64) if counted else None
    per_trial = [[] for _ in range(runs)]
    # the check columns' shared priors are replaced per trial: any probability does
    shared = np.concatenate([np.full(N, omega / N, dtype=np.float64), np.full(step, 0.5, dtype=np.float64)])
    with np.errstate(divide="ignore"):
        bpd = (bp_decoder or _default_bp())(TannerGraph.from_csr(step, N + step, ptr, cols[:step].reshape(-1)), max_iter=max_iter,
                                            bp_method=bp_method, channel_probs=shared)
    try:
        for s, R in enumerate(steps):
            R = int(R)
            if s:
                bpd.append_rows(ptr, cols[R - step : R].reshape(-1), N + R, np.full(step, 0.5, dtype=np.float64))
            live = np.flatnonzero(needed < 0) if retiring else np.arange(runs, dtype=np.int64)
            decoded[s] = live.size
            for first in range(0, live.size, chunk):
                ids = live[first : first + chunk]
                if retiring:
                    out = bpd.mc_hqc_run_soft_at(ids, omega, table, seed, max_iter=max_iter, want_stats=True)
                else:
                    out = bpd.mc_hqc_run_soft(ids.size, omega, table, seed, first_trial=first, max_iter=max_iter, want_stats=True)
                ok = np.asarray(out["success"]).astype(bool)
                st = np.asarray(out["stats"])
                cost = np.asarray(out["cost"], dtype=np.int64) if counted else None
                successes[s] += int(ok.sum())
                for i in np.flatnonzero(needed[ids] < 0):
                    t = int(ids[i])
                    row = {"trial": t, "checks": R, "oracle_calls": int(cost[i]) if counted else None}
                    row.update(zip(HQC_STATS_COLUMNS, (int(v) for v in st[i])))
                    row["success"] = bool(ok[i])
                    per_trial[t].append(row)
                    if ok[i]:
                        needed[t] = R
                        if counted:
                            calls[t] = cost[i]
    finally:
        if hasattr(bpd, "close"):
            bpd.close()
    res = dict(steps=steps, successes=successes, checks_needed=needed, oracle_calls_needed=calls,
               decoder_stats=[row for rows_of in per_trial for row in rows_of])
    return dict(res, decoded=decoded) if retiring else res


def _precision_kw(precision):
    # (only where asked for: a stand-in decoder class need not know the keyword)
    return {} if precision is None else {"precision": precision}


def sweeps_in(precision, bp_decoder=None):
    """A decoder class whose Monte-Carlo sweeps (`mc_fer_run`, `mc_hqc_run`, `mc_hqc_run_soft` and their `_at` forms on chosen
    trials) decode in `precision` unless a
    call says otherwise: `bp_decoder` (default: the HIP class) with that one default changed, for the drivers that take a
    decoder class and no `precision` of their own -- `hqc_attack_curve(..., bp_decoder=sweeps_in("float64"))` is the
    checks-needed curve in the reference's float64 arithmetic.  `decode` / `decode_batch` are untouched.  "float64" on a min-sum
    decoder raises the `ValueError` of the methods themselves, at the first sweep."""
    if str(precision).lower() not in ("float32", "float64"):
        raise ValueError(f"precision '{precision}' is invalid. Choose 'float32' or 'float64'.")
    base = bp_decoder or _default_bp()

    class Sweeps(base):
        sweep_precision = str(precision).lower()  # (what a driver that also calls `decode_batch` on a sweep's exports reads: hqc_replay)

        def mc_fer_run(self, *args, **kw):
            return super().mc_fer_run(*args, **dict({"precision": precision}, **kw))

        def mc_hqc_run(self, *args, **kw):
            return super().mc_hqc_run(*args, **dict({"precision": precision}, **kw))

        def mc_hqc_run_soft(self, *args, **kw):
            return super().mc_hqc_run_soft(*args, **dict({"precision": precision}, **kw))

        def mc_fer_run_at(self, *args, **kw):
            return super().mc_fer_run_at(*args, **dict({"precision": precision}, **kw))

        def mc_hqc_run_at(self, *args, **kw):
            return super().mc_hqc_run_at(*args, **dict({"precision": precision}, **kw))

        def mc_hqc_run_soft_at(self, *args, **kw):
            return super().mc_hqc_run_soft_at(*args, **dict({"precision": precision}, **kw))

    Sweeps.__name__ = Sweeps.__qualname__ = f"{base.__name__}Sweeps{str(precision).capitalize()}"
    return Sweeps


def hqc_precision_audit(Hin, N, omega, table, runs, seed, chunk=4096, max_iter=100, bp_decoder=None):
    """On how many trials do the fp32 tanh kernels and the reference's float64 arithmetic decide differently?  The sweep of
    `hqc_oracle_sweep` (product-sum), every chunk of trial indices run twice on ONE decoder: `mc_hqc_run_soft` with
    precision="float32" and with precision="float64".  The trials are the same whatever the precision -- inputs, outcomes and
    certainties bit for bit (the float64 decode takes the table's certainties unrounded) -- so every difference is the decode's.
    Global trial indices 0 .. runs - 1 are scanned `chunk` at a time; the result does not depend on `chunk`.  Returns dict(
      runs, successes32, successes64,
      success_differs         int64 array: the trial indices whose success differs, ascending,
      iters_differ            the number of trials whose iteration count differs,
      iter_hist32, iter_hist64  int64 [max_iter + 1]: trials by the iteration count of their decode)."""
    g = TannerGraph.coerce(Hin)
    if g.n != N:
        raise ValueError(f"Hin has {g.n} columns, N = {N}")
    if runs < 0 or chunk < 1:
        raise ValueError("runs must not be negative and chunk must be positive")
    # the check columns' shared priors are replaced per trial: any probability does
    shared = np.concatenate([np.full(N, omega / N, dtype=np.float64), np.full(g.m, 0.5, dtype=np.float64)])
    bpd = (bp_decoder or _default_bp())(g.with_identity(), max_iter=max_iter, bp_method="product_sum", channel_probs=shared)
    hist = np.zeros((2, max_iter + 1), dtype=np.int64)
    successes = [0, 0]
    differs = []
    iters_differ = 0
    try:
        for first in range(0, runs, chunk):
            ok, its = [], []
            for k, precision in enumerate(("float32", "float64")):
                out = bpd.mc_hqc_run_soft(min(chunk, runs - first), omega, table, seed, first_trial=first, max_iter=max_iter,
                                          precision=precision)
                ok.append(np.asarray(out["success"]).astype(bool))
                its.append(np.asarray(out["iters"]))
                successes[k] += int(ok[k].sum())
                hist[k] += np.bincount(its[k], minlength=max_iter + 1)[: max_iter + 1]
            differs.append(first + np.flatnonzero(ok[0] != ok[1]))
            iters_differ += int((its[0] != its[1]).sum())
    finally:
        if hasattr(bpd, "close"):
            bpd.close()
    return dict(runs=int(runs), successes32=successes[0], successes64=successes[1],
                success_differs=np.concatenate(differs).astype(np.int64) if differs else np.zeros(0, dtype=np.int64),
                iters_differ=iters_differ, iter_hist32=hist[0], iter_hist64=hist[1])


def hqc_decode(N, Hin, checks, y_sparse, bp_decoder=None, max_iter=100, precision=None):
    """simulate/hqc.py:661-759.  Hin: TannerGraph (R x N, one row per oracle answer) or a
    dense array; checks: [(value, certainty)]; returns (success, stats) with the seven
    fields `tracking.add_decoder_stats` records (hqc.py:750-758).
    precision: None (the decoder's default), "float32" or "float64" (the reference's own float64 recursion), handed to the
    decoder's constructor."""
    g = TannerGraph.coerce(Hin)
    R = g.m
    H = g.with_identity()
    prob_for_one = len(y_sparse) / N
    channel_probs = np.concatenate(
        [np.full(N, prob_for_one, dtype=np.float64), np.array([1 - p for (_, p) in checks], dtype=np.float64)]
    )
    with np.errstate(divide="ignore"):
        bpd = (bp_decoder or _default_bp())(H, max_iter=max_iter, bp_method="product_sum", channel_probs=channel_probs,
                                            **_precision_kw(precision))
    cvals = np.array([int(c) for (c, _) in checks], dtype=np.uint8)
    msg = np.concatenate([np.zeros(N, dtype=np.uint8), cvals])
    decoded = bpd.decode_batch(msg[None, :], early_exit=True, input_vector_type="received_vector")["bits"][0]
    return hqc_stats(N, decoded, cvals, y_sparse)


def hqc_decode_batch(N, Hin, checks_per_trial, y_sparse_per_trial, bp_decoder=None, max_iter=100, precision=None):
    """The batched twin of `hqc_decode`: many trials over the SAME Hin, each with its own answers and its own
    certainties (the oracles of hqc.py:782-806 raise a check's certainty with every repeated measurement, so two trials
    differ on their R check columns).  ONE decoder, ONE call: the per-trial `1 - certainty` rows go in as per-codeword
    priors of the last R columns (`decode_batch(..., channel_probs=)`), the first N columns share `len(y) / N`.
    Trials whose secrets differ in weight cannot share that prior: all n columns then go in per codeword.

      checks_per_trial    one [(value, certainty)] list of length R per trial
      y_sparse_per_trial  the secrets' supports
      precision           None (the decoder's default), "float32" or "float64": handed to the decoder's constructor; a float64
                          decoder takes the per-trial priors as float64
    Returns [(success, stats)]: per trial what `hqc_decode` returns for it."""
    g = TannerGraph.coerce(Hin)
    R = g.m
    H = g.with_identity()
    batch = len(checks_per_trial)
    if batch == 0 or len(y_sparse_per_trial) != batch:
        raise ValueError("hqc_decode_batch expects one list of checks and one secret per trial")
    if any(len(c) != R for c in checks_per_trial):
        raise ValueError(f"every trial needs one (value, certainty) pair per row of Hin ({R})")
    cvals = np.array([[int(c) for (c, _) in checks] for checks in checks_per_trial], dtype=np.uint8).reshape(batch, R)
    check_part = np.array([[1 - p for (_, p) in checks] for checks in checks_per_trial], dtype=np.float64).reshape(batch, R)
    weights = [len(y) for y in y_sparse_per_trial]
    shared = np.concatenate([np.full(N, weights[0] / N, dtype=np.float64), check_part[0]])
    with np.errstate(divide="ignore"):
        bpd = (bp_decoder or _default_bp())(H, max_iter=max_iter, bp_method="product_sum", channel_probs=shared,
                                            **_precision_kw(precision))
    if len(set(weights)) == 1:
        soft = check_part
    else:
        soft = np.concatenate([np.repeat(np.array(weights, dtype=np.float64)[:, None] / N, N, axis=1), check_part], axis=1)
    msg = np.concatenate([np.zeros((batch, N), dtype=np.uint8), cvals], axis=1)
    try:
        decoded = bpd.decode_batch(msg, early_exit=True, input_vector_type="received_vector",
                                   channel_probs=soft if getattr(bpd, "precision", "float32") == "float64"
                                   else soft.astype(np.float32))["bits"]
    finally:
        if hasattr(bpd, "close"):
            bpd.close()
    return [hqc_stats(N, decoded[i], cvals[i], y_sparse_per_trial[i]) for i in range(batch)]


def hqc_stats(N, decoded, cvals, y_sparse):
    """The counters of hqc.py:709-758 from one decoded vector."""
    truth = np.zeros(N, dtype=bool)
    truth[np.asarray(list(y_sparse), dtype=np.int64)] = True
    dy = decoded[:N].astype(bool)
    dc = decoded[N:].astype(bool)
    cv = cvals.astype(bool)
    stats = {
        "checks": int(cvals.size),
        "unsatisfied": int(cv.sum()),
        "good_flips": int((dy & truth).sum()),
        "bad_flips": int((dy & ~truth).sum()),
        "found_bad_satisfied_checks": int((~cv & dc).sum()),
        "found_bad_unsatisfied_checks": int((cv & ~dc).sum()),
    }
    success = bool((dy == truth).all())
    stats["success"] = success
    return success, stats


# -- the four FER commands of main.py (as functions; the CLI itself is out of scope) ------
def regular_ldpc_code(seed, runs, error_rate=None, error_file=None, bp_decoder=None):
    """main.py:189-208 (BASELINE config 1 with error_file = binary_distr.txt)."""
    rng = codes.make_random_state(seed)
    ep = ErrorsProvider(error_rate, error_file, rng)
    H = codes.make_regular_ldpc_graph(300, 150, 3, 6, rng)
    return simulate_frame_error_rate(H, ep, runs, rng, bp_decoder)


def regular_ldpc_code_identity(seed, runs, error_rate=None, error_file=None, bp_decoder=None):
    """main.py:210-231."""
    rng = codes.make_random_state(seed)
    ep = ErrorsProvider(error_rate, error_file, rng)
    H = codes.make_regular_ldpc_identity_graph(300, 150, 3, 6, rng)
    return simulate_frame_error_rate(H, ep, runs, rng, bp_decoder)


def qc_ldpc_code(seed, runs, error_rate=None, error_file=None, bp_decoder=None):
    """main.py:233-250."""
    rng = codes.make_random_state(seed)
    ep = ErrorsProvider(error_rate, error_file, rng)
    H = codes.make_qc_parity_check_graph(500, 3, 2, rng)
    return simulate_frame_error_rate(H, ep, runs, rng, bp_decoder)


def official_example(seed, runs, error_rate=None, error_file=None, bp_decoder=None):
    """main.py:265-276."""
    rng = codes.make_random_state(seed)
    ep = ErrorsProvider(error_rate, error_file, rng)
    return simulate_frame_error_rate(codes.rep_code_graph(13), ep, runs, rng, bp_decoder)


# -- the attack loop's side of the decode path -------------------------
class HqcCheckAccumulator:
    """The check-accumulation half of the reference's attack loop, sparse and incremental.

    The reference keeps `H` dense and grows it with `np.vstack([H, Hgen[bit_n]])` per oracle
    answer (simulate/hqc.py:885-908), then rebuilds `[H | I]` and a fresh decoder from the dense
    matrix on every decode (hqc.py:680,694; every DECODE_EVERY answers, hqc.py:972-980) -- O(R(N+R))
    per decode.  Here a check is W+1 appended CSR entries (row `bit_n` of circulant(first_row),
    then its identity column), and a decode hands the CSR arrays to the library as they stand:
    O(E) per decode, nothing dense, the same result as `hqc_decode`.
    """

    def __init__(self, N, first_row_support, weight_of_y, bp_decoder=None, max_iter=100, decode_every=0):
        self.N = int(N)
        self.k = np.sort(np.asarray(first_row_support, dtype=np.int64))
        self.omega = int(weight_of_y)
        self.bp_decoder = bp_decoder
        self.max_iter = max_iter
        self.decode_every = int(decode_every)
        self._cols = np.empty((64, self.k.size + 1), dtype=np.int32)  # row i: sorted support of Hin row i, then N + i
        self._vals = np.empty(64, dtype=np.uint8)  # measured check values
        self._cert = np.empty(64, dtype=np.float64)  # their certainties
        self._R = 0
        self.decoder_stats = []
        self.num_oracle_calls = 0
        self._previous_decoding = 0
        self._bpd = None  # the decoder kept alive between decodes (rows are appended to it)
        self._bpd_R = 0  # checks it already holds
        self._bpd_omega = None

    def __len__(self):
        return self._R

    @property
    def checks(self):
        """[(value, certainty)], the list simulate/hqc.py keeps (hqc.py:907)."""
        return [(int(v), float(c)) for v, c in zip(self._vals[: self._R], self._cert[: self._R])]

    def add_check(self, bit_n, check, certainty):
        """hqc.py:885-908: append row `bit_n` of Hgen with its measured value."""
        if self._R == self._cols.shape[0]:  # amortised doubling
            self._cols = np.concatenate([self._cols, np.empty_like(self._cols)])
            self._vals = np.concatenate([self._vals, np.empty_like(self._vals)])
            self._cert = np.concatenate([self._cert, np.empty_like(self._cert)])
        row = self._cols[self._R]
        row[:-1] = np.sort((int(bit_n) - self.k) % self.N)
        row[-1] = self.N + self._R
        self._vals[self._R] = int(bool(check))
        self._cert[self._R] = float(certainty)
        self._R += 1

    def graph(self):
        """H = [Hin | I_R] as a TannerGraph, built from the appended rows (never dense)."""
        R, W = self._R, self.k.size
        # each row: its W sorted circulant positions (< N), then its identity column N + i -- CSR as it stands
        return TannerGraph.from_csr(R, self.N + R, np.arange(R + 1, dtype=np.int64) * (W + 1), self._cols[:R].reshape(-1))

    def _decoder(self, omega):
        """The decoder for the checks accumulated so far.  The reference builds a new one from the dense
        matrix on every decode (hqc.py:680,694); here ONE decoder lives through the attack and the checks
        added since the last decode are APPENDED to it (`append_rows`: CSR tail, their identity columns and
        priors) -- same results as a fresh decoder, without re-validating, re-sorting and re-uploading the
        rows it already holds.  Decoder classes without `append_rows` (test doubles) are rebuilt."""
        R, W = self._R, self.k.size
        cls = self.bp_decoder or _default_bp()
        if self._bpd is not None and (not hasattr(self._bpd, "append_rows") or self._bpd_omega != omega or R < self._bpd_R):
            self.close()
        if self._bpd is None:
            probs = np.concatenate([np.full(self.N, omega / self.N), 1 - self._cert[:R]])
            with np.errstate(divide="ignore"):
                self._bpd = cls(self.graph(), max_iter=self.max_iter, bp_method="product_sum", channel_probs=probs)
            self._bpd_omega = omega
        elif R > self._bpd_R:
            k = R - self._bpd_R
            try:
                with np.errstate(divide="ignore"):
                    self._bpd.append_rows(np.arange(k + 1, dtype=np.int32) * (W + 1), self._cols[self._bpd_R : R].reshape(-1),
                                          self.N + R, 1 - self._cert[self._bpd_R : R])
            except Exception:
                # a failed append (a certainty outside [0, 1], no memory) must not wedge the accumulator: drop the live
                # decoder, so that the next decode builds a fresh one -- the reference's behaviour on every decode
                self.close()
                raise
        self._bpd_R = R
        return self._bpd

    def close(self):
        """Release the live decoder (device memory, stream).  The accumulator stays usable: the next decode builds a
        new decoder from all the checks.  Call it -- or use the accumulator as a context manager -- when the attack is
        over; rows are APPEND-ONLY (`add_check`), which is what lets the live decoder be extended instead of rebuilt."""
        if self._bpd is not None and hasattr(self._bpd, "close"):
            self._bpd.close()
        self._bpd = None
        self._bpd_R = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode(self, y_sparse):
        """hqc.py:661-759 on the accumulated checks; appends the stats row (hqc.py:750-758)."""
        R = self._R
        bpd = self._decoder(len(y_sparse))
        cvals = self._vals[:R].copy()
        msg = np.concatenate([np.zeros(self.N, dtype=np.uint8), cvals])
        decoded = bpd.decode_batch(msg[None, :], early_exit=True, input_vector_type="received_vector")["bits"][0]
        success, stats = hqc_stats(self.N, decoded, cvals, y_sparse)
        row = {"checks": R, "oracle_calls": self.num_oracle_calls}
        row.update({k: v for k, v in stats.items() if k != "checks"})
        self.decoder_stats.append(row)
        return success

    def add_checks(self, bits, check_value, y_sparse):
        """hqc.py:953-984: add (bit_n, certainty) pairs, decoding every `decode_every` checks.
        Returns True as soon as a decode succeeds, else False."""
        for bit_n, certainty in bits:
            self.add_check(bit_n, check_value, certainty)
            R = self._R
            if self.decode_every and R % self.decode_every == 0 and self._previous_decoding != R:
                self._previous_decoding = R
                if self.decode(y_sparse):
                    self.close()  # the attack is over (hqc.py:976-980 returns here): give the GPU decoder back
                    return True
        return False


STATS_COLUMNS = ["label", "alg", "weight", "epsilon0", "epsilon1", "checks", "oracle_calls", "unsatisfied", "good_flips",
                 "bad_flips", "found_bad_satisfied_checks", "found_bad_unsatisfied_checks", "success"]  # fmt: skip
# the per-trial counters of `BpDecoder.mc_hqc_run_soft(want_stats=True)`, in the order of its `stats` columns (bp.HQC_STATS_COLUMNS)
HQC_STATS_COLUMNS = tuple(STATS_COLUMNS[7:12])


def write_decoder_stats_csv(path, decoder_stats, label, alg, weight, epsilon):
    """The CSV `main.py hqc_simulate --csv-output` produces (main.py:146-156 from
    hqc.py:245-264): static columns label/alg/weight/epsilon0/epsilon1, then the stats
    fields; header only when the file is new, rows appended otherwise -- the format
    `visualize.load_data` reads (visualize.py:102-119)."""
    import csv
    import os

    new = not os.path.exists(path)
    with open(path, "a" if not new else "w", newline="") as f:
        w = csv.writer(f)
        if new:
            w.writerow(STATS_COLUMNS)
        for row in decoder_stats:
            w.writerow([label, alg, weight, epsilon[0], epsilon[1]] + [row[c] for c in STATS_COLUMNS[5:]])


def kyber_channel_probabilities(s_distr, ssum_distr, sum_weight, check_blocks, eta=2, block_len=256, num_blocks=3):
    """Input layout of the Kyber decoders (simulate/kyber.py:362-376): secret-coefficient
    pmfs [num_blocks*block_len, 2*eta+1] and row-sum pmfs [block_len*check_blocks,
    2*sum_weight*eta+1], the latter REVERSED so that every row of H sums to 0."""
    assert len(s_distr) == num_blocks and len(s_distr[0]) == block_len
    ssum_len = block_len * check_blocks
    assert len(ssum_distr) == ssum_len
    B = sum_weight * eta
    channel_output = np.zeros((block_len * num_blocks, 2 * eta + 1), dtype=np.float32)
    channel_output_sum = np.zeros((ssum_len, 2 * B + 1), dtype=np.float32)
    for j in range(num_blocks):
        for i in range(block_len):
            channel_output[i + j * block_len] = s_distr[j][i]
    for i in range(ssum_len):
        channel_output_sum[i] = np.asarray(ssum_distr[i])[::-1]
    return channel_output, channel_output_sum
