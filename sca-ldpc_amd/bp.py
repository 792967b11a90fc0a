"""`ldpc.bp_decoder`-shaped front end of the HIP binary BP decoder.

Mirrors the constructor/`decode()` surface the reference uses
(simulate/decode.py:155-161,171; simulate/hqc.py:694-699,708): same argument
names and meaning, same error behaviour (ValueError on a bad method, a bad
`channel_probs` length or a wrong-length input), same read-only result
attributes (`bp_decoding`, `log_prob_ratios`, `converge`, `iter`).  On top of
that: `decode_batch`, which decodes many independent inputs per call -- the
Monte-Carlo drivers' trials are independent (decode.py:165), so the batch
dimension is what feeds the GPU.

Differences from the reference package, all deliberate:
  * messages are fp32 (the package computes in float64);
  * "product_sum" runs the tanh rule in the LLR domain (the package's ratio-domain
    recursion is the same function of the messages);
    `precision="float64"` (or SCALDPC_PRECISION=float64 in the environment) asks for the
    package's own arithmetic instead -- the ratio-domain recursion in float64, operation for
    operation (scaldpc_bp_decode_batch_f64): its decisions, iteration counts and converged
    flags exactly, at a fraction of the fp32 path's throughput;
  * H may be a dense array (as the reference passes), a scipy sparse matrix or a
    `TannerGraph`; it is never densified.
There is no CPU fallback: constructing a decoder without libscaldpc.so raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from .graph import TannerGraph

_PS = {"prod_sum", "product_sum", "ps", "0", "prod sum", "prod_sum_log", "product_sum_log", "ps_log", "2", "psl"}
_MS = {"min_sum", "minimum_sum", "ms", "1", "minimum sum", "min sum", "min_sum_log", "minimum_sum_log", "ms_log", "3",
       "minimum sum_log", "msl"}  # fmt: skip


def _method_id(bp_method):
    key = str(bp_method).lower()
    if key in _PS:
        return _lib.BP_PRODUCT_SUM
    if key in _MS:
        return _lib.BP_MIN_SUM
    raise ValueError(
        f"BP method '{bp_method}' is invalid. Please choose from the following methods: "
        "'product_sum', 'minimum_sum', 'product_sum_log' or 'minimum_sum_log'"
    )


def _vector_type(t):
    if t in (-1, "auto", None):
        return -1
    if t in (0, "syndrome"):
        return _lib.IN_SYNDROME
    if t in (1, "received_vector", "received"):
        return _lib.IN_RECEIVED
    raise ValueError(f"input_vector_type '{t}' is invalid. Choose 'syndrome', 'received_vector' or 'auto'.")


_PRECISIONS = ("float32", "float64")


def _precision(value, method, source="precision"):
    """"float32" / "float64" from the keyword (or the environment's default); float64 exists for the product-sum rule only."""
    key = str(value).lower()
    if key not in _PRECISIONS:
        raise ValueError(f"{source} '{value}' is invalid. Choose 'float32' or 'float64'.")
    if key == "float64" and method != _lib.BP_PRODUCT_SUM:
        raise ValueError(f"{source}='float64' is the reference's ratio-domain product-sum recursion: it has no min-sum form")
    return key


# the five per-trial counters of scaldpc_mc_hqc_run_stats, in the order of its out_stats (= driver.STATS_COLUMNS[7:12])
HQC_STATS_COLUMNS = ("unsatisfied", "good_flips", "bad_flips", "found_bad_satisfied_checks", "found_bad_unsatisfied_checks")


class BpDecoder:
    def __init__(
        self,
        parity_check_matrix,
        error_rate=None,
        max_iter=0,
        bp_method=0,
        ms_scaling_factor=1.0,
        channel_probs=[None],
        input_vector_type=-1,
        precision=None,
    ):
        """precision: "float32" (the fp32 kernels) or "float64" (the reference package's own ratio-domain float64 recursion,
        product-sum only); None reads SCALDPC_PRECISION once, here, and defaults to "float32".  `decode()` follows it;
        `decode_batch` / `decode_batch_device` take a `precision` of their own that overrides it per call."""
        self._h = None
        # (before any library call: a float64 min-sum decoder is refused with nothing built)
        if precision is None:
            env = os.environ.get("SCALDPC_PRECISION")
            self.precision = _precision(env, _method_id(bp_method), "SCALDPC_PRECISION") if env else "float32"
        else:
            self.precision = _precision(precision, _method_id(bp_method))
        self._lib = _lib.load()  # raises when the HIP extension is missing
        g = TannerGraph.coerce(parity_check_matrix)
        self.graph = g
        self.m, self.n = g.m, g.n
        self.max_iter = int(max_iter) if int(max_iter) != 0 else self.n
        if self.max_iter < 0:
            raise ValueError("max_iter must be non-negative")
        self._method = _method_id(bp_method)
        self.bp_method = "product_sum" if self._method == _lib.BP_PRODUCT_SUM else "minimum_sum"
        self.ms_scaling_factor = float(ms_scaling_factor)
        self._vector_type = _vector_type(input_vector_type)
        h = C.c_void_p()
        _lib.check(
            self._lib.scaldpc_bp_create(g.m, g.n, g.nnz, _lib.ptr(g.row_ptr), _lib.ptr(g.col_idx), C.byref(h))
        )
        self._h = h
        # priors, as the package resolves them: channel_probs wins over error_rate
        # (no list() round trip: a 20 000-entry ndarray per decoder is the attack loop's normal case)
        have_cp = channel_probs is not None and len(channel_probs) > 0 and channel_probs[0] is not None
        if have_cp:
            if len(channel_probs) != self.n:
                raise ValueError(
                    f"The length of the channel probability vector must be eqaul to the block length n={self.n}."
                )
            probs = np.asarray(channel_probs, dtype=np.float64)
        elif error_rate is not None:
            probs = np.full(self.n, float(error_rate), dtype=np.float64)
        else:
            raise ValueError(
                "Please specify the error channel. Either: 1) error_rate: float or 2) channel_probs: list of floats "
                "indicating the error probability on each bit. "
            )
        self.update_channel_probs(probs)
        self.error_rate = error_rate
        # result attributes of the last decode()
        self.bp_decoding = np.zeros(self.n, dtype=int)
        self.log_prob_ratios = np.zeros(self.n, dtype=np.float64)
        self.converge = 0
        self.iter = 0

    # -- ldpc-compatible API --------------------------------------------------
    def update_channel_probs(self, channel):
        probs = np.ascontiguousarray(channel, dtype=np.float64)
        if probs.shape != (self.n,):
            raise ValueError(
                f"The length of the channel probability vector must be eqaul to the block length n={self.n}."
            )
        _lib.check(self._lib.scaldpc_bp_set_channel_probs(self._h, _lib.ptr(probs)))
        self._probs = probs
        self._probs_tails = []

    @property
    def channel_probs(self):
        if self._probs_tails:
            self._probs = np.concatenate([self._probs] + self._probs_tails)
            self._probs_tails = []
        return self._probs

    def append_rows(self, row_ptr, col_idx, new_n, channel_probs_tail):
        """The graph GROWS (the attack loop's `H = np.vstack([H, row])`, simulate/hqc.py:885-908, where the
        reference builds a new decoder per decode): append checks to this live decoder.

          row_ptr, col_idx    CSR of the NEW rows only (row_ptr[0] = 0; columns strictly ascending, < new_n)
          new_n               block length afterwards (>= n: new columns come last -- for H = [Hin | I] every
                              appended row brings its identity column)
          channel_probs_tail  priors of the new columns [n, new_n)

        Results of later decodes are those of a decoder freshly built on the grown graph, bit for bit."""
        rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(col_idx, dtype=np.int32)
        tail = np.ascontiguousarray(channel_probs_tail, dtype=np.float64)
        new_n = int(new_n)
        if rp.ndim != 1 or rp.size < 1 or ci.ndim != 1 or ci.size != int(rp[-1]):
            raise ValueError("append_rows expects CSR arrays of the new rows (row_ptr[0] = 0, len(col_idx) = row_ptr[-1])")
        if tail.shape != (new_n - self.n,):
            raise ValueError(f"channel_probs_tail must hold the priors of the {new_n - self.n} new columns")
        # validated BEFORE the graph grows: a bad prior must not leave a grown decoder with unset priors behind
        if tail.size and not bool(((tail >= 0.0) & (tail <= 1.0)).all()):
            bad = int(np.flatnonzero(~((tail >= 0.0) & (tail <= 1.0)))[0])
            raise ValueError(f"channel_probs[{self.n + bad}] = {tail[bad]} is not a probability")
        old_n = self.n
        _lib.check(self._lib.scaldpc_bp_append_rows(self._h, rp.size - 1, _lib.ptr(rp), _lib.ptr(ci), new_n))
        self.m += rp.size - 1
        self.n = new_n
        self.graph = None  # (the constructor's graph no longer describes this decoder)
        _lib.check(self._lib.scaldpc_bp_set_channel_probs_tail(self._h, old_n, new_n - old_n, _lib.ptr(tail)))
        self._probs_tails.append(tail)  # (`channel_probs` is put together when somebody asks: appends are on the attack loop's critical path)

    def _resolve_kind(self, length, input_vector_type=None):
        kind = self._vector_type if input_vector_type is None else _vector_type(input_vector_type)
        if kind == -1:
            if self.m == self.n:
                raise ValueError(
                    "parity check matrix is square: the input vector type is ambiguous, please set "
                    "input_vector_type to 'syndrome' or 'received_vector'"
                )
            if length == self.m:
                kind = _lib.IN_SYNDROME
            elif length == self.n:
                kind = _lib.IN_RECEIVED
        want = self.m if kind == _lib.IN_SYNDROME else self.n if kind == _lib.IN_RECEIVED else None
        if want is None or length != want:
            raise ValueError(
                f"The input to the ldpc.bp_decoder.decode must be either a received word (of length={self.n}) or a "
                f"syndrome (of length={self.m}). The inputted vector has length={length}. Valid formats are "
                "`np.ndarray` or `scipy.sparse.spmatrix`."
            )
        return kind

    def decode(self, input_vector):
        """One decode, reference semantics (early exit at H e == s).  Returns int array [n]."""
        if hasattr(input_vector, "toarray"):  # scipy.sparse vector, which the package accepts too
            input_vector = input_vector.toarray()
        v = np.asarray(input_vector)
        if v.ndim != 1:
            v = v.reshape(-1)
        r = self.decode_batch(v[None, :], want_llr=True)
        self.bp_decoding = r["bits"][0].astype(int)
        self.log_prob_ratios = r["llr"][0].astype(np.float64)  # (precision "float64": the reference's values as they are)
        self.converge = int(r["converged"][0])
        self.iter = int(r["iters"][0])
        return self.bp_decoding

    # -- batched API ------------------------------------------------------------
    def decode_batch(self, inputs, max_iter=None, early_exit=True, want_llr=False, input_vector_type=None,
                     channel_probs=None, precision=None):
        """inputs: [batch, m] syndromes or [batch, n] received words (any integer dtype).
        channel_probs: None (the decoder's priors for every codeword), or a 2-D array [batch, k] of prior error
        probabilities PER CODEWORD for the last k columns (1 <= k <= n; the columns below keep the decoder's priors):
        hqc.decode()'s `1 - certainty` of every check with k = R on H = [Hin | I_R] (simulate/hqc.py:684-699).  Values are
        taken as float32.  The decoder's own priors are left as they are.
        precision: None (the decoder's), "float32" or "float64".  With "float64" the call runs the reference's ratio-domain
        float64 recursion (scaldpc_bp_decode_batch_f64): `llr` is float64 and `channel_probs` is taken as float64.
        Returns dict(bits uint8 [batch, n], llr float32 [batch, n] or None,
        iters int32 [batch], converged uint8 [batch])."""
        f64 = (self.precision if precision is None else _precision(precision, self._method)) == "float64"
        x = np.asarray(inputs)
        if x.ndim != 2:
            raise ValueError("decode_batch expects a 2-D array [batch, length]")
        kind = self._resolve_kind(x.shape[1], input_vector_type)
        x = np.ascontiguousarray(x & 1 if x.dtype != np.uint8 else x, dtype=np.uint8)
        batch = x.shape[0]
        if batch == 0:
            raise ValueError("empty batch")
        bits = np.empty((batch, self.n), dtype=np.uint8)
        llr = np.empty((batch, self.n), dtype=np.float64 if f64 else np.float32) if want_llr else None
        iters = np.empty(batch, dtype=np.int32)
        conv = np.empty(batch, dtype=np.uint8)
        flags = _lib.F_EARLY_EXIT if early_exit else 0
        cp = None
        if channel_probs is not None:
            cp = np.ascontiguousarray(channel_probs, dtype=np.float64 if f64 else np.float32)
            if cp.ndim != 2 or cp.shape[0] != batch:
                raise ValueError(f"channel_probs must be a 2-D array [batch = {batch}, k], got shape {cp.shape}")
            if not 1 <= cp.shape[1] <= self.n:
                raise ValueError(f"channel_probs covers {cp.shape[1]} columns: expected 1 to n = {self.n}")
        if f64:
            _lib.check(
                self._lib.scaldpc_bp_decode_batch_f64(
                    self._h, _lib.ptr(x), kind, batch, _lib.ptr(cp), 0 if cp is None else cp.shape[1],
                    self.max_iter if max_iter is None else int(max_iter), flags, None,
                    _lib.ptr(bits), _lib.ptr(llr), _lib.ptr(iters), _lib.ptr(conv),
                )  # fmt: skip
            )
            return {"bits": bits, "llr": llr, "iters": iters, "converged": conv}
        if cp is not None:
            _lib.check(
                self._lib.scaldpc_bp_decode_batch_soft(
                    self._h, _lib.ptr(x), kind, batch, _lib.ptr(cp), cp.shape[1],
                    self.max_iter if max_iter is None else int(max_iter), self._method, self.ms_scaling_factor, flags, None,
                    _lib.ptr(bits), _lib.ptr(llr), _lib.ptr(iters), _lib.ptr(conv),
                )  # fmt: skip
            )
            return {"bits": bits, "llr": llr, "iters": iters, "converged": conv}
        _lib.check(
            self._lib.scaldpc_bp_decode_batch(
                self._h, _lib.ptr(x), kind, batch, self.max_iter if max_iter is None else int(max_iter),
                self._method, self.ms_scaling_factor, flags, None, _lib.ptr(bits), _lib.ptr(llr),
                _lib.ptr(iters), _lib.ptr(conv),
            )  # fmt: skip
        )
        return {"bits": bits, "llr": llr, "iters": iters, "converged": conv}

    def decode_batch_device(self, d_in, kind, batch, d_out_bits, max_iter=None, early_exit=False, stream=0,
                            d_out_llr=0, d_out_iters=0, d_out_conv=0, asynchronous=False, d_channel_probs=0, prob_cols=0,
                            precision=None):
        """Device-pointer variant (ints, e.g. torch `tensor.data_ptr()`): nothing crosses PCIe.
        d_channel_probs / prob_cols: float32 [batch, prob_cols] per-codeword priors of the last prob_cols columns (see
        decode_batch); a value that is no probability raises ValueError when the call synchronises -- an asynchronous
        call does not check.
        precision: None (the decoder's), "float32" or "float64"; with "float64" d_out_llr and d_channel_probs hold float64
        and the call cannot be asynchronous (scaldpc_bp_decode_batch_f64)."""
        flags = _lib.F_DEVICE_IO | (_lib.F_EARLY_EXIT if early_exit else 0) | (_lib.F_ASYNC if asynchronous else 0)
        if (self.precision if precision is None else _precision(precision, self._method)) == "float64":
            _lib.check(
                self._lib.scaldpc_bp_decode_batch_f64(
                    self._h, C.c_void_p(d_in), kind, batch, C.c_void_p(d_channel_probs or None), int(prob_cols),
                    self.max_iter if max_iter is None else int(max_iter), flags, C.c_void_p(stream or None),
                    C.c_void_p(d_out_bits), C.c_void_p(d_out_llr or None), C.c_void_p(d_out_iters or None),
                    C.c_void_p(d_out_conv or None),
                )  # fmt: skip
            )
            return
        if d_channel_probs or prob_cols:
            _lib.check(
                self._lib.scaldpc_bp_decode_batch_soft(
                    self._h, C.c_void_p(d_in), kind, batch, C.c_void_p(d_channel_probs or None), int(prob_cols),
                    self.max_iter if max_iter is None else int(max_iter), self._method, self.ms_scaling_factor, flags,
                    C.c_void_p(stream or None), C.c_void_p(d_out_bits), C.c_void_p(d_out_llr or None),
                    C.c_void_p(d_out_iters or None), C.c_void_p(d_out_conv or None),
                )  # fmt: skip
            )
            return
        _lib.check(
            self._lib.scaldpc_bp_decode_batch(
                self._h, C.c_void_p(d_in), kind, batch, self.max_iter if max_iter is None else int(max_iter),
                self._method, self.ms_scaling_factor, flags, C.c_void_p(stream or None), C.c_void_p(d_out_bits),
                C.c_void_p(d_out_llr or None), C.c_void_p(d_out_iters or None), C.c_void_p(d_out_conv or None),
            )  # fmt: skip
        )

    def time_kernels(self, iters, stream=0):
        """HIP-event timing of the check / variable kernels on the last decode's state.
        Returns dict(ms_check, ms_var, launches_check, launches_var, codewords per check launch, lanes);
        lanes = 2: the two series ran concurrently on the two streams of the decode's schedule."""
        ms = (C.c_float * 2)()
        ln = (C.c_int32 * 6)()
        _lib.check(
            self._lib.scaldpc_bp_time_kernels(
                self._h, iters, self._method, self.ms_scaling_factor, C.c_void_p(stream or None), ms, ln
            )
        )
        return {"ms_check": ms[0], "ms_var": ms[1], "launches_check": ln[0], "launches_var": ln[1], "codewords": ln[2],
                "lanes": ln[3], "codewords_var": ln[4], "record_form": bool(ln[5] & 1),
                # the variable pass is timed in the form the last decode launched it in (early exit: every pass writes
                # decisions for all columns; fixed iterations: no output, record form without the degree <= 1 columns)
                "var_writes_out": bool(ln[5] & 2), "var_slim": bool(ln[5] & 4)}

    # -- Monte-Carlo helpers on the device (K6) --------------------------------------
    def mc_fer_run(self, runs, seed, first_trial=0, max_iter=None, early_exit=True, want_errors=False, precision="float32"):
        """`runs` trials of the FER loop body (simulate/decode.py:165-175) entirely on the
        device: error ~ Bernoulli(channel_probs), syndrome, decode, compare.
        precision: "float32" (the default WHATEVER the decoder's own `precision`: the sweeps have always run the fp32 kernels)
        or "float64": the same trials decoded by the reference's float64 recursion (scaldpc_mc_fer_run_f64), product-sum only.
        Returns dict(success uint8 [runs], iters int32 [runs], errors uint8 [runs, n] or None)."""
        return _mc_fer(self, int(first_trial), int(runs), "", seed, max_iter, early_exit, want_errors, precision)

    def mc_fer_run_at(self, trial_ids, seed, max_iter=None, early_exit=True, want_errors=False, precision="float32"):
        """`mc_fer_run` on CHOSEN trials: slot i of the result is global trial `trial_ids[i]` (any order, duplicates allowed,
        indices up to 2^63 - 1), row for row what `mc_fer_run` returns for that index on any range that contains it
        (scaldpc_mc_fer_run_at / _at_f64).  trial_ids: a one-dimensional array of non-negative integers (ValueError
        otherwise, before any library call; a float array is refused, not rounded).  Returns `mc_fer_run`'s dict with
        len(trial_ids) rows."""
        ids = _lib.trial_ids(trial_ids)
        return _mc_fer(self, _lib.ptr(ids), len(ids), "_at", seed, max_iter, early_exit, want_errors, precision)

    def mc_hqc_run(self, runs, omega, eps, seed, first_trial=0, max_iter=None, early_exit=True, want_inputs=False,
                   want_stats=False, want_bits=False, precision="float32"):
        """`runs` synthetic hqc.decode() trials (simulate/hqc.py:684-705,742-749) on H = [Hin | I]:
        secret y, noisy checks, msg = [0]*N ++ checks, decode, success = (decoded[:N] == y).
        Returns dict(success, iters, msg uint8 [runs, n] or None, y int32 [runs, omega] or None).
        want_stats / want_bits: the same trials through scaldpc_mc_hqc_run_stats with the two-outcome table that IS this sweep
        (include/scaldpc.h); the result gains `stats` and `bits` as `mc_hqc_run_soft`'s does.
        precision: "float32" (the default WHATEVER the decoder's own `precision`) or "float64": the same trials decoded by the
        reference's float64 recursion (scaldpc_mc_hqc_run_f64; with want_stats / want_bits the two-outcome table through
        scaldpc_mc_hqc_run_stats_f64, its probabilities unrounded), product-sum only."""
        f64 = _precision(precision, self._method) == "float64"
        if want_stats or want_bits:
            eps = float(eps)
            table = dict(weights=np.array([[eps, 1.0 - eps]] * 2), flips=np.array([1, 0], dtype=np.uint8),
                         probs=np.array([eps, eps]), costs=None)
            r = self.mc_hqc_run_soft(runs, omega, table, seed, first_trial=first_trial, max_iter=max_iter, early_exit=early_exit,
                                     want_inputs=want_inputs, want_stats=want_stats, want_bits=want_bits, precision=precision)
            return {k: r[k] for k in ("success", "iters", "msg", "y", "stats", "bits")}
        succ = np.empty(runs, dtype=np.uint8)
        iters = np.empty(runs, dtype=np.int32)
        msg = np.empty((runs, self.n), dtype=np.uint8) if want_inputs else None
        y = np.empty((runs, omega), dtype=np.int32) if want_inputs else None
        args = (
            self._h, int(omega), float(eps), int(first_trial), int(runs), int(seed),
            self.max_iter if max_iter is None else int(max_iter),
            *(() if f64 else (self._method, self.ms_scaling_factor)),  # (no method, no alpha: product-sum only)
            _lib.F_EARLY_EXIT if early_exit else 0, None, _lib.ptr(succ), _lib.ptr(iters), _lib.ptr(msg), _lib.ptr(y),
        )  # fmt: skip
        _lib.check(getattr(self._lib, "scaldpc_mc_hqc_run" + ("_f64" if f64 else ""))(*args))
        return {"success": succ, "iters": iters, "msg": msg, "y": y}

    def mc_hqc_run_at(self, trial_ids, omega, eps, seed, max_iter=None, early_exit=True, want_inputs=False, want_stats=False,
                      want_bits=False, precision="float32"):
        """`mc_hqc_run` on CHOSEN trials: slot i of the result is global trial `trial_ids[i]`, row for row what `mc_hqc_run`
        returns for that index on any range that contains it.  Always through the two-outcome table that IS this sweep
        (scaldpc_mc_hqc_run_stats_at), as `mc_hqc_run(want_stats=True)` goes.  trial_ids: as `mc_fer_run_at`'s.  Returns
        `mc_hqc_run`'s dict with len(trial_ids) rows (`stats` / `bits` with want_stats / want_bits)."""
        ids = _lib.trial_ids(trial_ids)
        _precision(precision, self._method)
        eps = float(eps)
        table = dict(weights=np.array([[eps, 1.0 - eps]] * 2), flips=np.array([1, 0], dtype=np.uint8),
                     probs=np.array([eps, eps]), costs=None)
        r = self.mc_hqc_run_soft_at(ids, omega, table, seed, max_iter=max_iter, early_exit=early_exit, want_inputs=want_inputs,
                                    want_stats=want_stats, want_bits=want_bits, precision=precision)
        return {k: r[k] for k in ("success", "iters", "msg", "y") + (("stats", "bits") if want_stats or want_bits else ())}

    def mc_hqc_run_soft_at(self, trial_ids, omega, table, seed, max_iter=None, early_exit=True, want_inputs=False,
                           want_stats=False, want_bits=False, precision="float32"):
        """`mc_hqc_run_soft` on CHOSEN trials: slot i of the result is global trial `trial_ids[i]` (any order, duplicates
        allowed, indices up to 2^63 - 1), row for row -- success, iters, flips, cost, msg, y, outcome, stats, bits -- what
        `mc_hqc_run_soft` returns for that index on any range that contains it (scaldpc_mc_hqc_run_stats_at / _at_f64, whose
        out_stats is optional).  trial_ids: a one-dimensional array of non-negative integers (ValueError otherwise, before
        any library call; a float array is refused, not rounded).  Returns `mc_hqc_run_soft`'s dict with len(trial_ids) rows."""
        ids = _lib.trial_ids(trial_ids)
        return _mc_hqc_soft(self, _lib.ptr(ids), len(ids), True, omega, table, seed, max_iter, early_exit, want_inputs, want_stats,
                                 want_bits, precision)

    def mc_hqc_run_soft(self, runs, omega, table, seed, first_trial=0, max_iter=None, early_exit=True, want_inputs=False,
                        want_stats=False, want_bits=False, precision="float32"):
        """`runs` synthetic hqc.decode() trials whose checks come from the oracles of simulate/hqc.py:782-871: every check
        draws an OUTCOME conditional on its true value, and the outcome brings the reported bit, the certainty the decoder
        is given with it (its own prior, hqc.py:689) and the oracle calls it spent -- all on the device
        (scaldpc_mc_hqc_run_soft; the law is stated in include/scaldpc.h).

          table  dict(weights [2, K], flips [K], probs [K], costs [K] or None), e.g. `trials.wrapped_oracle_table(...)`:
                 weights[b] = probabilities of the K outcomes when the true check bit is b, flips = 1 where the reported bit
                 is the complement, probs = the prior error probability given with the outcome (float32), costs = oracle calls
        Returns dict(success uint8 [runs], iters int32 [runs], flips int32 [runs] (checks reported wrong), cost int32 [runs]
        (oracle calls of the trial; None without costs in the table), and with want_inputs msg uint8 [runs, n],
        y int32 [runs, omega], outcome uint8 [runs, R] (else None)).
        want_stats / want_bits: the call goes through scaldpc_mc_hqc_run_stats and the result gains
          stats  int32 [runs, 5]: per trial the counters of tracking.add_decoder_stats (hqc.py:709-758) in the order of
                 HQC_STATS_COLUMNS -- what `driver.hqc_stats` counts on the decoded word, counted on the device
          bits   uint8 [runs, n] with want_bits (else None): the decoded word, `decode_batch`'s bits for `msg`
        everything else is unchanged; without the two flags the call and its result are the plain sweep's.
        precision: "float32" (the default WHATEVER the decoder's own `precision`) or "float64": the same trials -- inputs,
        outcomes, flips and costs bit for bit -- decoded by the reference's float64 recursion (scaldpc_mc_hqc_run_stats_f64),
        product-sum only; the table's `probs` then go in as float64, unrounded."""
        return _mc_hqc_soft(self, int(first_trial), int(runs), False, omega, table, seed, max_iter, early_exit, want_inputs,
                                 want_stats, want_bits, precision)

    def last_compacted(self):
        """Codewords the last early-exit call re-decoded in its compact second pass."""
        c = C.c_int64()
        _lib.check(self._lib.scaldpc_bp_last_compacted(self._h, C.byref(c)))
        return int(c.value)

    def last_stats(self):
        """Path statistics of the last call: codewords handed to the compact pass, codewords decoded
        with the row-parallel (lane = edge) kernels, deepest compaction level reached."""
        out = (C.c_int64 * 4)()
        _lib.check(self._lib.scaldpc_bp_last_stats(self._h, out))
        return {"compacted": int(out[0]), "row_parallel": int(out[1]), "levels": int(out[2])}

    def last_schedule(self):
        """The schedule the last call ran on the tile kernels (scaldpc_bp_last_schedule): host-side counters, reset when
        a call starts.  groups / handed_down are per compaction level; the rest says where the early-exit scheduler
        polled, which groups stopped at the hand-over point unseen, which were chained lane to lane, and how often the
        ring of "still running" counter rows wrapped."""
        out = (C.c_int64 * 24)()
        _lib.check(self._lib.scaldpc_bp_last_schedule(self._h, out))
        w = [int(x) for x in out]
        return {"groups": w[0:4], "handed_down": w[4:7], "polls": w[7], "unseen": w[8], "continued": w[9],
                "left_open": w[10], "fixed_chained": w[11], "clears": w[12], "open_at_clear": w[13], "ring_rows": w[14],
                "row_parallel_polls": w[15], "ring_takes": w[16]}  # fmt: skip

    def last_settle(self):
        """Settled codewords in the last call (scaldpc_bp_last_settle): frozen_at = per 64-codeword tile the first iteration
        from which every pass repeated the one before (0 = never; empty = the call did not track), launches_saved = kernel
        launches the settle horizon did not enqueue, tiles_rerun = tiles decoded again because the horizon was too short for
        them, horizon = the K the call ran with (0 = none)."""
        info = (C.c_int64 * 4)()
        _lib.check(self._lib.scaldpc_bp_last_settle(self._h, None, 0, info))
        tiles = int(info[0])
        at = (C.c_int32 * max(tiles, 1))()
        _lib.check(self._lib.scaldpc_bp_last_settle(self._h, at, tiles, info))
        return {"frozen_at": [int(x) for x in at[:tiles]], "launches_saved": int(info[1]), "tiles_rerun": int(info[2]),
                "horizon": int(info[3])}

    def debug_sparse_flags(self):
        """The sparse settle gate's tables after the last (synchronous) call (scaldpc_bp_debug_sparse_flags): per tile a dict
        row_stamp uint32 [m], row_dirty uint64 [m], col_flag uint32 [n]; [] = the call did not use them."""
        info = (C.c_int64 * 4)()
        _lib.check(self._lib.scaldpc_bp_debug_sparse_flags(self._h, 0, None, None, None, info))
        tiles, m, n = (int(x) for x in info[:3])
        out = []
        for t in range(tiles):
            rs, rd, cf = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
            _lib.check(self._lib.scaldpc_bp_debug_sparse_flags(
                self._h, t, rs.ctypes.data_as(C.POINTER(C.c_uint32)), rd.ctypes.data_as(C.POINTER(C.c_uint64)),
                cf.ctypes.data_as(C.POINTER(C.c_uint32)), info))
            out.append({"row_stamp": rs, "row_dirty": rd, "col_flag": cf})
        return out

    def debug_sparse_start(self):
        """The variable pass from which the last call's sparse gate gated (0 = the call did not use the gate)."""
        info = (C.c_int64 * 4)()
        _lib.check(self._lib.scaldpc_bp_debug_sparse_flags(self._h, 0, None, None, None, info))
        return int(info[3])

    def last_row_parallel(self):
        return self.last_stats()["row_parallel"]

    def configure(self, **knobs):
        """Tuning / test knobs of this decoder (include/scaldpc.h, scaldpc_bp_configure): path, split,
        group_mb, el_max, compact_after, first_fused, fuse_test, minsum_rec, settle, settle_horizon, settle_sparse.  A new decoder takes its
        defaults from the SCALDPC_* environment once, at construction; results never depend on them.
        minsum_rec=2 (passed through as it is): 1, and columns of 33 ... 64 edges stay in min-sum's record form -- opt-in;
        by default, and under 1, a graph with such a column runs the message form."""
        for k, v in knobs.items():
            _lib.check(self._lib.scaldpc_bp_configure(self._h, k.encode(), str(v).encode()))

    def device_of(self):
        """{device the decoder was created on, device of its graph / message / state allocations (-1: none yet)}."""
        out = (C.c_int32 * 4)()
        _lib.check(self._lib.scaldpc_bp_device_of(self._h, out))
        return {"device": out[0], "graph": out[1], "messages": out[2], "state": out[3]}

    def set_tile_group(self, tiles):
        _lib.check(self._lib.scaldpc_bp_set_tile_group(self._h, int(tiles)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.scaldpc_bp_destroy(self._h)
            self._h = None

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


# The bodies the contiguous sweeps share with their `_at` forms (dec: the decoder).
def _mc_fer(dec, trials, runs, at, seed, max_iter, early_exit, want_errors, precision):
    # trials: the first index ("" = the contiguous entries) or the pointer to an int64 list ("_at" = the list entries).
    f64 = _precision(precision, dec._method) == "float64"
    succ = np.empty(runs, dtype=np.uint8)
    iters = np.empty(runs, dtype=np.int32)
    err = np.empty((runs, dec.n), dtype=np.uint8) if want_errors else None
    args = (
        dec._h, trials, runs, int(seed), dec.max_iter if max_iter is None else int(max_iter),
        *(() if f64 else (dec._method, dec.ms_scaling_factor)),  # (no method, no alpha: product-sum only)
        _lib.F_EARLY_EXIT if early_exit else 0, None, _lib.ptr(succ), _lib.ptr(iters), _lib.ptr(err),
    )  # fmt: skip
    _lib.check(getattr(dec._lib, f"scaldpc_mc_fer_run{at}" + ("_f64" if f64 else ""))(*args))
    return {"success": succ, "iters": iters, "errors": err}


def _mc_hqc_soft(dec, trials, runs, listed, omega, table, seed, max_iter, early_exit, want_inputs, want_stats, want_bits,
                 precision):
    # trials: the first index of a contiguous call, or (listed) the pointer to the int64 list of an _at call
    f64 = _precision(precision, dec._method) == "float64"
    w = np.ascontiguousarray(table["weights"], dtype=np.float64)
    if w.ndim != 2 or w.shape[0] != 2:
        raise ValueError(f"table['weights'] must be [2, K], got shape {w.shape}")
    K = w.shape[1]
    fl = np.asarray(table["flips"])
    pr = np.ascontiguousarray(table["probs"], dtype=np.float64 if f64 else np.float32)
    costs = table.get("costs")
    if fl.shape != (K,) or pr.shape != (K,) or (costs is not None and np.shape(costs) != (K,)):
        raise ValueError(f"table: flips, probs and costs must hold one entry per outcome (K = {K})")
    # (the library validates the values; here only what a conversion to its types would hide)
    cs = None if costs is None else np.asarray(costs)
    for name, a, t in (("flips", fl, np.uint8), ("costs", cs, np.int32)):
        if a is not None and not np.array_equal(a.astype(t), a):
            raise ValueError(f"table['{name}'] = {a.tolist()} does not fit {np.dtype(t).name}")
    fl = np.ascontiguousarray(fl, dtype=np.uint8)
    cs = None if cs is None else np.ascontiguousarray(cs, dtype=np.int32)
    succ = np.empty(runs, dtype=np.uint8)
    iters = np.empty(runs, dtype=np.int32)
    flips = np.empty(runs, dtype=np.int32)
    cost = np.empty(runs, dtype=np.int32) if costs is not None else None
    msg = np.empty((runs, dec.n), dtype=np.uint8) if want_inputs else None
    y = np.empty((runs, omega), dtype=np.int32) if want_inputs else None
    outcome = np.empty((runs, dec.m), dtype=np.uint8) if want_inputs else None
    args = (
        dec._h, int(omega), _lib.ptr(w), _lib.ptr(fl), _lib.ptr(pr), _lib.ptr(cs), K,
        trials, runs, int(seed), dec.max_iter if max_iter is None else int(max_iter),
        *(() if f64 else (dec._method, dec.ms_scaling_factor)),  # (no method, no alpha: product-sum only)
        _lib.F_EARLY_EXIT if early_exit else 0, None, _lib.ptr(succ), _lib.ptr(iters),
        _lib.ptr(msg), _lib.ptr(y), _lib.ptr(outcome), _lib.ptr(flips), _lib.ptr(cost),
    )  # fmt: skip
    res = {"success": succ, "iters": iters, "flips": flips, "cost": cost, "msg": msg, "y": y, "outcome": outcome}
    want = want_stats or want_bits
    # a list or a float64 decode has one entry, whose out_stats is optional; the contiguous fp32 call without either flag is the
    # plain sweep, whose argument list ends before out_stats / out_bits
    with_stats = want or listed or f64
    entry = "scaldpc_mc_hqc_run_" + ("stats" if with_stats else "soft") + ("_at" if listed else "") + ("_f64" if f64 else "")
    stats = np.empty((runs, len(HQC_STATS_COLUMNS)), dtype=np.int32) if want else None
    bits = np.empty((runs, dec.n), dtype=np.uint8) if want_bits else None
    _lib.check(getattr(dec._lib, entry)(*args, *((_lib.ptr(stats), _lib.ptr(bits)) if with_stats else ())))
    return dict(res, stats=stats, bits=bits) if want else res


bp_decoder = BpDecoder
