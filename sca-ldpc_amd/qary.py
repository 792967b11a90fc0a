"""`simulate_rs`-shaped front end of the HIP q-ary min-sum decoders.

The reference generates one PyO3 class per compile-time size
(`register_py_decoder_class!`, simulate_rs/src/pydecoder.rs:12-70; sizes listed in
simulate_rs/src/lib.rs:32-75) and looks them up by name
(`getattr(simulate_rs, f"DecoderN{n}R{r}V{v}C{c}B{B}")`, simulate/decode.py:227-229).
Here sizes are run-time values: `decoder_class("DecoderN450R150V3C7B1")` builds a class
with the same constructor / `min_sum` surface for ANY name of that pattern, plus
`min_sum_batch` for many channel outputs per call, and `min_sum_soft` / `min_sum_soft_batch` for what the decoders
compute beyond the symbols: the last variable update's per-symbol totals, the margin of every decision and the number
of checks the decided word leaves unmet (include/scaldpc.h, scaldpc_qary_min_sum_batch_soft).
`mc_run` / `mc_run_device` run whole Monte-Carlo trials of the reference's q-ary sweep on the device: the symbols' pmf rows
are drawn there from a small table of levels, and one flag per trial comes back (include/scaldpc.h, scaldpc_mc_qary_run).
`QarySpecialDecoder.mc_run_secret` / `mc_run_secret_device` run the Kyber attack's trial instead: a secret drawn from a prior, the
row sums that follow from it, every variable answered by an oracle outcome drawn conditional on its true symbol -- is the key
recovered (include/scaldpc.h, scaldpc_mc_qary_run_secret; the tables: trials.oracle_posterior_table).

  DecoderN{N}R{R}V{DV}C{DC}B{B}(H: int8 [R, N], iterations)   .min_sum(pmf float32 [N, 2B+1]) -> list[int]
  DecoderN{N}R{R}SW{SW}(H: int8 [R, N], iterations)           .min_sum(pmf [N-R, 5], pmf_sum [R, 2*BSUM+1]) -> list[int]
      (B = 2, BSUM = SW*B, DC = SW+1: the Kyber decoders of lib.rs:54-75)
  DecoderN{N}R{R}SW{SW}B{B}(H: int8 [R, N], iterations)       .min_sum(pmf [N-R, 2B+1], pmf_sum [R, 2*SW*B+1]) -> list[int]
      (this project's extension of the name above to any B: BSUM = SW*B, DC = SW+1.  Rows of more than 7 coefficient
      edges run on the min-plus recursion for rows of any length, B = 1, 2, 3 and 2*B*SW + 1 <= 85:
      DecoderN1024R256SW9B2 is what the reference would call DecoderN1024R256SW9)

Inputs are probabilities; the LLR conversion (decoder.rs:668-692) happens inside, as in
the reference.  Errors: a pmf row not summing to 1 +- 1e-3 and a check without any
finite configuration raise (the reference panics); shape mismatches raise ValueError.
`min_sum` may be called concurrently from many Python threads on one object (the
reference's thread pool does, decode.py:247-262): calls are serialised in the library
and ctypes releases the GIL meanwhile.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import _lib

_GENERIC = re.compile(r"^DecoderN(\d+)R(\d+)V(\d+)C(\d+)B(\d+)$")
_SPECIAL = re.compile(r"^DecoderN(\d+)R(\d+)SW(\d+)$")
_SPECIAL_B = re.compile(r"^DecoderN(\d+)R(\d+)SW(\d+)B(\d+)$")


class _QaryBase:
    N = R = DV = DC = B = Q = 0

    def _check_H(self, H):
        H = np.asarray(H)
        if H.dtype != np.int8:
            raise TypeError("parity check matrix must have dtype int8 (as PyReadonlyArray2<i8>, pydecoder.rs:24)")
        if H.shape != (self.R, self.N):
            raise ValueError(f"parity check matrix has shape {H.shape}, this decoder is built for ({self.R}, {self.N})")
        nz = H != 0
        if nz.sum(axis=0).max() > self.DV or nz.sum(axis=1).max() > self.DC:
            # the reference panics in insert_first_none (decoder.rs:465-473)
            raise ValueError("Reached the end of the array, no more space left! (node degree exceeds DV/DC)")
        return np.ascontiguousarray(H)

    def configure(self, **knobs):
        """wave = -1 (auto) / 0 / 1, unroll = 0 / 1, tree = 0 / 1, dp = 0 / 1, dp_min = batch from which dp applies,
        dp_any = -1 (auto) / 0 / 1, timing = 0 / 1 (include/scaldpc.h, scaldpc_qary_configure)."""
        for k, v in knobs.items():
            _lib.check(self._lib.scaldpc_qary_configure(self._h, k.encode(), str(v).encode()))

    CHECK_KERNELS = ("k_q_check_unrolled<3,7>", "k_q_check_unrolled<5,5>", "k_q_special_check_tree<5,6>",
                     "k_q_special_check_wave", "k_q_check_wave", "k_q_special_check", "k_q_check", "k_q_special_check_dp<5,6>", "k_q_check_dp<3,7>",
                     "k_q_special_check_dp_any")

    def last_timing(self):
        """HIP-event times of the last call's launches (after `configure(timing=1)`; bench.py's measurement aid):
        dict(ms_check, ms_var, ms_loop, iterations, check_kernel, batch, max_check_degree)."""
        ms = (C.c_float * 3)()
        info = (C.c_int32 * 4)()
        _lib.check(self._lib.scaldpc_qary_last_timing(self._h, ms, info))
        return {"ms_check": ms[0], "ms_var": ms[1], "ms_loop": ms[2], "iterations": info[0],
                "check_kernel": self.CHECK_KERNELS[info[1]] if info[1] >= 0 else None, "batch": info[2],
                "max_check_degree": info[3]}

    # -- Monte-Carlo trials drawn on the device (include/scaldpc.h, scaldpc_mc_qary_run) -------------------------------
    @staticmethod
    def _mc_table(levels, weights, Q, what):
        """One level table as the C entry point takes it: float32 [K, Q] pmf rows, float64 [K] probabilities."""
        lv = np.ascontiguousarray(levels, dtype=np.float32)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if lv.ndim != 2 or lv.shape[1] != Q or w.shape != (lv.shape[0],):
            raise ValueError(f"{what}: levels {lv.shape} / weights {w.shape}, expected (K, {Q}) pmf rows and (K,) probabilities")
        return lv, w

    def _mc_call(self, tables, first_trial, runs, seed, flags, stream, outs, trial_ids=None):
        # trial_ids: None (a contiguous call from first_trial), or the int64 list `_lib.trial_ids` returned (an _at call)
        (lb, wb), (ls, ws) = tables
        listed = trial_ids is not None
        entry = self._lib.scaldpc_mc_qary_run_at if listed else self._lib.scaldpc_mc_qary_run
        _lib.check(entry(
            self._h, _lib.ptr(lb), _lib.ptr(wb), lb.shape[0], _lib.ptr(ls), _lib.ptr(ws), 0 if ls is None else ls.shape[0],
            _lib.ptr(trial_ids) if listed else int(first_trial), int(runs), int(seed), flags, C.c_void_p(stream or None), *outs))

    def _mc_host(self, tables, runs, seed, first_trial, want_levels, want_symbols, trial_ids=None):
        runs = int(runs)
        if runs <= 0:
            raise ValueError("runs must be positive")
        res = {"success": np.empty(runs, dtype=np.uint8), "errs": np.empty(runs, dtype=np.int32),
               "wrong": np.empty(runs, dtype=np.int32)}
        if want_levels:
            res["levels"] = np.empty((runs, self.N), dtype=np.uint8)
        if want_symbols:
            res["symbols"] = np.empty((runs, self.N), dtype=np.int8)
        self._mc_call(tables, first_trial, runs, seed, 0, 0, [_lib.ptr(res.get(k)) for k in ("success", "errs", "wrong", "levels", "symbols")],
                      trial_ids)
        return res

    def _mc_device(self, tables, runs, seed, first_trial, stream, d_outs, trial_ids=None):
        self._mc_call(tables, first_trial, runs, seed, _lib.F_DEVICE_IO, stream, [C.c_void_p(d or None) for d in d_outs], trial_ids)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.scaldpc_qary_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QaryDecoder(_QaryBase):
    """Decoder<N, R, DV, DC, Q=2B+1, B, i8> (decoder.rs:417-438)."""

    def __init__(self, py_parity_check, iterations):
        self._h = None
        self._lib = _lib.load()
        H = self._check_H(py_parity_check)
        h = C.c_void_p()
        _lib.check(self._lib.scaldpc_qary_create(self.R, self.N, self.B, _lib.ptr(H), int(iterations), C.byref(h)))
        self._h = h

    def min_sum_batch(self, channel_output):
        """float32 [batch, N, Q] -> int8 [batch, N]."""
        p = np.ascontiguousarray(channel_output, dtype=np.float32)
        if p.ndim != 3 or p.shape[1:] != (self.N, self.Q):
            raise ValueError(f"channel output has shape {p.shape}, expected (batch, {self.N}, {self.Q})")
        out = np.empty((p.shape[0], self.N), dtype=np.int8)
        _lib.check(self._lib.scaldpc_qary_min_sum_batch(self._h, _lib.ptr(p), p.shape[0], 0, None, _lib.ptr(out)))
        return out

    def min_sum_batch_device(self, d_channel_output, batch, d_out, stream=0):
        """Device-pointer variant (ints, e.g. torch `tensor.data_ptr()`): float32 [batch, N, Q] probabilities in HBM ->
        int8 [batch, N] in HBM; nothing crosses PCIe.  Returns after the stream work is complete."""
        _lib.check(self._lib.scaldpc_qary_min_sum_batch(self._h, C.c_void_p(d_channel_output), int(batch), _lib.F_DEVICE_IO,
                                                        C.c_void_p(stream or None), C.c_void_p(d_out)))

    def min_sum(self, py_channel_output):
        p = np.asarray(py_channel_output)
        if p.shape != (self.N, self.Q):
            raise ValueError(f"channel output has shape {p.shape}, expected ({self.N}, {self.Q})")
        return [int(x) for x in self.min_sum_batch(p[None])[0]]

    def min_sum_soft_batch(self, channel_output, costs=True, margins=True, unmet=True):
        """float32 [batch, N, Q] -> dict(symbols int8 [batch, N], costs float32 [batch, N, Q] (the last variable update's
        totals, index q = value q - B), margins float32 [batch, N] (runner-up total minus the decided one), unmet int32
        [batch] (checks the symbols leave unmet; 0 = a valid word)); entries not asked for are absent."""
        p = np.ascontiguousarray(channel_output, dtype=np.float32)
        if p.ndim != 3 or p.shape[1:] != (self.N, self.Q):
            raise ValueError(f"channel output has shape {p.shape}, expected (batch, {self.N}, {self.Q})")
        nb = p.shape[0]
        res = {"symbols": np.empty((nb, self.N), dtype=np.int8)}
        if costs:
            res["costs"] = np.empty((nb, self.N, self.Q), dtype=np.float32)
        if margins:
            res["margins"] = np.empty((nb, self.N), dtype=np.float32)
        if unmet:
            res["unmet"] = np.empty(nb, dtype=np.int32)
        _lib.check(self._lib.scaldpc_qary_min_sum_batch_soft(
            self._h, _lib.ptr(p), nb, 0, None, _lib.ptr(res["symbols"]), _lib.ptr(res.get("costs")), _lib.ptr(res.get("margins")),
            _lib.ptr(res.get("unmet"))))
        return res

    def min_sum_soft_batch_device(self, d_channel_output, batch, d_out, d_costs=0, d_margins=0, d_unmet=0, stream=0):
        """Device-pointer variant (ints; 0 = not wanted): float32 [batch, N, Q] in HBM -> int8 [batch, N], float32
        [batch, N, Q], float32 [batch, N], int32 [batch] in HBM.  Returns after the stream work is complete."""
        _lib.check(self._lib.scaldpc_qary_min_sum_batch_soft(
            self._h, C.c_void_p(d_channel_output), int(batch), _lib.F_DEVICE_IO, C.c_void_p(stream or None), C.c_void_p(d_out),
            C.c_void_p(d_costs or None), C.c_void_p(d_margins or None), C.c_void_p(d_unmet or None)))

    def mc_run(self, runs, seed, levels, weights, first_trial=0, want_levels=False, want_symbols=False):
        """`runs` trials of the reference's q-ary sweep (decode.py:246-257), drawn on the device: every variable of an all-zero
        word takes the pmf row levels[k] (float32 [K, Q]) with probability weights[k], Philox-keyed by (seed, first_trial + i)
        -- a trial does not depend on how the sweep is cut into calls.  Returns dict(success uint8 [runs] (every decision 0),
        errs int32 [runs] (variables NOT at the last level: with levels (bad, good) the reference's `errs`), wrong int32 [runs]
        (decisions != 0)), with want_levels / want_symbols also levels uint8 [runs, N] / symbols int8 [runs, N]: the symbols
        are `min_sum_batch(levels[res["levels"]])`, bit for bit."""
        tables = (self._mc_table(levels, weights, self.Q, "levels"), (None, None))
        return self._mc_host(tables, runs, seed, first_trial, want_levels, want_symbols)

    def mc_run_device(self, runs, seed, levels, weights, d_success, d_errs=0, d_wrong=0, d_levels=0, d_symbols=0, first_trial=0,
                      stream=0):
        """Device-pointer variant (ints; 0 = not wanted): the outputs of `mc_run` into HBM; the tables stay host arrays.
        Returns after the stream work is complete."""
        tables = (self._mc_table(levels, weights, self.Q, "levels"), (None, None))
        self._mc_device(tables, runs, seed, first_trial, stream, (d_success, d_errs, d_wrong, d_levels, d_symbols))

    def mc_run_at(self, trial_ids, seed, levels, weights, want_levels=False, want_symbols=False):
        """`mc_run` on CHOSEN trials (scaldpc_mc_qary_run_at): slot i of the result is global trial `trial_ids[i]` (any order,
        duplicates allowed, indices up to 2^63 - 1), row for row what `mc_run` returns for that index on any range that
        contains it.  trial_ids: a one-dimensional array of non-negative integers (ValueError otherwise, before any library
        call; a float array is refused, not rounded).  Returns `mc_run`'s dict with len(trial_ids) rows."""
        ids = _lib.trial_ids(trial_ids)
        tables = (self._mc_table(levels, weights, self.Q, "levels"), (None, None))
        return self._mc_host(tables, len(ids), seed, 0, want_levels, want_symbols, trial_ids=ids)

    def mc_run_at_device(self, trial_ids, seed, levels, weights, d_success, d_errs=0, d_wrong=0, d_levels=0, d_symbols=0, stream=0):
        """Device-pointer variant of `mc_run_at` (ints; 0 = not wanted); the trial list and the tables stay host arrays."""
        ids = _lib.trial_ids(trial_ids)
        tables = (self._mc_table(levels, weights, self.Q, "levels"), (None, None))
        self._mc_device(tables, len(ids), seed, 0, stream, (d_success, d_errs, d_wrong, d_levels, d_symbols), trial_ids=ids)

    def min_sum_soft(self, py_channel_output, costs=True, margins=True, unmet=True):
        """The single-codeword twin of `min_sum`: symbols as a list of ints, costs [N, Q], margins [N], unmet an int."""
        p = np.asarray(py_channel_output)
        if p.shape != (self.N, self.Q):
            raise ValueError(f"channel output has shape {p.shape}, expected ({self.N}, {self.Q})")
        return _single(self.min_sum_soft_batch(p[None], costs, margins, unmet))


class QarySpecialDecoder(_QaryBase):
    """DecoderSpecial<N, R, N-R, DC-1, DC, DV, B, 2B+1, BSUM, 2BSUM+1, i8> (decoder_special.rs:294-322)."""

    BSUM = QS = 0

    def __init__(self, py_parity_check, iterations):
        self._h = None
        self._lib = _lib.load()
        H = self._check_H(py_parity_check)
        h = C.c_void_p()
        _lib.check(
            self._lib.scaldpc_qary_special_create(self.R, self.N, self.B, self.BSUM, _lib.ptr(H), int(iterations), C.byref(h))
        )
        self._h = h

    def min_sum_batch(self, channel_output, channel_output_sum):
        p = np.ascontiguousarray(channel_output, dtype=np.float32)
        ps = np.ascontiguousarray(channel_output_sum, dtype=np.float32)
        if p.ndim != 3 or p.shape[1:] != (self.N - self.R, self.Q):
            raise ValueError(f"channel output has shape {p.shape}, expected (batch, {self.N - self.R}, {self.Q})")
        if ps.shape != (p.shape[0], self.R, self.QS):
            raise ValueError(f"channel output sum has shape {ps.shape}, expected ({p.shape[0]}, {self.R}, {self.QS})")
        out = np.empty((p.shape[0], self.N), dtype=np.int8)
        _lib.check(
            self._lib.scaldpc_qary_special_min_sum_batch(self._h, _lib.ptr(p), _lib.ptr(ps), p.shape[0], 0, None, _lib.ptr(out))
        )
        return out

    def min_sum_batch_device(self, d_channel_output, d_channel_output_sum, batch, d_out, stream=0):
        """Device-pointer variant: float32 [batch, N-R, 2B+1] and [batch, R, 2BSUM+1] in HBM -> int8 [batch, N] in HBM."""
        _lib.check(self._lib.scaldpc_qary_special_min_sum_batch(self._h, C.c_void_p(d_channel_output), C.c_void_p(d_channel_output_sum),
                                                                int(batch), _lib.F_DEVICE_IO, C.c_void_p(stream or None),
                                                                C.c_void_p(d_out)))

    def min_sum(self, py_channel_output, py_channel_output_sum):
        p, ps = np.asarray(py_channel_output), np.asarray(py_channel_output_sum)
        if p.ndim != 2 or ps.ndim != 2:
            raise ValueError("channel outputs must be 2-D")
        return [int(x) for x in self.min_sum_batch(p[None], ps[None])[0]]

    def min_sum_soft_batch(self, channel_output, channel_output_sum, costs=True, margins=True, unmet=True):
        """As QaryDecoder.min_sum_soft_batch; the totals come as `costs` float32 [batch, N-R, 2B+1] and `costs_sum` float32
        [batch, R, 2BSUM+1] (the shapes of the two inputs), margins and symbols cover all N variables, and a check's sum
        includes its row-sum variable."""
        p = np.ascontiguousarray(channel_output, dtype=np.float32)
        ps = np.ascontiguousarray(channel_output_sum, dtype=np.float32)
        if p.ndim != 3 or p.shape[1:] != (self.N - self.R, self.Q):
            raise ValueError(f"channel output has shape {p.shape}, expected (batch, {self.N - self.R}, {self.Q})")
        if ps.shape != (p.shape[0], self.R, self.QS):
            raise ValueError(f"channel output sum has shape {ps.shape}, expected ({p.shape[0]}, {self.R}, {self.QS})")
        nb = p.shape[0]
        res = {"symbols": np.empty((nb, self.N), dtype=np.int8)}
        if costs:
            res["costs"] = np.empty((nb, self.N - self.R, self.Q), dtype=np.float32)
            res["costs_sum"] = np.empty((nb, self.R, self.QS), dtype=np.float32)
        if margins:
            res["margins"] = np.empty((nb, self.N), dtype=np.float32)
        if unmet:
            res["unmet"] = np.empty(nb, dtype=np.int32)
        _lib.check(self._lib.scaldpc_qary_special_min_sum_batch_soft(
            self._h, _lib.ptr(p), _lib.ptr(ps), nb, 0, None, _lib.ptr(res["symbols"]), _lib.ptr(res.get("costs")),
            _lib.ptr(res.get("costs_sum")), _lib.ptr(res.get("margins")), _lib.ptr(res.get("unmet"))))
        return res

    def min_sum_soft_batch_device(self, d_channel_output, d_channel_output_sum, batch, d_out, d_costs=0, d_costs_sum=0,
                                  d_margins=0, d_unmet=0, stream=0):
        """Device-pointer variant (ints; 0 = not wanted; d_costs and d_costs_sum together or not at all)."""
        _lib.check(self._lib.scaldpc_qary_special_min_sum_batch_soft(
            self._h, C.c_void_p(d_channel_output), C.c_void_p(d_channel_output_sum), int(batch), _lib.F_DEVICE_IO,
            C.c_void_p(stream or None), C.c_void_p(d_out), C.c_void_p(d_costs or None), C.c_void_p(d_costs_sum or None),
            C.c_void_p(d_margins or None), C.c_void_p(d_unmet or None)))

    def mc_run(self, runs, seed, levels, weights, levels_sum, weights_sum, first_trial=0, want_levels=False, want_symbols=False):
        """As QaryDecoder.mc_run, with a table of their own for the R row-sum variables: levels_sum float32 [K_s, 2BSUM+1],
        weights_sum [K_s].  `levels` and `symbols` cover all N variables (the row-sum variables last); the symbols are
        `min_sum_batch(levels[lv[:, :N-R]], levels_sum[lv[:, N-R:]])`, bit for bit."""
        tables = (self._mc_table(levels, weights, self.Q, "levels"), self._mc_table(levels_sum, weights_sum, self.QS, "levels_sum"))
        return self._mc_host(tables, runs, seed, first_trial, want_levels, want_symbols)

    def mc_run_device(self, runs, seed, levels, weights, levels_sum, weights_sum, d_success, d_errs=0, d_wrong=0, d_levels=0,
                      d_symbols=0, first_trial=0, stream=0):
        """Device-pointer variant (ints; 0 = not wanted); the tables stay host arrays."""
        tables = (self._mc_table(levels, weights, self.Q, "levels"), self._mc_table(levels_sum, weights_sum, self.QS, "levels_sum"))
        self._mc_device(tables, runs, seed, first_trial, stream, (d_success, d_errs, d_wrong, d_levels, d_symbols))

    def mc_run_at(self, trial_ids, seed, levels, weights, levels_sum, weights_sum, want_levels=False, want_symbols=False):
        """`mc_run` on CHOSEN trials (scaldpc_mc_qary_run_at): slot i of the result is global trial `trial_ids[i]`, row for row
        what `mc_run` returns for that index on any range that contains it.  trial_ids: as QaryDecoder.mc_run_at's."""
        ids = _lib.trial_ids(trial_ids)
        tables = (self._mc_table(levels, weights, self.Q, "levels"), self._mc_table(levels_sum, weights_sum, self.QS, "levels_sum"))
        return self._mc_host(tables, len(ids), seed, 0, want_levels, want_symbols, trial_ids=ids)

    def mc_run_at_device(self, trial_ids, seed, levels, weights, levels_sum, weights_sum, d_success, d_errs=0, d_wrong=0, d_levels=0,
                         d_symbols=0, stream=0):
        """Device-pointer variant of `mc_run_at` (ints; 0 = not wanted); the trial list and the tables stay host arrays."""
        ids = _lib.trial_ids(trial_ids)
        tables = (self._mc_table(levels, weights, self.Q, "levels"), self._mc_table(levels_sum, weights_sum, self.QS, "levels_sum"))
        self._mc_device(tables, len(ids), seed, 0, stream, (d_success, d_errs, d_wrong, d_levels, d_symbols), trial_ids=ids)

    # -- trials on drawn secrets under an oracle's law (include/scaldpc.h, scaldpc_mc_qary_run_secret) --------------------------
    @staticmethod
    def _secret_table(levels, weights, Q, what):
        """One table as the C entry point takes it: float32 [K, Q] pmf rows, float64 [Q, K] outcome laws (row = TRUE symbol)."""
        lv = np.ascontiguousarray(levels, dtype=np.float32)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if lv.ndim != 2 or lv.shape[1] != Q or w.shape != (Q, lv.shape[0]):
            raise ValueError(f"{what}: levels {lv.shape} / weights {w.shape}, expected (K, {Q}) pmf rows and ({Q}, K) outcome laws")
        return lv, w

    def _secret_call(self, prior, levels, weights, levels_sum, weights_sum, first_trial, runs, seed, flags, stream, outs, trial_ids=None):
        # trial_ids: None (a contiguous call from first_trial), or the int64 list `_lib.trial_ids` returned (an _at call)
        pr = np.ascontiguousarray(prior, dtype=np.float64)
        if pr.shape != (self.Q,):
            raise ValueError(f"prior has shape {pr.shape}, expected ({self.Q},)")
        lb, wb = self._secret_table(levels, weights, self.Q, "levels")
        ls, ws = self._secret_table(levels_sum, weights_sum, self.QS, "levels_sum")
        listed = trial_ids is not None
        entry = self._lib.scaldpc_mc_qary_run_secret_at if listed else self._lib.scaldpc_mc_qary_run_secret
        _lib.check(entry(
            self._h, _lib.ptr(pr), _lib.ptr(lb), _lib.ptr(wb), lb.shape[0], _lib.ptr(ls), _lib.ptr(ws), ls.shape[0],
            _lib.ptr(trial_ids) if listed else int(first_trial), int(runs), int(seed), flags, C.c_void_p(stream or None), *outs))

    def mc_run_secret(self, runs, seed, prior, levels, weights, levels_sum, weights_sum, first_trial=0, want_secret=False,
                      want_levels=False, want_symbols=False):
        """`runs` trials of the Kyber attack's decode (simulate/kyber.py), drawn on the device and Philox-keyed by (seed,
        first_trial + i): every coefficient draws its true symbol from `prior` (float64 [Q], index q = value q - B), every row-sum
        variable takes the one value that makes its check hold, and every variable draws an oracle outcome k with probability
        weights[s, k] (weights_sum[s, k]), s its TRUE symbol, which hands the decoder the pmf row levels[k] (levels_sum[k]) --
        `trials.oracle_posterior_table` builds both.  Returns dict(success uint8 [runs] (every coefficient decided as drawn: the key
        is recovered), wrong int32 [runs, 2] (decisions != secret over the coefficients, over the row sums), channel_wrong int32
        [runs, 2] (variables whose drawn row alone decides wrong)), with want_secret / want_levels / want_symbols also secret int8
        [runs, N], levels uint8 [runs, N], symbols int8 [runs, N]: the symbols are
        `min_sum_batch(levels[lv[:, :N-R]], levels_sum[lv[:, N-R:]])`, bit for bit."""
        return self._secret_host(runs, seed, prior, levels, weights, levels_sum, weights_sum, first_trial, want_secret, want_levels,
                                 want_symbols)

    def _secret_host(self, runs, seed, prior, levels, weights, levels_sum, weights_sum, first_trial, want_secret, want_levels, want_symbols,
                     trial_ids=None):
        runs = int(runs)
        if runs <= 0:
            raise ValueError("runs must be positive")
        res = {"success": np.empty(runs, dtype=np.uint8), "wrong": np.empty((runs, 2), dtype=np.int32),
               "channel_wrong": np.empty((runs, 2), dtype=np.int32)}
        if want_secret:
            res["secret"] = np.empty((runs, self.N), dtype=np.int8)
        if want_levels:
            res["levels"] = np.empty((runs, self.N), dtype=np.uint8)
        if want_symbols:
            res["symbols"] = np.empty((runs, self.N), dtype=np.int8)
        outs = [_lib.ptr(res.get(k)) for k in ("success", "wrong", "channel_wrong", "secret", "levels", "symbols")]
        self._secret_call(prior, levels, weights, levels_sum, weights_sum, first_trial, runs, seed, 0, 0, outs, trial_ids)
        return res

    def mc_run_secret_device(self, runs, seed, prior, levels, weights, levels_sum, weights_sum, d_success, d_wrong=0, d_channel_wrong=0,
                             d_secret=0, d_levels=0, d_symbols=0, first_trial=0, stream=0):
        """Device-pointer variant (ints; 0 = not wanted): the outputs of `mc_run_secret` into HBM; prior and tables stay host
        arrays.  Returns after the stream work is complete."""
        outs = [C.c_void_p(d or None) for d in (d_success, d_wrong, d_channel_wrong, d_secret, d_levels, d_symbols)]
        self._secret_call(prior, levels, weights, levels_sum, weights_sum, first_trial, runs, seed, _lib.F_DEVICE_IO, stream, outs)

    def mc_run_secret_at(self, trial_ids, seed, prior, levels, weights, levels_sum, weights_sum, want_secret=False, want_levels=False,
                         want_symbols=False):
        """`mc_run_secret` on CHOSEN trials (scaldpc_mc_qary_run_secret_at): slot i of the result is global trial `trial_ids[i]`
        (any order, duplicates allowed, indices up to 2^63 - 1), row for row -- success, wrong, channel_wrong, secret, levels,
        symbols -- what `mc_run_secret` returns for that index on any range that contains it.  trial_ids: as
        QaryDecoder.mc_run_at's.  Returns `mc_run_secret`'s dict with len(trial_ids) rows."""
        ids = _lib.trial_ids(trial_ids)
        return self._secret_host(len(ids), seed, prior, levels, weights, levels_sum, weights_sum, 0, want_secret, want_levels, want_symbols,
                                 trial_ids=ids)

    def mc_run_secret_at_device(self, trial_ids, seed, prior, levels, weights, levels_sum, weights_sum, d_success, d_wrong=0,
                                d_channel_wrong=0, d_secret=0, d_levels=0, d_symbols=0, stream=0):
        """Device-pointer variant of `mc_run_secret_at` (ints; 0 = not wanted); the trial list, prior and tables stay host arrays."""
        ids = _lib.trial_ids(trial_ids)
        outs = [C.c_void_p(d or None) for d in (d_success, d_wrong, d_channel_wrong, d_secret, d_levels, d_symbols)]
        self._secret_call(prior, levels, weights, levels_sum, weights_sum, 0, len(ids), seed, _lib.F_DEVICE_IO, stream, outs, trial_ids=ids)

    def min_sum_soft(self, py_channel_output, py_channel_output_sum, costs=True, margins=True, unmet=True):
        p, ps = np.asarray(py_channel_output), np.asarray(py_channel_output_sum)
        if p.ndim != 2 or ps.ndim != 2:
            raise ValueError("channel outputs must be 2-D")
        return _single(self.min_sum_soft_batch(p[None], ps[None], costs, margins, unmet))


def _single(res):
    """A batch-of-one soft result as `min_sum` returns its symbols: a list of ints, the arrays without the batch axis."""
    out = {k: v[0] for k, v in res.items()}
    out["symbols"] = [int(x) for x in out["symbols"]]
    if "unmet" in out:
        out["unmet"] = int(out["unmet"])
    return out


def into_llr(channel_output):
    """Decoder::into_llr (decoder.rs:668-692) on the device: float32 [rows, Q] probabilities ->
    float32 [rows, Q] LLRs ln(max / p), bit-identical to the host's logf; raises if a row does not
    sum to 1 +- 1e-3."""
    p = np.ascontiguousarray(channel_output, dtype=np.float32)
    if p.ndim != 2:
        raise ValueError("channel output must be 2-D [rows, Q]")
    out = np.empty_like(p)
    lib = _lib.load()
    _lib.check(lib.scaldpc_qary_into_llr(_lib.ptr(p), p.shape[0], p.shape[1], 0, None, _lib.ptr(out)))
    return out


# the enumeration kernels pack one 8-bit digit per edge of a check into a register word: 64 bits in every kernel
# (degree <= 8: all sizes the reference registers), 128 bits in the lane-per-codeword kernel of the plain decoder (<= 16)
MAX_CHECK_DEGREE = 16
MAX_SPECIAL_CHECK_DEGREE = 8
# beyond that, DecoderSpecial runs the min-plus recursion for rows of any length (k_q_special_check_dp_any): alphabets of 3, 5
# and 7 symbols, three LDS tables of 2*B*SW + 1 entries x 64 codewords within 64 KB
DP_ANY_B = (1, 2, 3)
DP_ANY_MAX_ENTRIES = 85


def _check_limits(name, DC, B, BSUM, special=False):
    """The reference generates a class per registered size (lib.rs:32-75: DC = 4, 7, 7, 7) and a name it
    has not registered is an AttributeError on `getattr(simulate_rs, name)` (decode.py:227-229).  Here
    any size resolves -- up to what the kernels are built for; beyond that the name does not resolve
    either, with the reason, at look-up time rather than at the first construction."""
    lim = MAX_SPECIAL_CHECK_DEGREE if special else MAX_CHECK_DEGREE
    if DC > lim:
        raise AttributeError(f"{name}: check degree {DC} > {lim} is not supported by the enumeration kernels "
                             f"(scaldpc_qary.hip; the reference's registered sizes use 4 and 7)")
    if B > 127 or BSUM > 127:
        raise AttributeError(f"{name}: symbols beyond +-127 do not fit the int8 hard decisions (decoder.rs i8)")


_cache = {}


def decoder_class(name: str):
    """Class for a `simulate_rs` decoder name (any size of either pattern)."""
    if name in _cache:
        return _cache[name]
    m = _GENERIC.match(name)
    if m:
        N, R, DV, DC, B = map(int, m.groups())
        _check_limits(name, DC, B, B)
        cls = type(name, (QaryDecoder,), dict(N=N, R=R, DV=DV, DC=DC, B=B, Q=2 * B + 1))
    else:
        m, mb = _SPECIAL.match(name), _SPECIAL_B.match(name)
        if m:
            N, R, SW = map(int, m.groups())
            B = 2  # Kyber eta (lib.rs:54-75: B = 2, BSUM = SW * B)
            _check_limits(name, SW + 1, B, SW * B, special=True)
        elif mb:
            N, R, SW, B = map(int, mb.groups())
            if SW + 1 <= MAX_SPECIAL_CHECK_DEGREE:
                _check_limits(name, SW + 1, B, SW * B, special=True)
            elif B not in DP_ANY_B or 2 * B * SW + 1 > DP_ANY_MAX_ENTRIES:
                raise AttributeError(f"{name}: check degree {SW + 1} > {MAX_SPECIAL_CHECK_DEGREE} runs on the min-plus recursion for rows "
                                     f"of any length, which takes B in {DP_ANY_B} and 2*B*SW + 1 <= {DP_ANY_MAX_ENTRIES} table entries "
                                     f"(here B = {B}, {2 * B * SW + 1} entries)")
        else:
            raise AttributeError(name)
        cls = type(
            name, (QarySpecialDecoder,),
            dict(N=N, R=R, DV=R, DC=SW + 1, B=B, Q=2 * B + 1, BSUM=SW * B, QS=2 * SW * B + 1),
        )  # fmt: skip
    _cache[name] = cls
    return cls
