"""Seeded random call sequences on ONE live `BpDecoder` (tests/handle_sequence_cases.py), one test per sequence.

After every decode of a sequence the result is held
  * to the oracle on the model's current graph and priors: min-sum bit for bit (`_exact` of tests/test_production_range_gpu.py);
    the tanh rule in float32 under `helpers.compare` with the tolerance the oracle's own sensitivity gives (`_own_sensitivity`
    of tests/test_bp_property_gpu.py, max_iter capped as there); float64 at the bar of tests/ref64_cases.py -- no tolerance of
    this file's own;
  * to a FRESH decoder on the model's current graph, priors and knobs, bit for bit, whatever the method and precision
    (`_same` of tests/test_append_gpu.py): history must be invisible.  The fresh decoder is code under test; it never stands
    in for the oracle.
Sweeps are held to the trial law (tests/mc_ref.py) and to the oracle on their exported inputs.  The last test (definition
order) asks that the device itself reported the paths the sequences claim to reach.  tests/test_handle_sequences.py shows,
without a GPU, that the sequences decide something and contain every transition."""
import importlib

import numpy as np
import pytest

import handle_sequence_cases as C
import mc_ref
from helpers import compare
from oracle import pyoracle
from ref64_cases import hold_to_bar
from test_append_gpu import _same
from test_bp_property_gpu import _own_sensitivity
from test_production_range_gpu import _exact

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")
lib = importlib.import_module("sca-ldpc_amd._lib")
LIVE = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes")
KIND = {"syndrome": lib.IN_SYNDROME, "received": lib.IN_RECEIVED}
METHOD = {"min_sum": lib.BP_MIN_SUM, "product_sum": lib.BP_PRODUCT_SUM}
SEEN = {"record_form": 0, "message_form": 0, "row_parallel": 0, "compacted": 0, "horizon_saved": 0, "rerun": 0}
COMPARED = {}  # (method, precision) -> decodes compared with the oracle and with a fresh decoder


@pytest.fixture(autouse=True)
def own_knobs(monkeypatch):
    """Every knob at the library's default unless a sequence sets it."""
    for v in ("SCALDPC_PATH", "SCALDPC_SPLIT", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_COMPACT_AFTER", "SCALDPC_FIRST_FUSED",
              "SCALDPC_FUSE_TEST", "SCALDPC_MINSUM_REC", "SCALDPC_PRECISION", "SCALDPC_SETTLE", "SCALDPC_SETTLE_HORIZON"):
        monkeypatch.delenv(v, raising=False)


class Handle:
    """`BpDecoder` behind the surface `replay` drives.  A Python decoder has one method; a call of the other one goes through
    the same handle and the same C entry points with that call's method and alpha (as tests/test_ref64_gpu.py's min_sum())."""

    def __init__(self, graph, probs, knobs, watch=False):
        with np.errstate(divide="ignore"):
            self.dec = bp.bp_decoder(graph, max_iter=30, bp_method="min_sum", channel_probs=probs)
        self.watch = watch
        self.configure(knobs)

    def _as(self, method, alpha):
        self.dec._method, self.dec.ms_scaling_factor = METHOD[method], float(alpha)

    def configure(self, knobs):
        for k, v in knobs.items():
            if k == "tile_group":
                self.dec.set_tile_group(v)
            else:
                self.dec.configure(**{k: v})

    def update_channel_probs(self, probs):
        with np.errstate(divide="ignore"):
            self.dec.update_channel_probs(probs)

    def append_rows(self, rp, ci, new_n, tail):
        self.dec.append_rows(rp, ci, new_n, tail)

    def decode(self, x, kind, cp, max_iter, early, want_llr, method, alpha, precision, io):
        self._as(method, alpha)
        dec = self.dec
        if io == "host":
            with np.errstate(divide="ignore"):
                got = dec.decode_batch(x, max_iter=max_iter, early_exit=early, want_llr=want_llr, input_vector_type=kind,
                                       channel_probs=cp, precision=precision)
        else:
            import torch

            f64 = precision == "float64"
            batch = x.shape[0]
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                d_in = torch.from_numpy(x).cuda()
                d_cp = None if cp is None else torch.from_numpy(cp.astype(np.float64) if f64 else cp).cuda()
                d_bits = torch.zeros((batch, dec.n), dtype=torch.uint8, device="cuda")
                d_llr = torch.zeros((batch, dec.n), dtype=torch.float64 if f64 else torch.float32, device="cuda") if want_llr else None
                d_iters = torch.zeros(batch, dtype=torch.int32, device="cuda")
                d_conv = torch.zeros(batch, dtype=torch.uint8, device="cuda")
            stream.synchronize()  # (the inputs are in place before the library's own stream order begins)
            dec.decode_batch_device(d_in.data_ptr(), KIND[kind], batch, d_bits.data_ptr(), max_iter=max_iter, early_exit=early,
                                    stream=stream.cuda_stream, d_out_llr=d_llr.data_ptr() if want_llr else 0,
                                    d_out_iters=d_iters.data_ptr(), d_out_conv=d_conv.data_ptr(), asynchronous=io == "async",
                                    d_channel_probs=0 if cp is None else d_cp.data_ptr(), prob_cols=0 if cp is None else cp.shape[1],
                                    precision=precision)
            stream.synchronize()  # an asynchronous call is synchronised before anything is compared
            got = {"bits": d_bits.cpu().numpy(), "llr": d_llr.cpu().numpy() if want_llr else None, "iters": d_iters.cpu().numpy(),
                   "converged": d_conv.cpu().numpy()}
        if self.watch and precision == "float32":
            st, settle = dec.last_stats(), dec.last_settle()
            SEEN["row_parallel"] += st["row_parallel"] > 0
            SEEN["compacted"] += dec.last_compacted() > 0
            SEEN["horizon_saved"] += settle["horizon"] > 0 and settle["launches_saved"] > 0
            SEEN["rerun"] += settle["tiles_rerun"] >= 1
        return got

    def sweep(self, kind, runs, seed, first, max_iter, early, alpha, omega, eps):
        self._as("min_sum", alpha)
        if kind == "fer":
            return self.dec.mc_fer_run(runs, seed, first_trial=first, max_iter=max_iter, early_exit=early, want_errors=True)
        return self.dec.mc_hqc_run(runs, omega, eps, seed, first_trial=first, max_iter=max_iter, early_exit=early, want_inputs=True)

    def probe(self, can_time):
        """Between two decodes: must change nothing.  time_kernels re-runs the last TILE decode's kernels, so it is asked only
        right after one."""
        if can_time:
            form = self.dec.time_kernels(2)["record_form"]
            if self.watch:
                SEEN["record_form" if form else "message_form"] += 1
        self.dec.last_schedule(), self.dec.last_settle(), self.dec.last_stats()
        lib.trim()

    def refused(self, x, kind, cp, max_iter):
        self._as("min_sum", 1.0)
        b, n = x.shape[0], self.dec.n
        out = {"bits": np.full((b, n), C.SENTINEL["bits"], np.uint8), "llr": np.full((b, n), C.SENTINEL["llr"], np.float32),
               "iters": np.full(b, C.SENTINEL["iters"], np.int32), "converged": np.full(b, C.SENTINEL["converged"], np.uint8)}
        rc = self.dec._lib.scaldpc_bp_decode_batch_soft(
            self.dec._h, lib.ptr(x), KIND[kind], b, lib.ptr(cp), cp.shape[1], max_iter, lib.BP_MIN_SUM, 1.0, lib.F_EARLY_EXIT, None,
            lib.ptr(out["bits"]), lib.ptr(out["llr"]), lib.ptr(out["iters"]), lib.ptr(out["converged"]))
        try:
            lib.check(rc)
            out["raised"] = None
        except Exception as e:  # noqa: BLE001
            out["raised"] = type(e)
        return out

    def close(self):
        self.dec.close()


def _hold_decode(step, model, a, got, live):
    g, probs, k = model.graph(), model.probs, KIND[a["kind"]]
    method, precision, x, cp = a["method"], a["precision"], a["x"], a["cp"]
    ref = C.oracle_decode(g, probs, cp, x, k, a["max_iter"], method, a["alpha"], precision, a["early"], threads=8)
    what = (step, method, precision)
    if precision == "float64":
        hold_to_bar(got, ref)
    elif method == "min_sum":
        _exact(got if got["llr"] is not None else dict(got, llr=ref["llr"]), ref, what)
    else:
        tol = 2e-4
        rows = [(probs, x, ref)] if cp is None else [(p, x[b : b + 1], {key: v[b : b + 1] for key, v in ref.items()})
                                                       for b, p in enumerate(C.full_priors(probs, cp))]
        for p, xb, rb in rows:  # (per-codeword priors: the oracle's sensitivity codeword by codeword, the largest counts)
            tol = max(tol, _own_sensitivity(pyoracle, g, p, xb, k, a["max_iter"], method, a["early"], rb)[0])
        compare(got, ref, method, widened_tol=tol, tie_codewords=1 + x.shape[0] // 64)
    # ... and a decoder without history
    fresh = Handle(g, probs.copy(), dict(model.explicit))
    try:
        again = fresh.decode(**a)
    finally:
        fresh.close()
    _same(got if got["llr"] is not None else dict(got, llr=np.zeros(0)), again if again["llr"] is not None else dict(again, llr=np.zeros(0)), what)
    COMPARED[(method, precision)] = COMPARED.get((method, precision), 0) + 1


def _hold_sweep(step, model, a, got, live):
    g = model.graph()
    with np.errstate(divide="ignore", invalid="ignore"):
        if a["kind"] == "fer":
            err, synd = mc_ref.fer(a["seed"], a["first"], a["runs"], g, model.probs)
            assert np.array_equal(got["errors"], err), "the sweep's errors are not the law's on the current priors"
            d = C.oracle_decode(g, model.probs, None, synd, 0, a["max_iter"], "min_sum", a["alpha"], "float32", a["early"], threads=8)
            success = (d["bits"] == err).all(axis=1).astype(np.uint8)
        else:
            y, msg = mc_ref.hqc(a["seed"], a["first"], a["runs"], model.hin(), a["omega"], a["eps"])
            assert np.array_equal(got["y"], y) and np.array_equal(got["msg"], msg), "the sweep's trials are not the law's on the current graph"
            d = C.oracle_decode(g, model.probs, None, msg, 1, a["max_iter"], "min_sum", a["alpha"], "float32", a["early"], threads=8)
            success = mc_ref.hqc_success(d["bits"], y, model.N)
    assert np.array_equal(got["iters"], d["iters"]), "sweep: iteration counts"
    assert np.array_equal(got["success"], success), "sweep: success flags"


@pytest.mark.parametrize("family,seed", C.SEQUENCES)
def test_sequence(oracle, family, seed):
    base = tuple(lib.live_blocks()[k] for k in LIVE)
    C.replay(C.sequence(family, seed), lambda g, p, kn: Handle(g, p, kn, watch=True), on_decode=_hold_decode, on_sweep=_hold_sweep)
    assert tuple(lib.live_blocks()[k] for k in LIVE) == base, "a block is still live after the sequence's handles were closed"


def test_the_sequences_reached_the_paths_they_claim():
    """Runs after the sequences (definition order): over the whole run the DEVICE reported the record form and the message
    form (time_kernels), the row-parallel kernels, a compact pass, a call under a learned or forced horizon that saved
    launches, and a tile decoded again because its horizon was too short."""
    print("decodes compared, by method and precision:", dict(sorted(COMPARED.items())), "reached:", SEEN)
    assert all(v > 0 for v in SEEN.values()), SEEN
