"""Test doubles: decoder classes with the product's Python surface, backed by the CPU
oracle, so that the HOST logic (drivers, sharding) can run in `-m "not gpu"` tests.
Never used by the product."""
import numpy as np

from helpers import S
from oracle import pyoracle


class OracleBp:
    def __init__(self, H, error_rate=None, max_iter=0, bp_method=0, ms_scaling_factor=1.0, channel_probs=[None],
                 input_vector_type=-1, dtype="f64"):
        self.g = S.TannerGraph.coerce(H)
        self.n, self.m = self.g.n, self.g.m
        self.max_iter = max_iter or self.n
        self.method = {"product_sum": "product_sum", "min_sum": "min_sum"}[bp_method]
        self.alpha = ms_scaling_factor
        cp = list(channel_probs)
        self.probs = np.asarray(cp, dtype=np.float64) if cp and cp[0] is not None else np.full(self.n, float(error_rate))
        self.dtype = dtype

    def decode_batch(self, inputs, max_iter=None, early_exit=True, want_llr=False, input_vector_type=None):
        x = np.asarray(inputs, dtype=np.uint8)
        kind = {"syndrome": 0, "received_vector": 1, None: 0 if x.shape[1] == self.m else 1}[input_vector_type]
        return pyoracle.bp_decode_batch(self.g, self.probs, x, kind, max_iter or self.max_iter, self.method,
                                        alpha=self.alpha, dtype=self.dtype, threads=4, early_exit=early_exit)


def oracle_qary_class(name):
    import re

    N, R, V, C, B = map(int, re.match(r"DecoderN(\d+)R(\d+)V(\d+)C(\d+)B(\d+)", name).groups())

    class _D:
        def __init__(self, H, iterations):
            self.g = S.TannerGraph.from_dense(np.asarray(H))
            self.it = iterations

        def min_sum_batch(self, pmf):
            return pyoracle.qary_min_sum_batch(self.g, 2 * B + 1, pmf, self.it, threads=4)

    return _D


class OracleLiveBp:
    """One LIVE binary decoder as tests/handle_sequence_cases.replay drives it -- decodes of any method, precision and prior
    source, knobs, prior updates, appended rows, sweeps, probes, refused calls -- answered by the CPU oracle.  It keeps its own
    CSR arrays and priors, put together from the calls it receives."""

    def __init__(self, graph, probs, knobs):
        self.m, self.n = graph.m, graph.n
        self.row_ptr = np.asarray(graph.row_ptr, dtype=np.int64).copy()
        self.col_idx = np.asarray(graph.col_idx, dtype=np.int32).copy()
        self.probs = np.asarray(probs, dtype=np.float64).copy()
        self.knobs = dict(knobs)
        self.closed = False

    def graph(self):
        return S.TannerGraph.from_csr(self.m, self.n, self.row_ptr, self.col_idx)

    def decode(self, x, kind, cp, max_iter, early, want_llr, method, alpha, precision, io):
        import handle_sequence_cases as cases

        r = cases.oracle_decode(self.graph(), self.probs, cp, x, 0 if kind == "syndrome" else 1, max_iter, method, alpha, precision,
                                early)
        return {"bits": r["bits"], "llr": r["llr"] if want_llr else None, "iters": r["iters"],
                "converged": r["converged"].astype(np.uint8)}

    def configure(self, knobs):
        self.knobs.update(knobs)

    def update_channel_probs(self, probs):
        assert probs.shape == (self.n,)
        self.probs = np.asarray(probs, dtype=np.float64).copy()

    def append_rows(self, row_ptr, col_idx, new_n, tail):
        assert row_ptr[0] == 0 and len(col_idx) == row_ptr[-1] and len(tail) == new_n - self.n and (np.asarray(col_idx) < new_n).all()
        self.row_ptr = np.concatenate([self.row_ptr, self.row_ptr[-1] + np.asarray(row_ptr[1:], dtype=np.int64)])
        self.col_idx = np.concatenate([self.col_idx, np.asarray(col_idx, dtype=np.int32)])
        self.probs = np.concatenate([self.probs, np.asarray(tail, dtype=np.float64)])
        self.m += len(row_ptr) - 1
        self.n = new_n

    def sweep(self, kind, runs, seed, first, max_iter, early, alpha, omega, eps):
        import mc_ref

        g = self.graph()
        if kind == "fer":
            err, synd = mc_ref.fer(seed, first, runs, g, self.probs)
            d = pyoracle.bp_decode_batch(g, self.probs, synd, 0, max_iter, "min_sum", alpha=alpha, dtype="f32", threads=4, early_exit=early)
            return {"success": (d["bits"] == err).all(axis=1).astype(np.uint8), "iters": d["iters"], "errors": err}
        N = self.n - self.m
        keep = np.ones(len(self.col_idx), dtype=bool)
        keep[self.row_ptr[1:] - 1] = False  # Hin: every row without its identity column
        hin = S.TannerGraph.from_csr(self.m, N, self.row_ptr - np.arange(self.m + 1), self.col_idx[keep])
        y, msg = mc_ref.hqc(seed, first, runs, hin, omega, eps)
        d = pyoracle.bp_decode_batch(g, self.probs, msg, 1, max_iter, "min_sum", alpha=alpha, dtype="f32", threads=4, early_exit=early)
        return {"success": mc_ref.hqc_success(d["bits"], y, N), "iters": d["iters"], "msg": msg, "y": y}

    def probe(self, can_time):
        pass

    def refused(self, x, kind, cp, max_iter):
        import handle_sequence_cases as cases

        bad = not bool(((cp >= 0.0) & (cp <= 1.0)).all())
        b = x.shape[0]
        return {"raised": ValueError if bad else None, "bits": np.full((b, self.n), cases.SENTINEL["bits"], np.uint8),
                "llr": np.full((b, self.n), cases.SENTINEL["llr"], np.float32), "iters": np.full(b, cases.SENTINEL["iters"], np.int32),
                "converged": np.full(b, cases.SENTINEL["converged"], np.uint8)}

    def close(self):
        self.closed = True
