"""What a Monte-Carlo sweep in the reference's own arithmetic costs on the device, and on how many trials it decides otherwise
than the fp32 sweep.  BASELINE config 5's geometry: the HQC-128 bench graph (W 50, R 4000: 204 000 edges), 65 536 trials per
call, max_iter 100, early exit, eps = 0.05; ONE handle in ONE process, warm, the routes taken in turn:

  float64_flat     mc_hqc_run(precision="float64") with compact_after = 0: every tile group runs to its end
  float64          the same with the default compact_after: one hand-over of the stragglers to dense tiles
  float32          mc_hqc_run, the fp32 tanh kernels (the sweep bench.py times)
  host_route       what the float64 sweep replaces: the fp32 sweep with want_inputs (the trials cross PCIe), then
                   decode_batch(precision="float64") on them (and back again), no hand-over

    python profiles/microbench/ref64_sweep_cost.py [--trials 65536] [--rounds 3] [--audit-chunk 16384]

Prints one JSON line: per route the median over `--rounds` rounds of one call each (every call ends in a stream synchronise),
the spread of the rounds (max - min), trials per second, and `last_compacted()` after the route's call (float64: the one
hand-over; float32: what the fp32 scheduler handed down from its first level); then `driver.hqc_precision_audit` on the
same trial indices at eps = 0.05 (the two-outcome table) and under the wrapped oracle's table t9 =
wrapped_oracle_table((0.98, 0.9), (0.999, 0.99)): the trials on which fp32 and float64 differ in success and in iteration
count."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
EPS, SEED, MAX_ITER = 0.05, 2, 100
ROUTES = ("float64_flat", "float64", "float32", "host_route")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--audit-chunk", type=int, default=16384)
    ap.add_argument("--skip-host-route", action="store_true")
    args = ap.parse_args()

    S = importlib.import_module("sca-ldpc_amd")
    bp = importlib.import_module("sca-ldpc_amd.bp")
    driver = importlib.import_module("sca-ldpc_amd.driver")
    trials = importlib.import_module("sca-ldpc_amd.trials")
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "hqc_first_rows.json")))
    H, Hin, _ = S.codes.hqc_bench_graph("hqc128", rows["N17669_W50_s0"])
    N, omega = S.codes.HQC_PARAMS["hqc128"]
    dec = bp.bp_decoder(H, max_iter=MAX_ITER, bp_method="product_sum", channel_probs=trials.hqc_priors(N, H.m, omega, EPS))
    nb = args.trials
    routes = tuple(r for r in ROUTES if not (args.skip_host_route and r == "host_route"))
    handed = {}

    def call(route):
        if route == "host_route":
            r = dec.mc_hqc_run(nb, omega, EPS, SEED, want_inputs=True)
            d = dec.decode_batch(r["msg"], early_exit=True, precision="float64")
            yv = np.zeros((nb, N), dtype=np.uint8)
            np.put_along_axis(yv, r["y"].astype(np.int64), 1, axis=1)
            return {"success": (d["bits"][:, :N] == yv).all(axis=1).astype(np.uint8), "iters": d["iters"]}
        dec.configure(compact_after=0 if route == "float64_flat" else -1)
        r = dec.mc_hqc_run(nb, omega, EPS, SEED, precision="float32" if route == "float32" else "float64")
        handed[route] = dec.last_compacted()
        dec.configure(compact_after=-1)
        return r

    first = {p: call(p) for p in routes}  # warm: workspaces, code objects
    for p in routes:  # the three float64 routes are one computation
        if p != "float32":
            assert np.array_equal(first[p]["success"], first["float64"]["success"]) and np.array_equal(first[p]["iters"], first["float64"]["iters"]), p
    ms = {p: [] for p in routes}
    for _ in range(args.rounds):
        for p in routes:
            t0 = time.perf_counter()
            call(p)
            ms[p].append((time.perf_counter() - t0) * 1e3)
    med = {p: statistics.median(v) for p, v in ms.items()}
    res = {"graph": "hqc128 N17669_W50_s0 R%d" % H.m, "edges": int(H.nnz), "rule": "product_sum", "max_iter": MAX_ITER, "early_exit": True,
           "eps": EPS, "trials_per_call": nb, "rounds": args.rounds,
           "ms_per_call": {p: round(v, 1) for p, v in med.items()},
           "ms_spread": {p: round(max(v) - min(v), 1) for p, v in ms.items()},
           "ms_rounds": {p: [round(x, 1) for x in v] for p, v in ms.items()},
           "trials_per_s": {p: float("%.4g" % (nb / (v * 1e-3))) for p, v in med.items()},
           "handed_over": handed,
           "successes": {p: int(first[p]["success"].sum()) for p in routes},
           "default_over_flat": round(med["float64"] / med["float64_flat"], 3),
           "float64_over_float32": round(med["float64"] / med["float32"], 3)}
    if "host_route" in med:
        res["host_route_over_float64"] = round(med["host_route"] / med["float64"], 3)
    dec.close()
    # the audit: the same trial indices through both precisions
    tables = {"eps_0.05": dict(weights=np.array([[EPS, 1.0 - EPS]] * 2), flips=np.array([1, 0], dtype=np.uint8), probs=np.array([EPS, EPS]),
                               costs=None),
              "t9": trials.wrapped_oracle_table((0.98, 0.9), (0.999, 0.99))}
    res["audit"] = {}
    for name, table in tables.items():
        t0 = time.perf_counter()
        a = driver.hqc_precision_audit(Hin, N, omega, table, nb, SEED, chunk=args.audit_chunk, max_iter=MAX_ITER)
        res["audit"][name] = {"runs": a["runs"], "successes32": a["successes32"], "successes64": a["successes64"],
                              "success_differs": int(a["success_differs"].size), "success_differs_first": a["success_differs"][:16].tolist(),
                              "iters_differ": a["iters_differ"], "seconds": round(time.perf_counter() - t0, 1)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
