"""What HQC Monte-Carlo trials with per-check certainties cost, on config 5's geometry (HQC-128, W 50, R 4000, tanh rule, early
exit, max_iter 100, 65 536 trials per call), three routes in one process, warm:

  (a) mc_hqc_run           `mc_hqc_run(eps=0.05)`: one shared error rate, the handle's shared priors
  (b) mc_hqc_run_soft      `mc_hqc_run_soft` with the equivalent K = 2 table: the same trials and the same decode work, so the
                           difference is the generator (one prior plane written per tile) plus the soft path (no fused first
                           iteration, the plane read by every pass and gathered for the compact passes)
  (c) host_soft            the route (b) replaces: `trials.hqc_soft_trials` + `decode_batch(channel_probs=)` on 4096 trials,
                           generation included (one RandomState per trial, inputs and certainties through PCIe)

    python profiles/microbench/hqc_soft_mc_cost.py [--trials 65536] [--reps 5] [--rounds 3] [--host-trials 4096]

(a) and (b) must agree in every success flag and iteration count.  Prints one JSON line: medians of `--rounds` rounds of `--reps`
calls per device route, the routes taken in turn within a round; the host route is timed once per round.  Every call ends in a
stream synchronise."""
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
EPS, SEED = 0.05, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-trials", type=int, default=4096)
    args = ap.parse_args()

    S = importlib.import_module("sca-ldpc_amd")
    bp = importlib.import_module("sca-ldpc_amd.bp")
    trials = importlib.import_module("sca-ldpc_amd.trials")
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "hqc_first_rows.json")))
    H, Hin, _ = S.codes.hqc_bench_graph("hqc128", rows["N17669_W50_s0"])
    N, omega = S.codes.HQC_PARAMS["hqc128"]
    dec = bp.bp_decoder(H, max_iter=100, bp_method="product_sum", channel_probs=trials.hqc_priors(N, H.m, omega, EPS))
    table = dict(weights=np.array([[EPS, 1.0 - EPS]] * 2), flips=np.array([1, 0], dtype=np.uint8), probs=np.array([EPS, EPS]),
                 costs=None)
    levels, weights = (1.0 - EPS,), (1.0,)  # the host generator's law at the same error rate

    def host_soft():
        msg, ys, cert = trials.hqc_soft_trials(Hin, omega, levels, weights, args.host_trials, base_seed=SEED)
        t1 = time.perf_counter()
        d = dec.decode_batch(msg, early_exit=True, channel_probs=(1.0 - cert).astype(np.float32))
        return trials.success(d["bits"], ys, N), time.perf_counter() - t1

    forms = {
        "mc_hqc_run": lambda: dec.mc_hqc_run(args.trials, omega, EPS, seed=SEED),
        "mc_hqc_run_soft": lambda: dec.mc_hqc_run_soft(args.trials, omega, table, seed=SEED),
    }
    out = {k: f() for k, f in forms.items()}  # warm: workspaces, code objects
    for k in ("success", "iters"):
        assert np.array_equal(out["mc_hqc_run"][k], out["mc_hqc_run_soft"][k]), k
    stats = dec.last_stats()
    host_soft()
    ms = {k: [] for k in forms}
    host_ms, host_decode_ms = [], []
    for _ in range(args.rounds):
        for k, f in forms.items():
            t0 = time.perf_counter()
            for _ in range(args.reps):
                f()  # (each call ends in a stream synchronise)
            ms[k].append((time.perf_counter() - t0) / args.reps * 1e3)
        t0 = time.perf_counter()
        ok, decode_s = host_soft()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        host_decode_ms.append(decode_s * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    hm = statistics.median(host_ms)
    print(json.dumps({
        "graph": "hqc128 N17669_W50_s0 R4000", "rule": "product_sum", "max_iter": 100, "early_exit": True, "eps": EPS,
        "trials_per_call": args.trials, "reps": args.reps, "rounds": args.rounds,
        "ms_per_call": {k: round(v, 3) for k, v in med.items()},
        "ms_spread": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
        "trials_per_s": {k: round(args.trials / v * 1e3) for k, v in med.items()},
        "soft_over_plain": round(med["mc_hqc_run_soft"] / med["mc_hqc_run"], 4),
        "host_soft": {"trials": args.host_trials, "ms": round(hm, 1), "ms_decode_only": round(statistics.median(host_decode_ms), 1),
                      "trials_per_s": round(args.host_trials / hm * 1e3), "success_rate": round(float(ok.mean()), 4)},
        "success_rate": round(float(out["mc_hqc_run_soft"]["success"].mean()), 4),
        "mean_iters": round(float(out["mc_hqc_run_soft"]["iters"].mean()), 3), "compacted_soft": stats["compacted"],
    }), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
