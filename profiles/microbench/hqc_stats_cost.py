"""What the attack's decoder statistics cost per trial of an HQC sweep, on config 5's geometry (HQC-128, W 50, R 4000, tanh rule,
early exit, max_iter 100, 65 536 trials per call), in one process, warm:

  (a) mc_hqc_run_soft        the plain sweep, which must cost what it cost before scaldpc_mc_hqc_run_stats existed: held against
                             the figure of profiles/hqc_soft_mc/hqc_soft_mc_cost_mi355x.txt, the margin being that file's own
                             run-to-run spread for the route
  (b) stats / stats_bits     `mc_hqc_run_soft(want_stats=True)` without and with `want_bits`: the same trials and the same decode,
                             plus k_mc_hqc_stats over three bit planes (and, with bits, a [trials, n] byte array through PCIe)
  (c) host_stats             the route (b) replaces, on 4096 trials: the sweep with `want_inputs`, `decode_batch(channel_probs=)`
                             on the exported inputs, `driver.hqc_stats` per trial

    python profiles/microbench/hqc_stats_cost.py [--trials 65536] [--reps 5] [--rounds 3] [--host-trials 4096]

(a) and (b) must agree in every success flag and iteration count, and (c) in every counter of its trials.  Prints one JSON line:
medians of `--rounds` rounds of `--reps` calls per device route, the routes taken in turn within a round; the host route is timed
once per round.  Every call ends in a stream synchronise."""
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
PARENT = os.path.join(ROOT, "profiles", "hqc_soft_mc", "hqc_soft_mc_cost_mi355x.txt")


def parent_figure():
    """(ms per call, spread) of mc_hqc_run_soft as measured before this entry existed."""
    line = [ln for ln in open(PARENT) if ln.startswith("{")][-1]
    d = json.loads(line)
    return d["ms_per_call"]["mc_hqc_run_soft"], d["ms_spread"]["mc_hqc_run_soft"], d["trials_per_call"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-trials", type=int, default=4096)
    args = ap.parse_args()

    S = importlib.import_module("sca-ldpc_amd")
    bp = importlib.import_module("sca-ldpc_amd.bp")
    driver = importlib.import_module("sca-ldpc_amd.driver")
    trials = importlib.import_module("sca-ldpc_amd.trials")
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "hqc_first_rows.json")))
    H, Hin, _ = S.codes.hqc_bench_graph("hqc128", rows["N17669_W50_s0"])
    N, omega = S.codes.HQC_PARAMS["hqc128"]
    dec = bp.bp_decoder(H, max_iter=100, bp_method="product_sum", channel_probs=trials.hqc_priors(N, H.m, omega, EPS))
    table = dict(weights=np.array([[EPS, 1.0 - EPS]] * 2), flips=np.array([1, 0], dtype=np.uint8), probs=np.array([EPS, EPS]),
                 costs=None)
    probs = table["probs"].astype(np.float32)

    def host_stats():
        r = dec.mc_hqc_run_soft(args.host_trials, omega, table, seed=SEED, want_inputs=True)
        d = dec.decode_batch(r["msg"], early_exit=True, channel_probs=probs[r["outcome"]])
        rows = [driver.hqc_stats(N, d["bits"][i], r["msg"][i, N:], r["y"][i]) for i in range(args.host_trials)]
        return np.array([[st[c] for c in bp.HQC_STATS_COLUMNS] for _, st in rows]), np.array([ok for ok, _ in rows])

    forms = {
        "mc_hqc_run_soft": lambda: dec.mc_hqc_run_soft(args.trials, omega, table, seed=SEED),
        "stats": lambda: dec.mc_hqc_run_soft(args.trials, omega, table, seed=SEED, want_stats=True),
        "stats_bits": lambda: dec.mc_hqc_run_soft(args.trials, omega, table, seed=SEED, want_stats=True, want_bits=True),
    }
    out = {k: f() for k, f in forms.items()}  # warm: workspaces, code objects
    for k in ("success", "iters", "flips"):
        assert np.array_equal(out["mc_hqc_run_soft"][k], out["stats"][k]) and np.array_equal(out["stats"][k], out["stats_bits"][k]), k
    assert np.array_equal(out["stats"]["stats"], out["stats_bits"]["stats"])
    compacted = dec.last_stats()["compacted"]
    host, host_ok = host_stats()
    k = min(args.host_trials, args.trials)
    assert np.array_equal(host[:k], out["stats"]["stats"][:k]) and np.array_equal(host_ok[:k], out["stats"]["success"][:k].astype(bool))
    sums = out["stats"]["stats"].sum(axis=0, dtype=np.int64)
    del out["stats_bits"]
    ms = {k: [] for k in forms}
    host_ms = []
    for _ in range(args.rounds):
        for k, f in forms.items():
            t0 = time.perf_counter()
            for _ in range(args.reps):
                f()  # (each call ends in a stream synchronise)
            ms[k].append((time.perf_counter() - t0) / args.reps * 1e3)
        t0 = time.perf_counter()
        host_stats()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    hm = statistics.median(host_ms)
    was, spread, was_trials = parent_figure()
    res = {
        "graph": "hqc128 N17669_W50_s0 R4000", "rule": "product_sum", "max_iter": 100, "early_exit": True, "eps": EPS,
        "trials_per_call": args.trials, "reps": args.reps, "rounds": args.rounds,
        "ms_per_call": {k: round(v, 3) for k, v in med.items()},
        "ms_spread": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
        "trials_per_s": {k: round(args.trials / v * 1e3) for k, v in med.items()},
        "stats_over_plain": round(med["stats"] / med["mc_hqc_run_soft"], 4),
        "stats_bits_over_plain": round(med["stats_bits"] / med["mc_hqc_run_soft"], 4),
        "host_stats": {"trials": args.host_trials, "ms": round(hm, 1), "trials_per_s": round(args.host_trials / hm * 1e3)},
        "success_rate": round(float(out["stats"]["success"].mean()), 4), "compacted": compacted,
        "counter_sums": dict(zip(bp.HQC_STATS_COLUMNS, (int(v) for v in sums))),
    }
    if args.trials == was_trials:
        res["plain_before"] = {"ms_per_call": was, "ms_spread": spread, "ms_now_minus_before": round(med["mc_hqc_run_soft"] - was, 3),
                               "within_spread": bool(med["mc_hqc_run_soft"] <= was + spread)}
    print(json.dumps(res), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
