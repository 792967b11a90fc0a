"""What Monte-Carlo sweeps on chosen trials cost, on config 5's geometry (HQC-128, W 50, R 4000, tanh rule, early exit, max_iter
100, 65 536 trials per call), warm:

  (a) list against range   `mc_hqc_run_soft` against `mc_hqc_run_soft_at` with the identity list (the same trials: the results
                           must be identical), routes alternating in one process -- the difference is the list's upload (512 KB)
                           and its loads in the two generator kernels
  (b) this build against   the plain `mc_hqc_run` of this checkout against another, built one (`--parent-root`: a checkout of the
      the parent's         parent commit with its libscaldpc.so), alternating CHILD processes (a process binds one library and
                           one package), each warm, the same call -- the evidence that the contiguous entries did not slow
                           down; the margin is the parent's own run-to-run spread, printed next to the numbers
  (c) the retiring curve   `driver.hqc_attack_curve` against `driver.hqc_attack_curve_retiring` on one curve: the graph's first
                           `--curve-checks` rows, `--decode-every` at a time, `--curve-runs` keys, the table
                           trials.wrapped_oracle_table((0.98, 0.9), (0.999, 0.99)); the time of each and the `decoded` column

    python profiles/microbench/mc_trial_list_cost.py [--trials 65536] [--reps 5] [--rounds 3] [--parent-root DIR] [--pairs 3]
           [--curve-runs 4096] [--curve-checks 4000] [--decode-every 500]

Prints one JSON line per part.  Every call ends in a stream synchronise."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--root" in sys.argv:  # (a child of part (b): the checkout whose package and library it measures)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
EPS, SEED = 0.05, 2


def setup():
    S = importlib.import_module("sca-ldpc_amd")
    bp = importlib.import_module("sca-ldpc_amd.bp")
    trials = importlib.import_module("sca-ldpc_amd.trials")
    first_rows = json.load(open(os.path.join(ROOT, "tests", "golden", "hqc_first_rows.json")))
    sup = first_rows["N17669_W50_s0"]
    H, Hin, rows = S.codes.hqc_bench_graph("hqc128", sup)
    N, omega = S.codes.HQC_PARAMS["hqc128"]
    return S, bp, trials, sup, H, rows, N, omega


def timed(forms, reps, rounds):
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                f()  # (each call ends in a stream synchronise)
            ms[k].append((time.perf_counter() - t0) / reps * 1e3)
    return ms


def child_plain(args):
    """(b), one process: the plain mc_hqc_run of the checkout `--root` names, warm."""
    S, bp, trials, sup, H, rows, N, omega = setup()
    dec = bp.bp_decoder(H, max_iter=100, bp_method="product_sum", channel_probs=trials.hqc_priors(N, H.m, omega, EPS))
    out = dec.mc_hqc_run(args.trials, omega, EPS, seed=SEED)
    ms = timed({"mc_hqc_run": lambda: dec.mc_hqc_run(args.trials, omega, EPS, seed=SEED)}, args.reps, args.rounds)["mc_hqc_run"]
    print(json.dumps({"child": True, "ms": ms, "successes": int(out["success"].sum()), "iters": int(out["iters"].sum())}), flush=True)
    dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--curve-runs", type=int, default=4096)
    ap.add_argument("--curve-checks", type=int, default=4000)
    ap.add_argument("--decode-every", type=int, default=500)
    ap.add_argument("--child-plain", action="store_true")
    args = ap.parse_args()
    if args.child_plain:
        return child_plain(args)

    # ---- (b) first: child processes, before this one opens the device
    if args.parent_root:
        runs = {"parent": [], "this": []}
        sums = set()
        for _ in range(args.pairs):
            for which, root in (("parent", args.parent_root), ("this", ROOT)):
                env = dict(os.environ)
                env.pop("SCALDPC_SO", None)
                cmd = [sys.executable, os.path.abspath(__file__), "--child-plain", "--root", os.path.abspath(root), "--trials", str(args.trials),
                       "--reps", str(args.reps), "--rounds", str(args.rounds)]
                done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                if done.returncode:
                    sys.exit(f"the child on {root} failed ({done.returncode}):\n{done.stderr[-2000:]}")
                lines = done.stdout.splitlines()
                got = json.loads([ln for ln in lines if ln.startswith("{")][-1])
                runs[which] += got["ms"]
                sums.add((got["successes"], got["iters"]))
        assert len(sums) == 1, sums  # both builds decode the same trials to the same end
        med = {k: statistics.median(v) for k, v in runs.items()}
        print(json.dumps({
            "part": "b", "what": "mc_hqc_run, this build against the parent's, alternating processes", "trials_per_call": args.trials,
            "processes_each": args.pairs, "rounds_per_process": args.rounds, "reps": args.reps,
            "ms_per_call_median": {k: round(v, 3) for k, v in med.items()},
            "ms_per_call_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in runs.items()},
            "ms_spread": {k: round(max(v) - min(v), 3) for k, v in runs.items()},
            "this_over_parent": round(med["this"] / med["parent"], 4),
            "within_the_parents_spread": bool(med["this"] - med["parent"] <= max(runs["parent"]) - min(runs["parent"])),
        }), flush=True)

    S, bp, trials, sup, H, rows, N, omega = setup()
    driver = importlib.import_module("sca-ldpc_amd.driver")
    # ---- (a) the identity list against the range
    dec = bp.bp_decoder(H, max_iter=100, bp_method="product_sum", channel_probs=trials.hqc_priors(N, H.m, omega, EPS))
    table = dict(weights=np.array([[EPS, 1.0 - EPS]] * 2), flips=np.array([1, 0], dtype=np.uint8), probs=np.array([EPS, EPS]), costs=None)
    ids = np.arange(args.trials, dtype=np.int64)
    forms = {
        "mc_hqc_run_soft": lambda: dec.mc_hqc_run_soft(args.trials, omega, table, seed=SEED),
        "mc_hqc_run_soft_at": lambda: dec.mc_hqc_run_soft_at(ids, omega, table, seed=SEED),
    }
    out = {k: f() for k, f in forms.items()}  # warm: workspaces, code objects
    for k in ("success", "iters", "flips"):
        assert np.array_equal(out["mc_hqc_run_soft"][k], out["mc_hqc_run_soft_at"][k]), k
    ms = timed(forms, args.reps, args.rounds)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "part": "a", "graph": "hqc128 N17669_W50_s0 R4000", "rule": "product_sum", "max_iter": 100, "early_exit": True, "eps": EPS,
        "trials_per_call": args.trials, "reps": args.reps, "rounds": args.rounds, "list": "identity, int64, %d bytes" % ids.nbytes,
        "ms_per_call": {k: round(v, 3) for k, v in med.items()}, "ms_spread": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
        "list_minus_range_ms": round(med["mc_hqc_run_soft_at"] - med["mc_hqc_run_soft"], 3),
        "list_over_range": round(med["mc_hqc_run_soft_at"] / med["mc_hqc_run_soft"], 4), "results_identical": True,
        "success_rate": round(float(out["mc_hqc_run_soft_at"]["success"].mean()), 4),
    }), flush=True)
    dec.close()

    # ---- (c) the curve, retiring against not
    t9 = trials.wrapped_oracle_table((0.98, 0.9), (0.999, 0.99))
    how = dict(max_checks=args.curve_checks, chunk=4096, bp_method="product_sum", max_iter=100)
    curve_args = (sup, N, rows, omega, t9, args.curve_runs, SEED, args.decode_every)
    res, sec = {}, {}
    for name, f in (("hqc_attack_curve", driver.hqc_attack_curve), ("hqc_attack_curve_retiring", driver.hqc_attack_curve_retiring)) * 2:
        t0 = time.perf_counter()
        res[name] = f(*curve_args, **how)
        sec.setdefault(name, []).append(time.perf_counter() - t0)  # (the first round of each is the warm-up: both are printed)
    a, b = res["hqc_attack_curve"], res["hqc_attack_curve_retiring"]
    for k in ("steps", "checks_needed", "oracle_calls_needed"):
        assert np.array_equal(a[k], b[k]), k
    assert a["decoder_stats"] == b["decoder_stats"]
    print(json.dumps({
        "part": "c", "graph": "hqc128 N17669_W50_s0, rows RandomState(1).permutation(N)[:%d]" % args.curve_checks,
        "decode_every": args.decode_every, "runs": args.curve_runs, "chunk": 4096, "rule": "product_sum", "max_iter": 100,
        "table": "wrapped_oracle_table((0.98, 0.9), (0.999, 0.99))", "steps": b["steps"].tolist(),
        "seconds_first_then_warm": {k: [round(x, 3) for x in v] for k, v in sec.items()},
        "retiring_over_whole_warm": round(sec["hqc_attack_curve_retiring"][1] / sec["hqc_attack_curve"][1], 4),
        "successes_every_step": a["successes"].tolist(), "first_successes": b["successes"].tolist(), "decoded": b["decoded"].tolist(),
        "never_recovered": int((b["checks_needed"] < 0).sum()), "four_fields_equal": True,
    }), flush=True)


if __name__ == "__main__":
    main()
