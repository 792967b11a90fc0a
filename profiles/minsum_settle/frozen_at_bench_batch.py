"""The bench batch's frozen-at numbers: the hqc128_minsum configuration of bench.py, two calls, scaldpc_bp_last_settle."""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
S = importlib.import_module("sca-ldpc_amd")
bp = importlib.import_module("sca-ldpc_amd.bp")
trials = importlib.import_module("sca-ldpc_amd.trials")
name, key = (sys.argv[1], sys.argv[2]) if len(sys.argv) > 2 else ("hqc128", "N17669_W50_s0")
rows = json.load(open(os.path.join(ROOT, "tests", "golden", "hqc_first_rows.json")))
H, Hin, _ = S.codes.hqc_bench_graph(name, rows[key])
N, omega = S.codes.HQC_PARAMS[name]
probs = trials.hqc_priors(N, Hin.m, omega, 0.05)
msg, ys = trials.hqc_trials(Hin, omega, 0.05, 4096, base_seed=2, first_index=0)
dec = bp.bp_decoder(H, max_iter=50, bp_method="min_sum", channel_probs=probs)
for i in range(3):
    t = time.perf_counter()
    out = dec.decode_batch(msg, early_exit=False)
    st = dec.last_settle()
    print(json.dumps({"call": i, "s": round(time.perf_counter() - t, 3), "horizon": st["horizon"], "launches_saved": st["launches_saved"],
                      "tiles_rerun": st["tiles_rerun"], "frozen_at_histogram": np.bincount(st["frozen_at"]).tolist(),
                      "converged": int(out["converged"].sum())}), flush=True)
dec.close()
