"""What a Monte-Carlo call on drawn secrets (`mc_run_secret_device`) costs next to the q-ary sweep's call on the same trial
indices (`mc_run_device`): same handle, same process, the two forms alternating, results only (no [batch][N] output), on
DecoderN1280R512SW6 at batch 256 and 5 iterations.  Both calls use tables of the same K: the posterior tables of a 3-bit coding of
the 5 coefficient symbols and a 4-bit coding of the 25 row-sum symbols (the index modulo 16) at accuracy 0.95
(`trials.oracle_posterior_table`: 8 and 16 outcomes, the most `mc_run` takes); `mc_run` draws their levels with the outcomes'
marginal probabilities.

    python profiles/microbench/qary_secret_mc_cost.py [--reps 200] [--rounds 5]

The yardstick is `mc_run` on the same trials; what the secret call adds is one launch (k_q_mc_secret_sums) and a second
generator call per coefficient variable.  Config 4's decoder (DecoderN450R150V3C7B1) is not a special handle -- a drawn secret
needs the row-sum variables -- so it is not measured.  Prints one JSON line: medians of `--rounds` rounds of `--reps` calls after
a warm-up of both forms.  Every call ends in a stream synchronise."""
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
SEED = 2024


def expansion(symbols, bits):
    return [tuple((s >> (bits - 1 - i)) & 1 for i in range(bits)) for s in range(symbols)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch

    S = importlib.import_module("sca-ldpc_amd")
    qary = importlib.import_module("sca-ldpc_amd.qary")
    trials = importlib.import_module("sca-ldpc_amd.trials")
    gens = json.load(open(os.path.join(ROOT, "tests", "golden", "generators.json")))
    name, batch, iterations = "DecoderN1280R512SW6", 256, 5
    g = S.TannerGraph.from_coo(gens["qary_qc_256_6_3_s0_cb2"])
    dec = qary.decoder_class(name)(g.to_dense(np.int8), iterations)
    prior, prior_s = trials.centered_binomial(2), trials.centered_binomial(2, 6)
    tb = trials.oracle_posterior_table(expansion(5, 3), prior, 0.95)
    ts = trials.oracle_posterior_table([expansion(16, 4)[s & 15] for s in range(25)], prior_s, 0.95, reverse=True)
    lb, ls = tb["levels"].astype(np.float32), ts["levels"].astype(np.float32)
    marg_b, marg_s = prior @ tb["weights"], prior_s[::-1] @ ts["weights"]  # the outcomes' marginal laws: mc_run's weights
    stream = torch.cuda.current_stream().cuda_stream
    success = torch.empty(batch, dtype=torch.uint8, device="cuda")
    wrong = torch.empty((batch, 2), dtype=torch.int32, device="cuda")
    chan = torch.empty((batch, 2), dtype=torch.int32, device="cuda")
    success0 = torch.empty(batch, dtype=torch.uint8, device="cuda")
    errs0 = torch.empty(batch, dtype=torch.int32, device="cuda")
    wrong0 = torch.empty(batch, dtype=torch.int32, device="cuda")
    forms = {
        "mc_run": lambda: dec.mc_run_device(batch, SEED, lb, marg_b, ls, marg_s, success0.data_ptr(), errs0.data_ptr(), wrong0.data_ptr(),
                                            stream=stream),
        "mc_run_secret": lambda: dec.mc_run_secret_device(batch, SEED, prior, lb, tb["weights"], ls, ts["weights"], success.data_ptr(),
                                                          wrong.data_ptr(), chan.data_ptr(), stream=stream),
    }
    for f in forms.values():  # warm every shape the timed window uses
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, f in forms.items():
            t0 = time.perf_counter()
            for _ in range(args.reps):
                f()  # (each call ends in a stream synchronise)
            ms[k].append((time.perf_counter() - t0) / args.reps * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"decoder": name, "batch": batch, "iterations": iterations, "reps": args.reps, "rounds": args.rounds,
                      "levels": [int(lb.shape[0]), int(ls.shape[0])], "ms_per_call": {k: round(v, 4) for k, v in med.items()},
                      "ms_spread": {k: round(max(v) - min(v), 4) for k, v in ms.items()},
                      "secret_minus_mc_run_ms": round(med["mc_run_secret"] - med["mc_run"], 4),
                      "trials_per_s_secret": round(batch / med["mc_run_secret"] * 1e3), "keys_recovered": int(success.sum().item()),
                      "wrong_coefficients_per_trial": {"channel": round(chan[:, 0].float().mean().item(), 3),
                                                       "decoded": round(wrong[:, 0].float().mean().item(), 3)}}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
