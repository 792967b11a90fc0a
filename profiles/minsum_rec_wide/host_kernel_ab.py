#!/usr/bin/env python3
"""k_var<64, P> gained a record mode; what do its pre-existing users pay?  They are the message form on graphs with a column of
33 ... 64 edges: min-sum by default there, and the tanh rule.  One process per library (SCALDPC_SO selects the build, read at
import), so an A/B is a shell loop that alternates the parent's library and this commit's:

    SCALDPC_SO=PARENT/libscaldpc.so python profiles/minsum_rec_wide/host_kernel_ab.py
    python profiles/minsum_rec_wide/host_kernel_ab.py

HQC-128, W 50, R 8000, batch 4096, 50 fixed iterations, default knobs (minsum_rec = 1: the message form on this graph), device
I/O on the caller's stream; per update rule 3 warm-up calls, then 3 rounds of 5 calls.  Prints one JSON line: ms per step per
round, their median and spread, and the `time_kernels` figure per variable pass (k_var<64, SharedPrior> alone)."""
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

S = importlib.import_module("sca-ldpc_amd")
bp = importlib.import_module("sca-ldpc_amd.bp")
lib = importlib.import_module("sca-ldpc_amd._lib")
trials = importlib.import_module("sca-ldpc_amd.trials")


def main():
    import torch

    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "hqc_first_rows.json")))
    H, Hin, _ = S.codes.hqc_bench_graph("hqc128", rows["N17669_W50_s0"], R=8000)
    N, omega = S.codes.HQC_PARAMS["hqc128"]
    batch, eps = 4096, 0.05
    probs = trials.hqc_priors(N, Hin.m, omega, eps)
    msg, _ = trials.hqc_trials(Hin, omega, eps, batch, base_seed=2)
    d_in = torch.from_numpy(msg).cuda()
    d_out = torch.empty((batch, H.n), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"library": os.path.basename(os.path.dirname(os.path.abspath(lib.SO_PATH))) + "/" + os.path.basename(lib.SO_PATH)}
    for method in ("min_sum", "product_sum"):
        dec = bp.bp_decoder(H, max_iter=50, bp_method=method, channel_probs=probs)
        step = lambda: dec.decode_batch_device(d_in.data_ptr(), lib.IN_RECEIVED, batch, d_out.data_ptr(), early_exit=False, stream=stream)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        kt = dec.time_kernels(20, stream=stream)
        assert kt["record_form"] is False
        ms = []
        for _ in range(3):
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                step()
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) / 5 * 1e3, 3))
        med = statistics.median(ms)
        out[method] = {"ms_per_step": ms, "median": med, "spread": round((max(ms) - min(ms)) / med, 4),
                       "ms_per_var_pass": round(kt["ms_var"] / kt["launches_var"], 4)}
        dec.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
