"""What the q-ary soft outputs cost: ms per call of the plain call, of margins + unmet counts only, and of all outputs, on
bench.py's two q-ary geometries (qary_config4: DecoderN450R150V3C7B1, batch 1024; kyber_sw6: DecoderN1280R512SW6, batch 256;
5 iterations each), channel outputs resident in HBM and every output left there (device pointers).

    python profiles/microbench/qary_soft_cost.py [--reps 200] [--only qary_config4|kyber_sw6] [--mode plain|margins|all]

Prints one JSON line per geometry: medians of `--rounds` rounds of `--reps` calls, the three forms taken in turn within a
round.  With --mode only that form runs (a few calls, for a kernel trace of its own: the transposing copy is
k_q_soft_transpose, its bytes are in the JSON line)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--mode", default=None, choices=["plain", "margins", "all"])
    args = ap.parse_args()
    import torch

    import bench

    S = importlib.import_module("sca-ldpc_amd")
    qary = importlib.import_module("sca-ldpc_amd.qary")
    lib = importlib.import_module("sca-ldpc_amd._lib")
    for workload, batch in (("qary_config4", 1024), ("kyber_sw6", 256)):
        if args.only and workload != args.only:
            continue
        name, g, inputs, _, what = bench.qary_case(workload, S, batch, 0)
        cls = qary.decoder_class(name)
        dec = cls(g.to_dense(np.int8), 5)
        d_in = [torch.from_numpy(x).cuda() for x in inputs]
        ptrs = [t.data_ptr() for t in d_in]
        sym = torch.empty((batch, g.n), dtype=torch.int8, device="cuda")
        costs = [torch.empty(x.shape, dtype=torch.float32, device="cuda") for x in inputs]
        margins = torch.empty((batch, g.n), dtype=torch.float32, device="cuda")
        unmet = torch.empty(batch, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        forms = {
            "plain": lambda: dec.min_sum_batch_device(*ptrs, batch, sym.data_ptr(), stream=stream),
            "margins": lambda: dec.min_sum_soft_batch_device(*ptrs, batch, sym.data_ptr(), d_margins=margins.data_ptr(),
                                                             d_unmet=unmet.data_ptr(), stream=stream),
            "all": lambda: dec.min_sum_soft_batch_device(*ptrs, batch, sym.data_ptr(), *[c.data_ptr() for c in costs],
                                                         margins.data_ptr(), unmet.data_ptr(), stream=stream),
        }
        table_bytes = sum(int(np.prod(x.shape)) for x in inputs) * 4
        copy_bytes = 2 * (table_bytes + batch * g.n * 4)  # k_q_soft_transpose of the "all" form: every float read once, written once
        if args.mode:
            for _ in range(10):
                forms[args.mode]()
            torch.cuda.synchronize()
            print(json.dumps({"workload": workload, "mode": args.mode, "calls": 10, "cost_table_bytes": table_bytes,
                              "transpose_bytes_all_form": copy_bytes}), flush=True)
            dec.close()
            continue
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
        plain = dec.min_sum_batch(*inputs)
        assert np.array_equal(sym.cpu().numpy(), plain)
        rate = lib.measure_rmw_stream(copy_bytes // 2)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"workload": workload, "what": what, "batch": batch, "iterations": 5, "reps": args.reps, "rounds": args.rounds,
                          "ms_per_call": {k: round(v, 4) for k, v in med.items()},
                          "ms_spread": {k: round(max(v) - min(v), 4) for k, v in ms.items()},
                          "added_ms": {k: round(med[k] - med["plain"], 4) for k in ("margins", "all")},
                          "cost_table_bytes": table_bytes, "transpose_bytes_all_form": copy_bytes,
                          "rmw_stream_GBps_at_that_size": round(rate, 1), "unmet_mean": float(unmet.float().mean().item())}), flush=True)
        dec.close()


if __name__ == "__main__":
    main()
