"""What DecoderSpecial costs on checks of more than eight edges (k_q_special_check_dp_any), channel outputs resident in HBM
and the symbols left there (device pointers), 5 iterations per call:

    SW 9, B = 2 (DecoderN1024R256SW9B2) on codes.make_qary_qc_graph(256, 9, 3, make_random_state(0), 1) -- 256 x 1024, rows of
          10 edges -- at batch 1, 64 and 256;
    SW 12, B = 2 (DecoderN1024R256SW12B2) on the same generator's graph at sum weight 12, batch 256;
    the Kyber SW 6 graph (bench.py's kyber_sw6, DecoderN1280R512SW6) at batch 256 with dp_any = 1 against the default kernels.

    python profiles/microbench/qary_special_any_cost.py [--reps 20] [--rounds 5]

Prints one JSON line per point: the median over `--rounds` rounds of `--reps` calls of the wall time per call, and the
check / variable kernels' own shares of one call from the timing knob (HIP events around every launch)."""
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


def measure(torch, dec, inputs, batch, n, reps, rounds, knobs):
    dec.configure(**knobs)
    d_in = [torch.from_numpy(x).cuda() for x in inputs]
    ptrs = [t.data_ptr() for t in d_in]
    sym = torch.empty((batch, n), dtype=torch.int8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: dec.min_sum_batch_device(*ptrs, batch, sym.data_ptr(), stream=stream)  # noqa: E731
    for _ in range(3):
        call()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()  # (each call ends in a stream synchronise)
        ms.append((time.perf_counter() - t0) / reps * 1e3)
    dec.configure(timing=1)
    call()
    t = dec.last_timing()
    dec.configure(timing=0)
    return {"ms_per_call": round(statistics.median(ms), 4), "ms_spread": round(max(ms) - min(ms), 4), "check_kernel": t["check_kernel"],
            "ms_check": round(t["ms_check"], 4), "ms_var": round(t["ms_var"], 4), "ms_loop": round(t["ms_loop"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch

    import bench

    S = importlib.import_module("sca-ldpc_amd")
    qary = importlib.import_module("sca-ldpc_amd.qary")
    B = 2
    for SW, batches in ((9, (1, 64, 256)), (12, (256,))):
        g = S.codes.make_qary_qc_graph(256, SW, 3, S.codes.make_random_state(0), 1)
        name = f"DecoderN{g.n}R{g.m}SW{SW}B{B}"
        dec = qary.decoder_class(name)(g.to_dense(np.int8), 5)
        for batch in batches:
            rng = np.random.RandomState(SW + batch)
            pb = rng.dirichlet(np.ones(2 * B + 1), size=(batch, g.n - g.m)).astype(np.float32)
            ps = rng.dirichlet(np.ones(2 * SW * B + 1), size=(batch, g.m)).astype(np.float32)
            out = measure(torch, dec, (pb, ps), batch, g.n, args.reps, args.rounds, dict())
            print(json.dumps({"decoder": name, "batch": batch, "iterations": 5, "reps": args.reps, "rounds": args.rounds, **out}), flush=True)
        dec.close()
    name, g, inputs, _, _ = bench.qary_case("kyber_sw6", S, 256, 0)
    dec = qary.decoder_class(name)(g.to_dense(np.int8), 5)
    for knobs in (dict(dp_any=-1), dict(dp_any=1), dict(dp_any=-1), dict(dp_any=1)):
        out = measure(torch, dec, inputs, 256, g.n, 10 * args.reps, args.rounds, knobs)
        print(json.dumps({"decoder": name, "batch": 256, "iterations": 5, "reps": 10 * args.reps, "rounds": args.rounds, **knobs, **out}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
