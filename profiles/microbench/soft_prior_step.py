#!/usr/bin/env python3
"""What per-codeword priors (scaldpc_bp_decode_batch_soft) cost a step of the flagship geometry: HQC-128, R = 4000,
batch 4096, 50 fixed iterations, min-sum alpha = 1, device I/O on the caller's stream (bench.py's `hqc128_minsum`).

One process, warm-up first, then `--repeats` rounds that ALTERNATE
  (a) the plain call;
  (b) the plain call with first_fused = 0: the launch sequence a soft call runs, plus nothing;
  (c) the soft call with prob_cols = R, every row equal to the shared check priors (outputs checked equal to (a));
  (d) the soft call with prob_cols = n.
Each repeat times `--steps` back-to-back steps.  Reads: (c) against (b) -- expected within (b)'s own run-to-run spread,
(max - min) / median of its repeats; (a) against the parent commit's (a) in the same GPU visit; (d) is reported next to
its byte model: 4 n 64 B per tile and variable pass on top of the pass's own bytes.  The conversion kernel alone is
timed between two events.  Prints one JSON line per repeat and a summary line.

    python profiles/microbench/soft_prior_step.py [--repeats 5] [--steps 10]
"""
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

S = importlib.import_module("sca-ldpc_amd")
bp = importlib.import_module("sca-ldpc_amd.bp")
lib = importlib.import_module("sca-ldpc_amd._lib")
trials = importlib.import_module("sca-ldpc_amd.trials")


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--eps", type=float, default=0.05)
    args = ap.parse_args()
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "hqc_first_rows.json")))
    H, Hin, _ = S.codes.hqc_bench_graph("hqc128", rows["N17669_W50_s0"])
    N, omega = S.codes.HQC_PARAMS["hqc128"]
    R, n, batch, iters = Hin.m, H.n, args.batch, 50
    probs = trials.hqc_priors(N, R, omega, args.eps)
    msg, _ = trials.hqc_trials(Hin, omega, args.eps, batch, base_seed=2)
    soft = hasattr(lib.load(), "scaldpc_bp_decode_batch_soft")  # (a library without the entry point: (a) and (b) only)
    d_in = torch.from_numpy(msg).cuda()
    p32 = torch.from_numpy(probs.astype(np.float32)).cuda()
    d_cp_R = p32[N:].repeat(batch, 1).contiguous()
    d_cp_n = p32.repeat(batch, 1).contiguous() if soft else None
    stream = torch.cuda.current_stream().cuda_stream
    # ONE decoder, so that every variant runs on the same message workspace (where an allocation lands moves a step by
    # more than what is being measured); (b) switches first_fused off for its steps and back on afterwards
    dec = bp.bp_decoder(H, max_iter=iters, bp_method="min_sum", channel_probs=probs)
    names = ("a", "b", "c", "d") if soft else ("a", "b")
    decs = {name: dec for name in names}
    outs = {name: (torch.empty((batch, n), dtype=torch.uint8, device="cuda"), torch.empty(batch, dtype=torch.uint8, device="cuda"))
            for name in names}

    def step(name):
        dec.configure(first_fused=0 if name == "b" else 1)
        kw = {}
        if name == "c":
            kw = dict(d_channel_probs=d_cp_R.data_ptr(), prob_cols=R)
        elif name == "d":
            kw = dict(d_channel_probs=d_cp_n.data_ptr(), prob_cols=n)
        decs[name].decode_batch_device(d_in.data_ptr(), lib.IN_RECEIVED, batch, outs[name][0].data_ptr(), early_exit=False,
                                       stream=stream, d_out_conv=outs[name][1].data_ptr(), **kw)

    for name in decs:  # warm-up: allocations, tables
        for _ in range(3):
            step(name)
    torch.cuda.synchronize()
    for name in decs:
        same = torch.equal(outs[name][0], outs["a"][0]) and torch.equal(outs[name][1], outs["a"][1])
        kt = decs[name].time_kernels(1, stream=stream)
        print(json.dumps({"outputs_equal_to_a": name, "equal": bool(same), "codewords_per_launch": kt["codewords"], "lanes": kt["lanes"]}), flush=True)
        assert same, name
    ms = {name: [] for name in decs}
    for rep in range(args.repeats):
        row = {"repeat": rep}
        for name in decs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(name)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            row[name + "_ms_per_step"] = round(ms[name][-1], 3)
        print(json.dumps(row), flush=True)
    summary = {"summary": True, "steps": args.steps, "repeats": args.repeats}
    for name in decs:
        summary[name + "_median_ms"] = round(statistics.median(ms[name]), 3)
    summary["b_spread"] = round((max(ms["b"]) - min(ms["b"])) / statistics.median(ms["b"]), 4)
    summary["a_spread"] = round((max(ms["a"]) - min(ms["a"])) / statistics.median(ms["a"]), 4)
    if soft:
        summary["c_over_b"] = round(statistics.median(ms["c"]) / statistics.median(ms["b"]) - 1.0, 4)
        summary["d_over_b"] = round(statistics.median(ms["d"]) / statistics.median(ms["b"]) - 1.0, 4)
        # the conversion alone: a soft call of ONE iteration against a plain first_fused = 0 call of one iteration brackets it
        # too loosely, so the kernel is timed through the library's own path at max_iter = 1 between two events, minus (b) at 1
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for name, e0, e1 in (("b", ev[0], ev[1]), ("c", ev[2], ev[3])):
            kw = dict(d_channel_probs=d_cp_R.data_ptr(), prob_cols=R) if name == "c" else {}
            for timed in (False, True):
                if timed:
                    e0.record()
                dec.configure(first_fused=0)  # (both)
                for _ in range(20):
                    decs[name].decode_batch_device(d_in.data_ptr(), lib.IN_RECEIVED, batch, outs[name][0].data_ptr(), max_iter=1,
                                                   early_exit=False, stream=stream, d_out_conv=outs[name][1].data_ptr(), **kw)
                if timed:
                    e1.record()
                torch.cuda.synchronize()
        summary["one_iteration_call_b_ms"] = round(ev[0].elapsed_time(ev[1]) / 20, 4)
        summary["one_iteration_call_c_ms"] = round(ev[2].elapsed_time(ev[3]) / 20, 4)
        summary["conversion_R_cols_ms"] = round((ev[2].elapsed_time(ev[3]) - ev[0].elapsed_time(ev[1])) / 20, 4)
        tiles = (batch + 63) // 64
        summary["plane_MB_R_cols"] = round(tiles * R * 256 / 1e6, 1)
        summary["plane_MB_n_cols"] = round(tiles * n * 256 / 1e6, 1)
        summary["d_extra_bytes_per_tile_and_variable_pass"] = 4 * n * 64
    print(json.dumps(summary), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
