#!/usr/bin/env python3
"""What the min-sum record form on columns of 33 ... 64 edges (`minsum_rec = 2`) costs and saves, per step: HQC graphs past
the 32-edge line, batch 4096, 50 fixed iterations, min-sum alpha = 1, device I/O on the caller's stream (bench.py's call).

One process, warm-up first, then `--rounds` rounds that ALTERNATE the routes, `--calls` back-to-back calls each, the order
of the routes reversed in every other round (the route that runs second is not always the same one); medians over the
rounds, spread = (max - min) / median.

  wide graph (default: HQC-128, W 50, R 8000 -- 54 columns of 33 .. 36 edges among 25 669):
    msg        minsum_rec = 0: the message form, what such a graph runs by default
    rec        minsum_rec = 2, settle = 0: the record form, every pass run
    rec_settle minsum_rec = 2, the default settle (2 on a graph [Hin | I])
  outputs of all three are checked equal first.  `time_kernels` figures per route: ms per check pass and per variable pass
  (under minsum_rec = 2 a variable pass is TWO launches, the narrow slice and the wide one; the C ABI times the pass as one
  figure -- the per-launch split is in the kernel trace profiles/minsum_rec_wide/README.md quotes).
  bench graph (HQC-128, W 50, R 4000, no column past 24): minsum_rec = 1 against 2.  ASSERTED equal: the form bits and
  PASS counts of `time_kernels` and the words of `last_schedule()` / `last_settle()`.  None of these counts kernel launches
  inside a variable pass; that knob 2 adds none there follows from the code (`launch_var`: no bucket past 32, no second
  launch) and shows in the times reported.

    python profiles/microbench/rec_wide_cost.py [--name hqc128 --key N17669_W50_s0 --R 8000] [--rounds 3] [--calls 5]
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


def measure(torch, H, Hin, name, eps, batch, routes, rounds, calls, label):
    """routes: {route: knobs}.  One decoder per route (a knob flip between calls would rebuild nothing, but the settle
    horizon is learned per handle).  -> {route: [ms per step per round]}, prints the rows."""
    N, omega = S.codes.HQC_PARAMS[name]
    probs = trials.hqc_priors(N, Hin.m, omega, eps)
    msg, _ = trials.hqc_trials(Hin, omega, eps, batch, base_seed=2)
    d_in = torch.from_numpy(msg).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    decs, outs = {}, {}
    for r, knobs in routes.items():
        decs[r] = bp.bp_decoder(H, max_iter=50, bp_method="min_sum", channel_probs=probs)
        decs[r].configure(**knobs)
        outs[r] = (torch.empty((batch, H.n), dtype=torch.uint8, device="cuda"), torch.empty(batch, dtype=torch.uint8, device="cuda"))

    def step(r):
        decs[r].decode_batch_device(d_in.data_ptr(), lib.IN_RECEIVED, batch, outs[r][0].data_ptr(), early_exit=False, stream=stream,
                                    d_out_conv=outs[r][1].data_ptr())

    for r in routes:  # warm-up: allocations, tables, the settle horizon
        for _ in range(3):
            step(r)
    torch.cuda.synchronize()
    first = next(iter(routes))
    info = {}
    for r in routes:
        assert torch.equal(outs[r][0], outs[first][0]) and torch.equal(outs[r][1], outs[first][1]), (label, r)
        kt = decs[r].time_kernels(20, stream=stream)
        info[r] = {"record_form": kt["record_form"], "var_slim": kt["var_slim"], "lanes": kt["lanes"], "codewords_per_launch": kt["codewords"],
                   "launches_check": kt["launches_check"], "launches_var": kt["launches_var"],
                   "ms_per_check_pass": round(kt["ms_check"] / kt["launches_check"], 4),
                   "ms_per_var_pass": round(kt["ms_var"] / kt["launches_var"], 4)}
        step(r)  # (time_kernels ran on the decode's state: the next timed call starts from a decode again)
        info[r]["schedule"] = decs[r].last_schedule()
        info[r]["settle"] = {k: v for k, v in decs[r].last_settle().items() if k != "frozen_at"}
        print(json.dumps({"graph": label, "route": r, "knobs": routes[r], "outputs_equal": True, **info[r]}), flush=True)
    torch.cuda.synchronize()
    ms = {r: [] for r in routes}
    for rnd in range(rounds):
        row = {"graph": label, "round": rnd}
        for r in (list(routes)[::-1] if rnd % 2 else list(routes)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                step(r)
            torch.cuda.synchronize()
            ms[r].append((time.perf_counter() - t0) / calls * 1e3)
            row[r + "_ms_per_step"] = round(ms[r][-1], 3)
        print(json.dumps(row), flush=True)
    for d in decs.values():
        d.close()
    return ms, info


def summary(label, ms, extra=None):
    out = {"summary": label}
    for r, v in ms.items():
        out[r + "_median_ms"] = round(statistics.median(v), 3)
        out[r + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 4)
    out.update(extra or {})
    print(json.dumps(out), flush=True)
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="hqc128")
    ap.add_argument("--key", default="N17669_W50_s0")
    ap.add_argument("--R", type=int, default=8000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--eps", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--skip-bench-graph", action="store_true")
    args = ap.parse_args()
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "hqc_first_rows.json")))
    H, Hin, _ = S.codes.hqc_bench_graph(args.name, rows[args.key], R=args.R)
    cdeg = np.diff(np.asarray(H.col_ptr))
    label = f"{args.name} {args.key} R={args.R}"
    print(json.dumps({"graph": label, "edges": int(H.nnz), "columns": int(H.n), "max_col_deg": int(cdeg.max()),
                      "columns_over_32": int((cdeg > 32).sum()), "batch": args.batch, "eps": args.eps}), flush=True)
    assert 32 < cdeg.max() <= 64, "the wide graph must hold a column of 33 ... 64 edges"
    routes = {"msg": {"minsum_rec": 0}, "rec": {"minsum_rec": 2, "settle": 0}, "rec_settle": {"minsum_rec": 2}}
    ms, info = measure(torch, H, Hin, args.name, args.eps, args.batch, routes, args.rounds, args.calls, label)
    assert info["msg"]["record_form"] is False and info["rec"]["record_form"] and info["rec_settle"]["record_form"]
    med = {r: statistics.median(v) for r, v in ms.items()}
    summary(label, ms, {"rec_over_msg": round(med["rec"] / med["msg"], 4), "rec_settle_over_msg": round(med["rec_settle"] / med["msg"], 4)})
    if args.skip_bench_graph:
        return
    # the bench graph: no wide column, so 2 must be 1 launch for launch
    H, Hin, _ = S.codes.hqc_bench_graph("hqc128", rows["N17669_W50_s0"])
    label = f"hqc128 N17669_W50_s0 R={Hin.m} (bench)"
    ms, info = measure(torch, H, Hin, "hqc128", args.eps, args.batch, {"knob1": {"minsum_rec": 1}, "knob2": {"minsum_rec": 2}},
                       args.rounds, args.calls, label)
    same = ("record_form", "var_slim", "lanes", "codewords_per_launch", "launches_check", "launches_var", "schedule", "settle")
    for k in same:
        assert info["knob1"][k] == info["knob2"][k], (k, info["knob1"][k], info["knob2"][k])
    med = {r: statistics.median(v) for r, v in ms.items()}
    summary(label, ms, {"same_passes_and_schedule": True, "knob2_over_knob1": round(med["knob2"] / med["knob1"], 4)})


if __name__ == "__main__":
    main()
