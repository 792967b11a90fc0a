"""What the reference's own arithmetic costs on the device: `precision="float64"` (scaldpc_bp_decode_batch_f64, the
probability-ratio recursion in float64) against the fp32 tanh kernels, on ONE handle in ONE process, warm, the two routes
taken in turn:

  graph    HQC-128 bench graph (W 50, R 4000: 204 000 edges), priors of eps = 0.05
  call     50 fixed iterations, device pointers in and out (decisions, iteration counts, flags; no posteriors)
  batch    256 and 4096
  single   one `decode()` of one received word from host memory, early exit, max_iter 100: the attack loop's call

    python profiles/microbench/ref64_cost.py [--batches 256 4096] [--iters 50] [--reps 3] [--rounds 3] [--tile-groups 2 4]

--tile-groups: also time the float64 route with `set_tile_group(g)` for each g (tiles per group; the default is the handle's
"group_mb" budget at 16 bytes per edge and codeword, one tile on this graph), as routes "float64_g<g>".

Prints one JSON line: per batch and route the median over `--rounds` rounds of the mean of `--reps` calls (every call ends in
a stream synchronise), the spread of the rounds, and directed edge-message updates per second (2 E messages per codeword and
iteration).  By bytes alone the float64 form moves at least twice what the fp32 message form moves: 8-byte messages."""
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
ROUTES = ("float32", "float64")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tile-groups", type=int, nargs="*", default=[])
    args = ap.parse_args()
    import torch

    routes = ROUTES + tuple("float64_g%d" % g for g in args.tile_groups)

    S = importlib.import_module("sca-ldpc_amd")
    bp = importlib.import_module("sca-ldpc_amd.bp")
    lib = importlib.import_module("sca-ldpc_amd._lib")
    trials = importlib.import_module("sca-ldpc_amd.trials")
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "hqc_first_rows.json")))
    H, Hin, _ = S.codes.hqc_bench_graph("hqc128", rows["N17669_W50_s0"])
    N, omega = S.codes.HQC_PARAMS["hqc128"]
    dec = bp.bp_decoder(H, max_iter=args.iters, bp_method="product_sum", channel_probs=trials.hqc_priors(N, H.m, omega, EPS))
    msg = dec.mc_hqc_run(max(args.batches), omega, EPS, SEED, max_iter=1, want_inputs=True)["msg"]  # the sweep's own trials
    res = {"graph": "hqc128 N17669_W50_s0 R%d" % H.m, "edges": int(H.nnz), "rule": "product_sum", "iters": args.iters,
           "early_exit": False, "eps": EPS, "reps": args.reps, "rounds": args.rounds, "device_io": True, "batches": {}}
    for nb in args.batches:
        d_in = torch.from_numpy(np.ascontiguousarray(msg[:nb])).cuda()
        out = {p: (torch.empty((nb, H.n), dtype=torch.uint8, device="cuda"), torch.empty(nb, dtype=torch.int32, device="cuda"),
                   torch.empty(nb, dtype=torch.uint8, device="cuda")) for p in routes}
        torch.cuda.synchronize()

        def call(p):
            b, it, cv = out[p]
            dec.set_tile_group(int(p.split("_g")[1]) if "_g" in p else 0)
            dec.decode_batch_device(d_in.data_ptr(), lib.IN_RECEIVED, nb, b.data_ptr(), max_iter=args.iters, early_exit=False,
                                    d_out_iters=it.data_ptr(), d_out_conv=cv.data_ptr(), precision=p.split("_g")[0])  # (synchronises)
            dec.set_tile_group(0)

        for p in routes:
            call(p)  # warm: workspaces, code objects
            assert torch.equal(out[p][0], out[p.split("_g")[0]][0])  # (results never depend on the group size)
        conv = {p: out[p][2].cpu().numpy().astype(bool) for p in ROUTES}
        same_bits = float((out["float32"][0][torch.from_numpy(conv["float64"]).cuda()] ==
                           out["float64"][0][torch.from_numpy(conv["float64"]).cuda()]).float().mean().item()) if conv["float64"].any() else None
        ms = {p: [] for p in routes}
        for _ in range(args.rounds):
            for p in routes:
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    call(p)
                ms[p].append((time.perf_counter() - t0) / args.reps * 1e3)
        med = {p: statistics.median(v) for p, v in ms.items()}
        res["batches"][str(nb)] = {
            "ms_per_call": {p: round(v, 3) for p, v in med.items()},
            "ms_spread": {p: round(max(v) - min(v), 3) for p, v in ms.items()},
            "edge_message_updates_per_s": {p: float("%.4g" % (2.0 * H.nnz * nb * args.iters / (v * 1e-3))) for p, v in med.items()},
            "float64_over_float32": round(med["float64"] / med["float32"], 3),
            "converged": {p: round(float(conv[p].mean()), 4) for p in ROUTES},
            "bits_equal_on_float64_converged": same_bits,
        }
    # the attack loop's call: one decode() of one word from host memory
    single = {}
    singles = {p: bp.bp_decoder(H, max_iter=100, bp_method="product_sum", channel_probs=trials.hqc_priors(N, H.m, omega, EPS),
                                precision=p) for p in ROUTES}
    for p in ROUTES:
        singles[p].decode(msg[0])
    t = {p: [] for p in ROUTES}
    for _ in range(max(args.rounds, 3)):
        for p in ROUTES:
            t0 = time.perf_counter()
            for k in range(10):
                singles[p].decode(msg[k])
            t[p].append((time.perf_counter() - t0) / 10 * 1e3)
    for p in ROUTES:
        single[p] = {"ms_per_decode": round(statistics.median(t[p]), 3), "iterations_of_the_last": int(singles[p].iter)}
        singles[p].close()
    res["single_decode_early_exit_max_iter_100"] = single
    print(json.dumps(res), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
