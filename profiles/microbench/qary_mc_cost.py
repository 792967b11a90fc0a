"""What a Monte-Carlo call of the q-ary decoders costs next to the plain call on the same trials: ms per call of
`min_sum_batch_device` (the materialised pmfs resident in HBM, symbols left there), of `mc_run_device` with the per-trial results
only, and of `mc_run_device` with the levels and the symbols as well, on config 4's decoder (DecoderN450R150V3C7B1, batch 1024,
the reference's good / bad rows at error rate 0.005) and on DecoderN1280R512SW6 (batch 256, two levels per table); 5 iterations.

    python profiles/microbench/qary_mc_cost.py [--reps 200] [--rounds 5] [--only qary_config4|kyber_sw6]

The plain call decodes exactly the trials the Monte-Carlo call draws (its input is built from the drawn levels), and the two must
return the same symbols.  Prints one JSON line per geometry: medians of `--rounds` rounds of `--reps` calls, the forms taken in
turn within a round, all in one process after a warm-up of every form.  Every call ends in a stream synchronise."""
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


def tables(workload):
    """((levels, weights), ...) per alphabet: config 4's (bad, good) of decode.py:232-237; two Dirichlet rows with their weight
    near 0 for the Kyber decoder's two alphabets."""
    if workload == "qary_config4":
        p = 1 / 3
        rows = np.array([[p, 0.25 * p, 1.75 * p], [p, 1.75 * p, 0.25 * p]], dtype=np.float32)
        return ((rows, (0.005, 0.995)),)
    rng = np.random.RandomState(6)
    out = []
    for Q in (5, 25):
        rows = rng.dirichlet(np.ones(Q), size=2)
        rows[1] = 0.5 * rows[1] + 0.5 * np.eye(Q)[Q // 2]
        out.append((rows.astype(np.float32), (0.1, 0.9)))
    return tuple(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch

    S = importlib.import_module("sca-ldpc_amd")
    qary = importlib.import_module("sca-ldpc_amd.qary")
    gens = json.load(open(os.path.join(ROOT, "tests", "golden", "generators.json")))
    for workload, name, graph, batch in (("qary_config4", "DecoderN450R150V3C7B1", "regular_identity_300_150_3_6_s1", 1024),
                                         ("kyber_sw6", "DecoderN1280R512SW6", "qary_qc_256_6_3_s0_cb2", 256)):
        if args.only and workload != args.only:
            continue
        g = S.TannerGraph.from_coo(gens[graph])
        dec = qary.decoder_class(name)(g.to_dense(np.int8), 5)
        tabs = tables(workload)
        flat = [a for t in tabs for a in t]
        stream = torch.cuda.current_stream().cuda_stream
        success = torch.empty(batch, dtype=torch.uint8, device="cuda")
        errs = torch.empty(batch, dtype=torch.int32, device="cuda")
        wrong = torch.empty(batch, dtype=torch.int32, device="cuda")
        levels = torch.empty((batch, g.n), dtype=torch.uint8, device="cuda")
        sym_mc = torch.empty((batch, g.n), dtype=torch.int8, device="cuda")
        sym = torch.empty((batch, g.n), dtype=torch.int8, device="cuda")
        mc_all = lambda: dec.mc_run_device(batch, SEED, *flat, success.data_ptr(), errs.data_ptr(), wrong.data_ptr(),  # noqa: E731
                                           levels.data_ptr(), sym_mc.data_ptr(), stream=stream)
        mc_all()
        # the plain call's input: the drawn trials, materialised in HBM
        lv = levels.long()
        bv = g.n - g.m if len(tabs) == 2 else g.n
        d_in = [torch.from_numpy(tabs[0][0]).cuda()[lv[:, :bv]].contiguous()]
        if len(tabs) == 2:
            d_in.append(torch.from_numpy(tabs[1][0]).cuda()[lv[:, bv:]].contiguous())
        ptrs = [t.data_ptr() for t in d_in]
        forms = {
            "plain": lambda: dec.min_sum_batch_device(*ptrs, batch, sym.data_ptr(), stream=stream),
            "mc": lambda: dec.mc_run_device(batch, SEED, *flat, success.data_ptr(), errs.data_ptr(), wrong.data_ptr(), stream=stream),
            "mc_levels_symbols": mc_all,
        }
        for f in forms.values():  # warm every shape the timed window uses
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        assert torch.equal(sym, sym_mc), "the plain call on the materialised trials must return the Monte-Carlo call's symbols"
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    f()  # (each call ends in a stream synchronise)
                ms[k].append((time.perf_counter() - t0) / args.reps * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"workload": workload, "decoder": name, "batch": batch, "iterations": 5, "reps": args.reps, "rounds": args.rounds,
                          "ms_per_call": {k: round(v, 4) for k, v in med.items()},
                          "ms_spread": {k: round(max(v) - min(v), 4) for k, v in ms.items()},
                          "mc_minus_plain_ms": {k: round(med[k] - med["plain"], 4) for k in ("mc", "mc_levels_symbols")},
                          "trials_per_s_mc": round(batch / med["mc"] * 1e3),
                          "successes": int(success.sum().item()), "frames_with_a_bad_symbol": int((errs > 0).sum().item()),
                          "input_bytes_the_plain_call_reads": sum(t.numel() * 4 for t in d_in)}), flush=True)
        dec.close()


if __name__ == "__main__":
    main()
