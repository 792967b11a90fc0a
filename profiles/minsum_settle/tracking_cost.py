"""Tracking cost: a workload that never settles (a (3,6)-regular graph), settle = 1 (tracking forced) against settle = 0, same
build.  Four handles, created in this order: A settle = 0, B settle = 1, C settle = 0 (a second one: what two handles differ by
when nothing differs), D the default (which does not track on a graph without an identity block)."""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
S = importlib.import_module("sca-ldpc_amd")
bp = importlib.import_module("sca-ldpc_amd.bp")
lib = importlib.import_module("sca-ldpc_amd._lib")
for n in (300, 12000):
    rng = np.random.RandomState(5)
    H = S.codes.make_regular_ldpc_graph(n, n // 2, 3, 6, rng)
    batch = 4096
    err = (rng.rand(batch, n) < 0.04).astype(np.uint8)
    synd = H.syndrome(err).astype(np.uint8)
    d_in = torch.from_numpy(synd).cuda(); d_out = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    decs = {}
    order = (("A", 0), ("B", 1), ("C", 0), ("D", None))
    for name, s in (order[::-1] if "reversed" in sys.argv[1:] else order):  # ("reversed": the handles created D, C, B, A)
        d = bp.bp_decoder(H, max_iter=50, bp_method="min_sum", channel_probs=np.full(n, 0.04))
        d.configure(path="stream")
        if s is not None:
            d.configure(settle=s)
        decs[name] = d
    res = {k: [] for k in decs}
    for rep in range(6):
        for k, d in decs.items():
            for _ in range(3): d.decode_batch_device(d_in.data_ptr(), lib.IN_SYNDROME, batch, d_out.data_ptr(), early_exit=False)
            torch.cuda.synchronize(); t = time.perf_counter()
            for _ in range(20): d.decode_batch_device(d_in.data_ptr(), lib.IN_SYNDROME, batch, d_out.data_ptr(), early_exit=False)
            torch.cuda.synchronize(); res[k].append((time.perf_counter() - t) / 20 * 1e3)
    med = {k: float(np.median(v[1:])) for k, v in res.items()}
    print(json.dumps({"graph": f"(3,6)-regular n={n}", "created": "".join(decs), "batch": batch, "ms_per_step": res, "median": med,
                      "B_over_A": med["B"] / med["A"], "C_over_A": med["C"] / med["A"], "D_over_A": med["D"] / med["A"],
                      "spread_A": (max(res["A"][1:]) - min(res["A"][1:])) / med["A"],
                      "tracked_tiles": {k: len(d.last_settle()["frozen_at"]) for k, d in decs.items()}}), flush=True)
