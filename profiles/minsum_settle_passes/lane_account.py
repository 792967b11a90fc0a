"""Per-lane account of one steady step of `bench.py --workload hqc128_minsum` from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python bench.py --gpus 1 --steps 5 --warmup 2
    python profiles/minsum_settle_passes/lane_account.py DIR/p_kernel_trace.csv

A step starts with its k_pack_bits dispatch; the LAST step of the trace is taken.  For every stream (lane) of that step:
kernel time by kind of launch, the idle time between the lane's consecutive launches, and -- per tile group, a group being
what lies between two k_var_first launches of the lane -- the wait in front of the group's first record-form check pass,
which is where lane 1 sits behind the phase event.  All times in microseconds.
"""
import collections
import csv
import re
import sys


def kind(name):
    m = re.search(r"(k_\w+)(<[^>]*>)?", name)
    if not m:
        return name.split("(")[0]
    k, t = m.group(1), m.group(2) or ""
    if k == "k_var_rec":
        return "k_var_rec<last>" if t.rstrip(">").endswith("true") else "k_var_rec"
    if k == "k_check_minsum_rec":
        return "k_check_minsum_rec<BOOT>" if t.split(",")[1].strip() == "true" else "k_check_minsum_rec"
    return k


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Stream_Id"], r["Queue_Id"], kind(r["Kernel_Name"]))
                 for r in rows))  # fmt: skip
    first = max(i for i, e in enumerate(ev) if e[4] == "k_pack_bits")
    ev = ev[first:]
    t0, t1 = ev[0][0], max(e[1] for e in ev)
    print(f"step: {len(ev)} dispatches, {(t1 - t0) / 1e3:.1f} us from the start of k_pack_bits to the end of the last kernel")
    lanes = collections.defaultdict(list)
    for e in ev:
        lanes[(e[2], e[3])].append(e)
    for (stream, queue), es in sorted(lanes.items()):
        busy = sum(e[1] - e[0] for e in es)
        print(f"\nstream {stream} (queue {queue}): {len(es)} dispatches, busy {busy / 1e3:.1f} us, "
              f"first start +{(es[0][0] - t0) / 1e3:.1f} us, last end +{(es[-1][1] - t0) / 1e3:.1f} us")
        by = collections.defaultdict(list)
        for e in es:
            by[e[4]].append((e[1] - e[0]) / 1e3)
        for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
            short = sum(1 for x in v if x < 8.0)
            print(f"  {k:28s} {len(v):4d} launches, {sum(v):8.1f} us in all, mean {sum(v) / len(v):6.1f}, of them {short} under 8 us")
        gaps = collections.defaultdict(list)
        for a, b in zip(es, es[1:]):
            gaps[(a[4], b[4])].append((b[0] - a[1]) / 1e3)
        idle = sum(sum(v) for v in gaps.values())
        print(f"  idle between consecutive launches: {idle:.1f} us in all")
        for (a, b), v in sorted(gaps.items(), key=lambda kv: -sum(kv[1])):
            if sum(v) >= 5.0:
                print(f"    {a} -> {b}: {len(v)} gaps, {sum(v):.1f} us in all, mean {sum(v) / len(v):.2f}, max {max(v):.1f}")
        waits = [(b[0] - a[1]) / 1e3 for a, b in zip(es, es[1:]) if a[4] == "k_var_first" and b[4].startswith("k_check_minsum_rec")]
        if waits:
            print(f"  wait between k_var_first and the group's first check pass: {len(waits)} groups, mean {sum(waits) / len(waits):.1f} us, "
                  f"{sum(waits):.1f} us in all")


if __name__ == "__main__":
    main()
