"""What the next forward waits for, from a rocprofv3 --kernel-trace CSV of bench.py: medians over the last N steady-state steps of
the intervals between the training stream's last kernel (the hot rows' launch), the next batch's plan chain and the next forward.
Usage: python tools/trace_gates.py <kernel_trace.csv> [N=50]"""
import bisect
import csv
import statistics
import sys

path = sys.argv[1]
last_n = int(sys.argv[2]) if len(sys.argv) > 2 else 50
ev = {"fwd": [], "hot": [], "dgrad": [], "front": [], "chain_end": []}
NAMES = (("fwd", "bf3_emb_linear_tail_kernel"), ("hot", "emb_bwd_hot_apply_kernel"), ("dgrad", "h2_occ_pp_kernel"),
         ("front", "plan_front_kernel<true"), ("chain_end", "plan_large_kernel"))
for r in csv.DictReader(open(path)):
    for key, sub in NAMES:
        if sub in r["Kernel_Name"]:
            ev[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
for v in ev.values():
    v.sort()


def first_from(key, t):
    """first launch of `key` that starts at or after t, or None"""
    i = bisect.bisect_left(ev[key], (t, 0))
    return ev[key][i] if i < len(ev[key]) else None


rows = {"forward start -> hot rows' end": [], "hot rows' end -> next forward's start": [], "plan chain's end -> next forward's start": [],
        "hot rows' end -> plan chain's end": [], "plan chain's end - its dgrad's start": []}
fwd = ev["fwd"]
for i in range(len(fwd) - 1):
    f0, f1 = fwd[i][0], fwd[i + 1][0]
    hot, front = first_from("hot", f0), first_from("front", f0)
    if hot is None or front is None or hot[0] > f1 or front[0] > f1:
        continue
    chain, dgrad = first_from("chain_end", front[0]), first_from("dgrad", f1)     # the chain of batch i + 1 and that batch's dgrad
    if chain is None or dgrad is None:
        continue
    vals = (hot[1] - f0, f1 - hot[1], f1 - chain[1], chain[1] - hot[1], chain[1] - dgrad[0])
    for k, v in zip(rows, vals):
        rows[k].append(v / 1e3)
print("%d steps, medians of the last %d, us" % (len(rows["forward start -> hot rows' end"]), last_n))
for k, v in rows.items():
    v = v[-last_n:]
    print("%-42s %8.1f   (min %.1f, max %.1f)" % (k, statistics.median(v), min(v), max(v)))
