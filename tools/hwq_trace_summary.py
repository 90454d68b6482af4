"""Dev tool (CPU): hardware-queue figures from the rocprofv3 kernel trace of a plain `bench.py --steps S --warmup W` run
(profiles/hw_queues_at_load.txt).

usage: tools/hwq_trace_summary.py <..._kernel_trace.csv> [steps = 20]

The timed region is taken as the last 3 x steps optimizer launches (spans 1..3 of every step) and the other kernels between them.
  * distinct Queue_Id among the region's minimize_kernel launches: the hardware queues the batches in flight really got;
  * span-1 launches side by side: time share by the number of span-1 optimizer kernels running, and the largest number of different
    queues among span-1 kernels running at the same moment;
  * wait of stage_epilogue_grid_kernel: its start minus the end of the kernel launched before it by the same host thread (its own
    batch's optimizer launch) -- what a bookkeeping launch spends behind ANOTHER batch's kernel when two streams share a queue.
"""
import collections
import csv
import sys


def main():
    path = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows = list(csv.DictReader(open(path)))
    own = "Thread_Id" if "Thread_Id" in rows[0] else "Stream_Id"  # one host thread (and one stream) per batch in flight
    ev = []
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void slamdev::", "").replace("slamdev::", "")
        span = int(name[name.index("minimize_kernel<") + 16]) if "minimize_kernel<" in name else 0
        ev.append({"a": int(r["Start_Timestamp"]), "b": int(r["End_Timestamp"]), "name": name, "span": span, "q": r.get("Queue_Id", "?"), "own": r.get(own, "?")})
    ev.sort(key=lambda e: e["a"])
    opt = [e for e in ev if e["span"]]
    if len(opt) < 3 * steps:
        sys.exit(f"{path}: {len(opt)} optimizer launches, fewer than 3 x {steps}")
    region = opt[-3 * steps:]
    t0 = min(e["a"] for e in region)
    reg_all = [e for e in ev if e["a"] >= t0]
    t1 = max(e["b"] for e in reg_all)
    print(f"columns: {','.join(rows[0].keys())}")
    print(f"timed region: {len(region)} optimizer launches, {len(reg_all)} kernels, {(t1 - t0) * 1e-6:.2f} ms = {(t1 - t0) * 1e-6 / steps:.3f} ms/step under trace")
    qs = collections.Counter(e["q"] for e in region)
    print(f"distinct queue ids among minimize_kernel launches: {len(qs)}  {dict(sorted(qs.items()))}")
    print(f"distinct {own} among them: {len(set(e['own'] for e in region))}")
    per_owner = collections.defaultdict(set)
    for e in region:
        per_owner[e["own"]].add(e["q"])
    shared = collections.Counter()
    for o, s in per_owner.items():
        for q in s:
            shared[q] += 1
    print(f"queues used by more than one batch: {sum(1 for v in shared.values() if v > 1)}")

    # span-1 launches side by side
    s1 = [e for e in region if e["span"] == 1]
    marks = sorted([(e["a"], 1, i) for i, e in enumerate(s1)] + [(e["b"], -1, i) for i, e in enumerate(s1)])
    live, last, hist, most_q = set(), marks[0][0], collections.Counter(), 0
    for t, d, i in marks:
        hist[len(live)] += t - last
        last = t
        if d > 0:
            live.add(i)
            most_q = max(most_q, len(set(s1[j]["q"] for j in live)))
        else:
            live.discard(i)
    tot = sum(hist.values())
    print(f"span-1 launches: {len(s1)}, mean {sum(e['b'] - e['a'] for e in s1) * 1e-6 / len(s1):.3f} ms; time share by number running: "
          f"{ {k: round(100.0 * v / tot, 1) for k, v in sorted(hist.items())} }; most different queues among span-1 kernels running together: {most_q}")

    # wait of the bookkeeping launch behind its own optimizer launch
    prev, waits = {}, []
    for e in reg_all:
        if e["name"].startswith("stage_epilogue_grid_kernel") and e["own"] in prev:
            waits.append(max(0, e["a"] - prev[e["own"]]["b"]))
        prev[e["own"]] = e
    if waits:
        waits.sort()
        print(f"stage_epilogue_grid_kernel: {len(waits)} launches, wait behind the launch before it: sum {sum(waits) * 1e-6:.3f} ms, "
              f"mean {sum(waits) * 1e-3 / len(waits):.1f} us, median {waits[len(waits) // 2] * 1e-3:.1f} us, max {waits[-1] * 1e-3:.1f} us")
    per = collections.defaultdict(lambda: [0, 0])
    for e in reg_all:
        per[e["name"][:56]][0] += 1
        per[e["name"][:56]][1] += e["b"] - e["a"]
    for n, (c, t) in sorted(per.items(), key=lambda kv: -kv[1][1])[:6]:
        print(f"  {n:56s} n={c:5d} total {t * 1e-6:9.2f} ms avg {t * 1e-3 / c:9.1f} us")


if __name__ == "__main__":
    main()
