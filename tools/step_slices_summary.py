#!/usr/bin/env python3
"""The two chains of a step of bench.py at config[1], from a rocprofv3 kernel trace (csv): per slice the start, end and duration of its
scan3_kernel and of its replay (replay2_kernel or replay2_lean_kernel), and the chunks of the rebuild, in microseconds from the end of
the previous step's last replay; for the median step (by its length, last replay to last replay) and as medians over the timed steps.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python bench.py --gpus 1 --steps 20 --warmup 5
  python tools/step_slices_summary.py label=DIR/NAME_kernel_trace.csv ... [--steps 20] [--cut OUT_DIR]

--cut writes OUT_DIR/<label>_kernel_trace.csv with the rows of the median step only."""
import argparse
import csv
import json
import os
import statistics


def short(name):
    return name.replace("void ", "").split("(")[0].split("<")[0]


def analyse(path, steps):
    kern = sorted(csv.DictReader(open(path, newline="")), key=lambda r: int(r["Start_Timestamp"]))
    K = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r) for r in kern]
    resets = [i for i, k in enumerate(K) if k[2] == "reset_state_kernel"]          # a step begins with its reset
    found = []
    for a, b in zip(resets, resets[1:] + [len(K)]):
        seg = K[a:b]
        sc = [k for k in seg if k[2] == "scan3_kernel"]
        rp = [k for k in seg if k[2] in ("replay2_kernel", "replay2_lean_kernel")]
        if sc and len(sc) == len(rp):
            found.append((seg, sc, rp, [k for k in seg if k[2] == "derive_all_kernel"]))
    found = found[-(steps + 1):]
    ns = len(found[-1][1])
    found = [f for f in found if len(f[1]) == ns]
    length = sorted((found[i][2][-1][1] - found[i - 1][2][-1][1], i) for i in range(1, len(found)))
    d, i = length[len(length) // 2]
    seg, sc, rp, dv = found[i]
    t0 = found[i - 1][2][-1][1]
    us = lambda x: round((x - t0) / 1e3)
    row = lambda ks: [{"start": us(s), "end": us(e), "us": round((e - s) / 1e3)} for s, e, _, _ in ks]
    med = lambda which, j: round(statistics.median((f[which][j][1] - f[which][j][0]) / 1e3 for f in found[1:]))
    res = {"trace": path, "steps": len(found) - 1, "slices": ns, "median_step_us": round(d / 1e3),
           "median_step": {"scan": row(sc), "replay": row(rp), "rebuild_chunk": row(dv)},
           "scan_us_median_over_steps": [med(1, j) for j in range(ns)], "replay_us_median_over_steps": [med(2, j) for j in range(ns)]}
    return res, [k[3] for k in seg]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("traces", nargs="+", metavar="label=path")
    ap.add_argument("--steps", type=int, default=20, help="timed steps: the last ones of the trace")
    ap.add_argument("--cut", default=None)
    args = ap.parse_args()
    out = {}
    for t in args.traces:
        label, path = t.split("=", 1)
        out[label], rows = analyse(path, args.steps)
        if args.cut:
            os.makedirs(args.cut, exist_ok=True)
            with open(os.path.join(args.cut, label + "_kernel_trace.csv"), "w", newline="") as fh:
                w = csv.DictWriter(fh, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
                w.writeheader()
                w.writerows(rows)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
