#!/usr/bin/env python3
"""What happens between two steps of bench.py at config[1], from a rocprofv3 trace (kernel trace + HIP API trace + memory copies, csv):
per step, the interval from the end of the previous step's last replay2_kernel (or replay2_lean_kernel) to the start of the step's first scan3_kernel -- the
kernels and copies inside it, the time the device does nothing, and the runtime calls the host makes meanwhile.

  rocprofv3 --kernel-trace --hip-trace --memory-copy-trace --output-format csv -d DIR -o NAME -- python bench.py --gpus 1 --steps 20 --warmup 5
  python tools/step_head_summary.py DIR/NAME [--steps 20] [--cut OUT_PREFIX]

--cut writes the rows of the median step only: from the start of the previous step's last replay to the end of the step's last kernel
(the HIP API trace of a whole run is several megabytes, nearly all of it set-up)."""
import argparse
import collections
import csv
import json
import statistics


def rows(path):
    try:
        with open(path, newline="") as fh:
            return list(csv.DictReader(fh))
    except FileNotFoundError:
        return []


def short(name):
    name = name.replace("void ", "")
    return name.split("(")[0].split("<")[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("prefix")
    ap.add_argument("--steps", type=int, default=20, help="timed steps: the last ones of the trace")
    ap.add_argument("--cut", default=None)
    args = ap.parse_args()
    kern = sorted(rows(args.prefix + "_kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    api = [r for r in rows(args.prefix + "_hip_api_trace.csv") if r["Domain"].startswith("HIP_RUNTIME")]
    cop = rows(args.prefix + "_memory_copy_trace.csv")
    replays = [r for r in kern if short(r["Kernel_Name"]) in ("replay2_kernel", "replay2_lean_kernel")]
    scans = [r for r in kern if short(r["Kernel_Name"]) == "scan3_kernel"]
    per_step = len(replays) // (len([r for r in kern if short(r["Kernel_Name"]) == "snapshot_kernel"]) or 1)
    # a step ends with its last replay; the next one's first scan is the first scan that starts after it
    ends = [int(r["End_Timestamp"]) for r in replays[per_step - 1::per_step]]
    steps = []
    for e in ends:
        nxt = [int(s["Start_Timestamp"]) for s in scans if int(s["Start_Timestamp"]) > e]
        if nxt:
            steps.append((e, nxt[0]))
    steps = steps[-args.steps:]
    out = []
    for a, b in steps:
        inside = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in kern if a <= int(r["Start_Timestamp"]) < b]
        inside += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy " + r["Direction"].replace("MEMORY_COPY_", "").lower()) for r in cop if a <= int(r["Start_Timestamp"]) < b]
        inside.sort()
        busy, t = 0, a
        for s, e, _ in inside:
            busy += max(0, min(e, b) - max(s, t))
            t = max(t, min(e, b))
        calls = collections.Counter(r["Function"] for r in api if a <= int(r["Start_Timestamp"]) < b)
        out.append({"interval_us": (b - a) / 1e3, "device_idle_us": (b - a - busy) / 1e3,
                    "device": [{"what": n, "at_us": round((s - a) / 1e3, 1), "us": round((e - s) / 1e3, 1)} for s, e, n in inside],
                    "runtime_calls": sum(calls.values()), "calls": dict(calls)})
    med = lambda k: round(statistics.median(o[k] for o in out), 1)
    summary = {"trace": args.prefix, "steps": len(out), "what": "end of the previous step's last replay2_kernel -> start of the first scan3_kernel",
               "interval_us": {"median": med("interval_us"), "min": round(min(o["interval_us"] for o in out), 1), "max": round(max(o["interval_us"] for o in out), 1)},
               "device_idle_us_median": med("device_idle_us"), "runtime_calls_median": med("runtime_calls"),
               "median_step": sorted(out, key=lambda o: o["interval_us"])[len(out) // 2]}
    print(json.dumps(summary))
    if args.cut and steps:
        a, b = sorted(steps, key=lambda ab: ab[1] - ab[0])[len(steps) // 2]
        t0 = max(int(r["Start_Timestamp"]) for r in replays if int(r["End_Timestamp"]) <= a)
        later = [e for e in ends if e > b]
        t1 = later[0] if later else max(int(r["End_Timestamp"]) for r in kern)
        for suffix, data in (("_kernel_trace.csv", kern), ("_hip_api_trace.csv", api), ("_memory_copy_trace.csv", cop)):
            keep = [r for r in data if t0 <= int(r["Start_Timestamp"]) <= t1]
            if keep:
                with open(args.cut + suffix, "w", newline="") as fh:
                    w = csv.DictWriter(fh, fieldnames=list(keep[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
                    w.writeheader()
                    w.writerows(keep)


if __name__ == "__main__":
    main()
