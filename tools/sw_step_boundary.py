"""Where a config-2 step spends its time outside the fill: the batch of bench.py's headline (65 536 pairs of 150 x 150, scores
bound to page-locked memory), warmed for 0.5 s, then 200 launch() + scores() steps.

    python tools/sw_step_boundary.py run              the untraced step: median, min and mean of the 200 steps (one JSON line)
    python tools/sw_step_boundary.py parse DIR        the spans of the same program's trace (tools/sw_step_boundary.sh wrote DIR):
        A  the launch API call            B  its return to the kernel's start
        K  the kernel                     C  the kernel's end to the return of the wait (hipStreamSynchronize or hipEventSynchronize)
    medians over the last 200 fills, in microseconds, and A + B + K + C beside the traced step."""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = 200


def run():
    import accelerating_genomics_amd.api as agx
    import accelerating_genomics_amd.synth as synth

    with agx.Context(0) as ctx:
        sw = synth.sw_pairs(65536, 150, 150, seed=2, related_frac=0.25)
        out = agx.host_array(sw.n_pairs, np.int32)
        dev = ctx.sw_batch(sw)
        dev.bind_scores(out)
        t_end = time.perf_counter() + 0.5
        while time.perf_counter() < t_end:
            dev.launch()
            dev.scores(out)
        per = np.empty(STEPS)
        for k in range(STEPS):
            t0 = time.perf_counter()
            dev.launch()
            dev.scores(out)
            per[k] = time.perf_counter() - t0
        dev.close()
    print(json.dumps({"lib": os.path.basename(agx.LIB_PATH), "steps": STEPS, "step_us": {"median": float(np.median(per)) * 1e6, "min": float(per.min()) * 1e6,
                                                                                       "mean": float(per.mean()) * 1e6},
                      "checksum": int(out.astype(np.int64).sum())}))


def parse(d):
    kern, api = [], []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "sw_fill" in r["Kernel_Name"]:
                kern.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Correlation_Id"])))
    for f in glob.glob(d + "/**/*hip_api_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            api.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Correlation_Id"]), r["Function"]))
    kern.sort()
    kern = kern[-STEPS:]
    by_corr = {a[2]: a for a in api if "LaunchKernel" in a[3]}
    if not all(k[2] in by_corr for k in kern):  # no shared correlation ids: the last launch call that began before the kernel
        launches = sorted(a for a in api if "LaunchKernel" in a[3])
        starts = [a[0] for a in launches]
        by_corr = {k[2]: launches[int(np.searchsorted(starts, k[0])) - 1] for k in kern}
    waits = sorted(a for a in api if a[3] in ("hipStreamSynchronize", "hipEventSynchronize"))
    rows, names, w = [], {}, 0
    for k, (ks, ke, corr) in enumerate(kern):
        la = by_corr[corr]
        while waits[w][1] < ke:  # the first wait that returns behind the kernel's end
            w += 1
        names[(la[3], waits[w][3])] = names.get((la[3], waits[w][3]), 0) + 1
        nxt = by_corr[kern[k + 1][2]][0] if k + 1 < len(kern) else None
        rows.append((la[1] - la[0], ks - la[1], ke - ks, waits[w][1] - ke, waits[w][1] - la[0], (nxt - la[0]) if nxt else np.nan))
    m = np.nanmedian(np.array(rows, dtype=float), axis=0) / 1e3
    print("calls (launch, wait): %s" % ", ".join("%s + %s x %d" % (a, b, n) for (a, b), n in sorted(names.items())))
    print("medians over %d fills, us:  A %.2f   B %.2f   K %.2f   C %.2f   sum %.2f" % (len(rows), m[0], m[1], m[2], m[3], m[:4].sum()))
    print("launch call's start to the wait's return %.2f; to the next launch call's start (the traced step) %.2f" % (m[4], m[5]))


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else parse(sys.argv[2])
