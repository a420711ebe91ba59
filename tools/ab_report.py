#!/usr/bin/env python3
"""the reports of tools/ab_prune.sh: `compare OUT` (bench.py --dump-outputs of the two builds, array by array), `line NAME FILE` (one bench
line's kernel_ms, ms_per_step, value, hand-ons) and `summary LOG` (median, min, max per build; the pruned build's range against the parent's,
the gain against three times the parent's max - min; the MJPCX_PRUNE=0 build (tools/ab_park.sh: the MJPCX_PARK=0 build) against the parent's spread)"""
import json, os, sys
import numpy as np
mode = sys.argv[1]
if mode == "compare":
    out = sys.argv[2]
    for v in ("parent", "new"):
        d = json.loads(open(f"{out}/line_dump_{v}.json").read())
        print(f"{v} dump: handed_on {d['roofline']['handed_on_last_step']['candidates']}")
    names = sorted(os.listdir(f"{out}/dump_parent"))
    assert names == sorted(os.listdir(f"{out}/dump_new")), names
    bad = 0
    for n in names:
        a, b = np.load(f"{out}/dump_parent/{n}"), np.load(f"{out}/dump_new/{n}")
        eq = a.shape == b.shape and np.array_equal(a, b)
        bad += not eq
        print(f"outputs {n} {a.shape} {'array_equal' if eq else 'DIFFERENT'}")
    print(f"outputs: {len(names)} arrays, {bad} different")
    sys.exit(1 if bad else 0)
elif mode == "line":
    d = json.loads(open(sys.argv[3]).read())
    print(sys.argv[2], "kernel_ms", round(d["roofline"]["kernel_ms"], 3), "ms_per_step", round(d["ms_per_step"], 3), "value", round(d["value"]),
          "handed_on", d["roofline"]["handed_on_last_step"]["candidates"])
else:
    rows = {}
    for l in open(sys.argv[2]):
        w = l.split()
        if len(w) >= 5 and w[1] == "kernel_ms":
            rows.setdefault(w[0], []).append((float(w[2]), float(w[4])))
    for i, key in enumerate(("kernel_ms", "ms_per_step")):
        p = np.array([r[i] for r in rows["parent"]])
        sp = p.max() - p.min()
        txt = f"{key} parent median {np.median(p):.3f} ({p.min():.3f}-{p.max():.3f}, spread {sp:.3f})"
        for v in ["new"] + [k for k in rows if k not in ("parent", "new")]:   # (the third build: `noprune` of ab_prune.sh, `nopark` of ab_park.sh)
            x = np.array([r[i] for r in rows[v]])
            gain = np.median(p) - np.median(x)
            txt += f"  {v} median {np.median(x):.3f} ({x.min():.3f}-{x.max():.3f}) gain {gain:.3f} ({100 * gain / np.median(p):.1f} %)"
            if v == "new":
                txt += f" 3 x spread {3 * sp:.3f} ranges {'disjoint' if x.max() < p.min() else 'OVERLAP'}"
            else:
                txt += f" within the parent's spread: {'yes' if abs(gain) <= sp else 'NO'}"
        print(txt)
