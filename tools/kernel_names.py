#!/usr/bin/env python3
"""The kernel names of a `rocprofv3 --kernel-trace --output-format csv -d DIR -- <command>` run in launch order, for comparing the launch
sequence of two builds (durations ignored): python tools/kernel_names.py DIR out.txt, then diff the two out.txt.
Launches are ordered by dispatch id (the order the host submitted them in); several processes are listed one after the other, by their
first launch. The list is folded without losing a name or the order: a kernel's argument list is dropped (its template arguments stay), a
name launched n times in a row is one line `n<TAB>name`, and a block of up to four such lines that repeats back to back is written once
inside `repeat N { }`."""
import csv
import glob
import os
import sys


def short(name):
    depth = 0
    for i, ch in enumerate(name):   # cut at the '(' outside template brackets that opens the parameter list
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0 and not name.startswith("(anonymous namespace)", i):
            return name[:i]
    return name


def fold(lines):
    out, i = [], 0
    while i < len(lines):
        width, reps = 1, 1
        for w in (1, 2, 3, 4):
            block = lines[i:i + w]
            if len(block) < w or any(b.startswith("#") for b in block):
                break
            r = 1
            while lines[i + r * w:i + (r + 1) * w] == block:
                r += 1
            if r > 1 and r * w > width * reps:
                width, reps = w, r
        if reps > 1:
            out += [f"repeat {reps} {{"] + ["  " + b for b in lines[i:i + width]] + ["}"]
        else:
            out.append(lines[i])
        i += width * reps
    return out


src, dst = sys.argv[1], sys.argv[2]
procs = []
for f in glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True):
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Dispatch_Id"]))
    if rows:
        procs.append((int(rows[0]["Start_Timestamp"]), [short(r["Kernel_Name"]).replace("(anonymous namespace)::", "") for r in rows]))
assert procs, f"no kernel trace under {src}"
lines, total = [], 0
for k, (_, names) in enumerate(sorted(procs, key=lambda p: p[0])):
    if len(procs) > 1:
        lines.append(f"# process {k}")
    i = 0
    while i < len(names):
        j = i
        while j < len(names) and names[j] == names[i]:
            j += 1
        lines.append(f"{j - i}\t{names[i]}")
        i = j
    total += len(names)
open(dst, "w").write("\n".join(fold(lines)) + "\n")
print(f"{dst}: {total} launches in {len(procs)} process(es)")
