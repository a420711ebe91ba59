#!/usr/bin/env python3
"""Static instruction census of a compiler-written assembly file (hipcc -S --cuda-device-only with the unit's switches of build.py), per
function and per basic block, for the register-shuffling work of DESIGN.md 4.6 round 12:
    python tools/isa_census.py quad_kernel.s [function-substring] [--blocks N] [--loops] [--json out.json]
Opcodes are classified by prefix / infix only: `v_accvgpr` (copies between the two halves of the register file), `ds_` (LDS), `scratch_`
(private segment; split by whether the opcode contains `load`), `_f64` (fp64 arithmetic and conversions) and the `_dpp` encoding suffix.
These are static counts: a block's weight in the run is its count times its trips (the stamps' iteration and trial counts)."""
import collections
import json
import re
import subprocess
import sys

CLASSES = ("total", "f64", "agpr_copy", "lds", "dpp", "scratch_load", "scratch_store")


def classify(op):
    c = ["total"]
    if op.startswith("v_accvgpr"):
        c.append("agpr_copy")
    elif op.startswith("ds_"):
        c.append("lds")
    elif op.startswith("scratch_"):
        c.append("scratch_load" if "load" in op else "scratch_store")
    elif "_f64" in op:
        c.append("f64")
    if op.endswith("_dpp"):
        c.append("dpp")
    return c


def census(path):
    """{function: {"blocks": [(label, Counter)], "sum": Counter, "loops": {(innermost loop header, depth): Counter}}} in file order; the loop
    of a block is read off the compiler's own block comments (`in Loop: Header=BB6_361 Depth=1`, `This Inner Loop Header: Depth=2`)"""
    funcs = collections.OrderedDict()
    cur = blk = None
    loop = ("-", 0)

    def new_block(label):
        nonlocal blk
        blk = collections.Counter()
        cur["blocks"].append((label, blk))

    for line in open(path):
        s = line.rstrip()
        if not s:
            continue
        if cur is not None:
            label = re.match(r"^\.L(BB\d+_\d+):", s)
            fall = re.match(r"^; %bb\.(\d+):", s)   # (a fall-through block has no label of its own)
            if label or fall:
                new_block(label.group(1) if label else "bb." + fall.group(1))
                m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", s)
                loop = (m.group(1), int(m.group(2))) if m else ("-", 0)
            m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", s)
            if m:
                loop = (cur["blocks"][-1][0], int(m.group(1)))
            if label or fall:
                continue
        if s.lstrip().startswith(";"):
            continue
        m = re.match(r"^([A-Za-z_$][\w$.]*):", s)
        if m and not s.startswith(".L"):
            cur = funcs.setdefault(m.group(1), {"blocks": [], "sum": collections.Counter(), "loops": collections.OrderedDict()})
            new_block("entry")
            loop = ("-", 0)
            continue
        if cur is None:
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]*)\b", s)
        if m and not s.lstrip().startswith("."):
            for c in classify(m.group(1)):
                blk[c] += 1
                cur["sum"][c] += 1
                cur["loops"].setdefault(loop, collections.Counter())[c] += 1
    return funcs


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    nblocks = int(argv[argv.index("--blocks") + 1]) if "--blocks" in argv else 8
    if "--blocks" in argv:
        args.remove(str(nblocks))
    out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
    if out_json:
        args.remove(out_json)
    funcs = census(args[0])
    want = args[1] if len(args) > 1 else ""
    names = demangle(list(funcs))
    report = {}
    for f, d in funcs.items():
        if d["sum"]["total"] < 200 or want not in names[f]:
            continue
        short = re.sub(r"\(.*", "", names[f])[:90]
        s = d["sum"]
        print(f"{short}\n   " + "  ".join(f"{c} {s[c]}" for c in CLASSES) + f"  copy share {s['agpr_copy'] / s['total']:.3f}")
        report[short] = {c: s[c] for c in CLASSES}
        if want:
            for label, b in sorted(d["blocks"], key=lambda lb: -lb[1]["agpr_copy"])[:nblocks]:
                if b["agpr_copy"]:
                    print(f"      {label:12s} " + "  ".join(f"{c} {b[c]}" for c in CLASSES))
            if "--loops" in argv:   # instructions by innermost loop: what runs once per call, once per trip of a depth-1 loop, of a depth-2 loop
                for (header, depth), b in d["loops"].items():
                    print(f"      loop {header:10s} depth {depth}  " + "  ".join(f"{c} {b[c]}" for c in CLASSES))
                report[short]["loops"] = {f"{h}/{dp}": {c: b[c] for c in CLASSES} for (h, dp), b in d["loops"].items()}
    if out_json:
        json.dump(report, open(out_json, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1:])
