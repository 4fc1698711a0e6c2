#!/usr/bin/env python3
"""Memory-op and wait counts of the kernels in a hipcc device assembly file (-S
--cuda-device-only with the build's flags, or -save-temps' *-gfx950.s): per kernel whose name
matches the filter (substring of the mangled name) the instruction total, the flat_* / global_* /
ds_* / buffer_* / scratch_* ops (loads, stores, atomics), the s_waitcnt instructions by operand,
and the code length, registers and scratch the compiler reports. Runs on the CPU; a sibling of
tools/kmeta.py, which reads the metadata block only.

    python tools/isa_ops.py build.s [k_env_step_pair] [--waits N]

--waits N lists the N most frequent s_waitcnt operands (default 12)."""
import collections
import re
import sys

FAMILIES = ("flat", "global", "ds", "buffer", "scratch")
INFO = {"codeLenInByte": "code_bytes", "NumVgprs": "vgpr", "NumAgprs": "agpr", "NumSgprs": "sgpr",
        "ScratchSize": "scratch", "Occupancy": "occupancy", "LDSByteSize": "lds"}


def kind_of(op: str) -> str:
    if "atomic" in op:
        return "atomic"
    if "load" in op or "read" in op:
        return "load"
    if "store" in op or "write" in op:
        return "store"
    return "other"


def kernels(txt: str):
    """(name, body lines, trailer lines) of every function: the body runs from the function's
    label to its .Lfunc_end label, the trailer (the compiler's '; key: value' summary) from there
    to the next function."""
    lines = txt.split("\n")
    starts = [(m.group(1), n) for n, ln in enumerate(lines)
              if (m := re.match(r"\s*\.type\s+([\w.$]+),@function", ln))]
    for k, (name, n0) in enumerate(starts):
        n1 = starts[k + 1][1] if k + 1 < len(starts) else len(lines)
        end = next((n for n in range(n0, n1) if lines[n].startswith(".Lfunc_end")), n1)
        yield name, lines[n0:end], lines[end:n1]


def count(body, trailer):
    ops = collections.Counter()
    waits = collections.Counter()
    total = 0
    for ln in body:
        s = ln.split(";")[0].strip()
        if not s or s[0] == "." or s.endswith(":"):
            continue
        total += 1
        op, _, rest = s.partition(" ")
        fam = op.split("_")[0]
        if fam in FAMILIES:
            ops[f"{fam}_{kind_of(op)}"] += 1
        elif op == "s_waitcnt":
            waits[" ".join(rest.split())] += 1
    info = {}
    for ln in trailer:
        m = re.match(r";\s*(\w+)\s*[:=]\s*(\d+)", ln.strip())
        if m and m.group(1) in INFO:
            info[INFO[m.group(1)]] = int(m.group(2))
    return total, ops, waits, info


def main():
    args = [a for a in sys.argv[1:]]
    nw = 12
    if "--waits" in args:
        k = args.index("--waits")
        nw = int(args[k + 1])
        del args[k:k + 2]
    path = args[0]
    filt = args[1] if len(args) > 1 else ""
    with open(path) as f:
        txt = f.read()
    for name, body, trailer in kernels(txt):
        if filt and filt not in name:
            continue
        total, ops, waits, info = count(body, trailer)
        print(name)
        print(f"  instructions {total}  " + "  ".join(f"{k} {v}" for k, v in info.items()))
        for fam in FAMILIES:
            print(f"  {fam + '_*':10s} load {ops[fam + '_load']:5d}  store {ops[fam + '_store']:5d}  "
                  f"atomic {ops[fam + '_atomic']:3d}  other {ops[fam + '_other']:3d}")
        nwait = sum(waits.values())
        vm0 = sum(v for k, v in waits.items() if "vmcnt(0)" in k)
        vmn = sum(v for k, v in waits.items() if "vmcnt(" in k and "vmcnt(0)" not in k)
        lgk = sum(v for k, v in waits.items() if "lgkmcnt(" in k and "vmcnt(" not in k)
        print(f"  s_waitcnt {nwait}: with vmcnt(0) {vm0}, with vmcnt(k > 0) {vmn}, lgkmcnt only {lgk}")
        for k, v in waits.most_common(nw):
            print(f"    {v:5d}  {k}")


if __name__ == "__main__":
    main()
