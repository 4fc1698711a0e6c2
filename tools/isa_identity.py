#!/usr/bin/env python
"""Per-kernel comparison of two builds' device assembly of csrc/mi_sim.hip (a view that adds a
kernel must leave every other kernel's instructions alone).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -S --cuda-device-only \\
        omniisaacgymenvs_amd/csrc/mi_sim.hip -o new.s        # likewise parent.s in a parent checkout
    python tools/isa_identity.py parent.s new.s [--out profiles/<view>/isa_identity.txt]

The assembly is split per function with tools/isa_ops.py's `kernels()`; comments are dropped, local
labels (.LBB<n>_, .Ltmp<n>, .Lfunc_end<n>) renumbered, and the compiler's resource summary (NumVgprs,
NumAgprs, NumSgprs, ScratchSize, LDSByteSize, codeLenInByte, Occupancy) kept. Exit status 1 when a
kernel of the parent differs or is missing."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_ops import kernels  # noqa: E402

KEEP = ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "LDSByteSize", "codeLenInByte", "Occupancy")


def normalised(path):
    out = {}
    for name, body, trailer in kernels(open(path).read()):
        ids = {}

        def label(m):
            return f"{m.group(1)}{ids.setdefault(m.group(0), len(ids))}"

        lines = []
        for ln in body:
            ln = ln.split(";")[0].rstrip()
            if ln.strip():
                lines.append(re.sub(r"(\.LBB|\.Ltmp|\.Lfunc_end|\.Lfunc_begin)\d+(?:_\d+)?", label, ln))
        res = [ln.strip() for ln in trailer if any(re.match(rf";\s*{k}:", ln.strip()) for k in KEEP)]
        out[name] = (lines[1:], res)        # the first line carries the function's own label
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a, b = normalised(args.parent), normalised(args.new)
    same = [k for k in a if k in b and a[k] == b[k]]
    differ = [k for k in a if k in b and a[k] != b[k]]
    missing = [k for k in a if k not in b]
    added = [k for k in b if k not in a]
    text = (f"parent functions {len(a)}, new {len(b)}; identical instruction streams and resource lines: "
            f"{len(same)}; differing: {len(differ)}{' ' + ' '.join(differ) if differ else ''};\n"
            f"missing in new: {' '.join(missing) if missing else 'none'}; added: {' '.join(added) if added else 'none'}\n")
    for k in added:
        text += f"{k}: {' '.join(b[k][1])}\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(__doc__.split("\n\n")[2].replace("\n", " ").strip() + "\n\n" + text)
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main())
