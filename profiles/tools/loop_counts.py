#!/usr/bin/env python3
"""Static instruction counts of the loops of one kernel, from the loop comments the compiler leaves in its assembly:

    hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only csrc/vpt_k1_volpath.hip -o volpath.s
    python profiles/tools/loop_counts.py volpath.s 'vpt_mesh_kernelILi0ELb0ELi4E' [--blocks HEADER]

One line per loop: header label, depth, parent loop, instructions in the loop's own blocks and with its child loops, and what tells
the loops of traverse() apart: global loads (dword / wider), LDS reads and writes, DPP moves, bpermutes.  In vpt_mesh_kernel the group
form of the node phase is the loop with eight global_load_dword and the quad_perm moves, its pop loop the child with one ds_read; the own
form's leaf walk is the loop with four global_load_dwordx3 (x4 with points and lines).  The own node step is no loop of its own: it is
the block of the query loop with seven global_load_dwordx4.  --blocks HEADER lists the blocks of one loop with their counts, to read a
common path off (the blocks a step goes through)."""
import re
import sys


def kernel_lines(path, name):
    lines, inside = [], False
    for line in open(path):
        if not inside:
            inside = re.match(r"^_Z\w*:", line) is not None and name in line
            continue
        if line.startswith(".Lfunc_end"):
            break
        lines.append(line.rstrip("\n"))
    if not lines:
        sys.exit(f"no kernel matching {name!r} in {path}")
    return lines


def is_instruction(line):
    s = line.strip()
    return bool(s) and not s.startswith((";", ".", "//")) and not s.endswith(":") and not re.match(r"^\.?\w+:", s)


def main():
    path, name = sys.argv[1], sys.argv[2]
    want = sys.argv[sys.argv.index("--blocks") + 1] if "--blocks" in sys.argv else None
    blocks, cur = [], {"label": "entry", "header": None, "depth": 0, "lines": []}
    lines = kernel_lines(path, name)
    for i, line in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):\s*;\s*(.*)", line) or re.match(r"^; %bb\.(\d+):\s*;?\s*(.*)", line)
        if m:
            blocks.append(cur)
            label, note = m.group(1), m.group(2)
            cur = {"label": re.sub(r"^\.L", "", label), "header": None, "depth": 0, "lines": [], "parent": None}
            # a loop header's own comment spans several lines: "Parent Loop BBx Depth=n" ... "=> This (Inner) Loop Header: Depth=n"
            notes = [note]
            for l in lines[i + 1:]:
                if not l.lstrip().startswith(";") or "Loop" not in l:
                    break
                notes.append(l)
            for n in notes:
                h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", n)
                if h:
                    cur["header"], cur["depth"] = h.group(1), int(h.group(2))
                p = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", n)
                if p:
                    cur["parent"] = p.group(1)   # the last one named is the innermost parent
                t = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", n)
                if t:
                    cur["header"], cur["depth"] = cur["label"], int(t.group(1))
            continue
        if is_instruction(line):
            cur["lines"].append(line.strip())
    blocks.append(cur)
    loops = {}
    for b in blocks:
        if b["header"]:
            l = loops.setdefault(b["header"], {"depth": b["depth"], "parent": None, "blocks": []})
            l["blocks"].append(b)
            if b["label"] == b["header"]:
                l["parent"] = b.get("parent")
    if want:
        for b in loops[want]["blocks"]:
            print(f"{b['label']:12s} {len(b['lines']):4d}")
        return

    def own(h):
        return [x for b in loops[h]["blocks"] for x in b["lines"]]

    def total(h):
        return len(own(h)) + sum(total(c) for c in loops if loops[c]["parent"] == h)

    print(f"{'loop':12s} depth {'parent':12s}  own  with children   gl.dword gl.wide ds_read ds_write dpp bpermute")
    for h, l in loops.items():
        ins = own(h)
        count = lambda pat: sum(1 for x in ins if re.match(pat, x))   # noqa: E731
        print(f"{h:12s} {l['depth']:5d} {str(l['parent']):12s} {len(ins):4d} {total(h):14d}   {count(r'global_load_dword '):8d} {count(r'global_load_dwordx'):7d} "
              f"{count(r'ds_read'):7d} {count(r'ds_write'):8d} {sum(1 for x in ins if 'quad_perm' in x):3d} {count(r'ds_bpermute'):8d}")


if __name__ == "__main__":
    main()
