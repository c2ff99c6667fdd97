#!/usr/bin/env python3
"""Register / scratch / LDS budget of every vpt_* kernel as the compiler reports it:

    python profiles/tools/kernel_resources.py [extra hipcc flags ...]

Compiles every HIP unit of libvpt_hip.so for gfx950 - the commands the Makefile runs (`make -n`), with
-Rpass-analysis=kernel-resource-usage and the objects written to a temporary directory (no GPU needed) - and prints
one line per kernel of ours, sorted by name (rocPRIM's sort kernels are skipped)."""
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "volumetric-path-tracer_amd")


def compile_commands(outdir):
    """the Makefile's compile command of every object of libvpt_hip.so, writing into outdir"""
    plan = subprocess.run(["make", "-n", "-B", "libvpt_hip.so"], cwd=PKG, stdout=subprocess.PIPE, text=True, check=True).stdout
    cmds = []
    for line in plan.splitlines():
        args = shlex.split(line)
        if "-c" not in args or "-o" not in args:
            continue
        o = args.index("-o")
        args[o + 1] = os.path.join(outdir, os.path.basename(args[o + 1]))
        cmds.append(args + ["-Rpass-analysis=kernel-resource-usage"] + sys.argv[1:])
    return cmds


def remarks(cmd):
    return subprocess.run(cmd, cwd=PKG, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True).stderr


def main():
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        errs = list(pool.map(remarks, compile_commands(tmp)))
    rows = []
    for err in errs:
        cur = None
        for line in err.splitlines():
            m = re.search(r"remark: [^:]*:\d+:\d+: +(\w[\w \[\]/]*): +(\S+)", line) or re.search(r"remark: +(\w[\w \[\]/]*): +(\S+)", line)
            if not m:
                m = re.search(r":\d+:\d+: +([A-Za-z][\w \[\]/]*): +(\S+) \[-Rpass-analysis", line)
            if not m:
                continue
            key, val = m.group(1).strip(), m.group(2)
            if key in ("Function Name", "Name"):
                cur = {"name": val}
                rows.append(cur)
            elif cur is not None:
                cur[key] = val
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    lines = []
    for r, name in zip(rows, names):
        if "rocprim" in name:
            continue
        short = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", ""))   # kernels of an unnamed namespace keep their names
        lines.append(f"{short:55s} VGPR {r.get('VGPRs', '?'):>4} AGPR {r.get('AGPRs', '?'):>3} SGPR {r.get('TotalSGPRs', r.get('SGPRs', '?')):>4} "
                     f"scratch {r.get('ScratchSize [bytes/lane]', '?'):>5} B/lane  occupancy {r.get('Occupancy [waves/SIMD]', '?')}  LDS {r.get('LDS Size [bytes/block]', '?')}")
    print("\n".join(sorted(lines)))


if __name__ == "__main__":
    main()
