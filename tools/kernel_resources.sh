#!/bin/bash
# kernel_resources.sh [extra -D flags] -- register / scratch use of every kernel of kernels.hip as the compiler reports it
# (no GPU needed): VGPRs, SGPRs, scratch bytes per lane, waves per SIMD.  RDX_KERNEL_SOURCE=shade.hip: another unit of csrc/
cd "$(dirname "$0")/../radiance-ray-tracing_amd/csrc"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -x hip -c "${RDX_KERNEL_SOURCE:-kernels.hip}" -o /dev/null \
  -Rpass-analysis=kernel-resource-usage "$@" 2>&1 | python3 -c '
import re, sys, subprocess
rows, cur = [], {}
for line in sys.stdin:
    m = re.search(r"remark: (?:[^ ]+:\d+:\d+: )?(.*?)(?: \[-Rpass-analysis=kernel-resource-usage\])?$", line.rstrip())
    if not m: continue
    t = m.group(1).strip()
    if t.startswith("Function Name:"):
        cur = {"name": t.split(":", 1)[1].strip()}
    for k, key in (("VGPRs:", "v"), ("SGPRs:", "s"), ("ScratchSize [bytes/lane]:", "scr"), ("Occupancy [waves/SIMD]:", "occ")):
        if t.startswith(k): cur[key] = t.split(":", 1)[1].strip()
    if t.startswith("LDS Size") and "name" in cur:
        rows.append(cur); cur = {}
names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.split("\n")
for r, n in sorted(zip(rows, names), key=lambda x: x[1]):
    n = re.sub(r"\(.*", "", n.replace("rdx::", "").replace("void ", ""))
    print("%-44s vgpr %-4s sgpr %-4s scratch %-4s waves/SIMD %s" % (n[:44], r.get("v"), r.get("s"), r.get("scr"), r.get("occ")))
'
