#!/usr/bin/env python3
"""tools/k3w_loop_count.py FILE.s -- static instruction counts of k3w_pass's unit loop in a device assembly file.

  cd grav1synth_amd/csrc && hipcc --offload-arch=gfx950 $(CXXFLAGS of the Makefile) --cuda-device-only -S \
      -Rpass-analysis=kernel-resource-usage -o engine.s engine.hip 2> engine.remarks

For k3w_pass<0, 2, 1, 1, 2, false> and <1, 2, 1, 1, 2, false> (the 4K 10-bit 4:2:0 job's two launches): every loop at depth 1 that
holds a matrix instruction, counted over the blocks the assembly's own comments put in the loop ("in Loop: Header=").  Every path
of the loop is counted once, the cold ones too (edge units, the masked multiplies, a residual outside int8): a count is
comparable between two builds, it is not what one wave issues an iteration."""
import collections
import re
import sys

PAT = re.compile(r"^_ZN3g1s8k3w_passILi([01])ELi2ELi1ELi1ELi2ELb0EEEvNS_4GeomENS_7WParamsE:")


def classify(c, line):
    t = line.strip().split()
    if not t or t[0].startswith((".", ";")) or t[0].endswith(":"):
        return
    op = t[0]
    if op.startswith("v_mfma"):
        c["mfma"] += 1
    elif op.startswith(("v_readfirstlane", "v_readlane")):
        c["v_readfirstlane"] += 1
    elif op.startswith("v_mov_b64"):
        c["v_mov_b64"] += 1
        c["VALU"] += 1
    elif op.startswith("v_mov_b32"):
        c["v_mov_dpp" if "row_" in line else "v_mov_b32"] += 1
        c["VALU"] += 1
    elif op.startswith("v_"):
        c["VALU"] += 1
    elif op.startswith("ds_"):
        c["LDS"] += 1
    elif op.startswith(("buffer_", "global_", "flat_")):
        c["VMEM"] += 1
    elif op.startswith("s_waitcnt"):
        c["s_waitcnt"] += 1
    elif op.startswith("s_barrier"):
        c["s_barrier"] += 1
    elif op.startswith(("s_cbranch", "s_branch")):
        c["branch"] += 1
    elif op.startswith("s_nop"):
        c["s_nop"] += 1
    elif op.startswith("s_"):
        c["SALU"] += 1


def main():
    src = open(sys.argv[1]).read().split("\n")
    for i, first in enumerate(src):
        m = PAT.match(first)
        if not m:
            continue
        end = i
        while not src[end].strip().startswith("s_endpgm"):
            end += 1
        body = src[i:end + 1]
        loops = collections.defaultdict(collections.Counter)
        cur = None
        for b in body:
            lab = re.match(r"^\.LBB(\d+_\d+):", b)
            if lab or b.strip().startswith("; %bb."):
                h = re.search(r"(?:in Loop: Header=|Parent Loop )BB(\d+_\d+)", b)
                cur = h.group(1) if h else (lab.group(1) if lab and "Loop Header: Depth=1" in b else None)
                continue
            if cur:
                classify(loops[cur], b)
        name = f"k3w_pass<{m.group(1)}, 2, 1, 1, 2, false>"
        for k, c in loops.items():
            if c["mfma"]:
                print(name, f"loop BB{k}:", "  ".join(f"{a} {n}" for a, n in sorted(c.items())))
        print(name, "instructions in the kernel:", sum(1 for b in body if b.startswith("\t") and not b.strip().startswith((".", ";"))))


if __name__ == "__main__":
    main()
