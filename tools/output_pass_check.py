#!/usr/bin/env python
"""Static check of the output pass of a k_quad instantiation in the compiler's assembly:
    python tools/kquad_asm.py anymal && python tools/output_pass_check.py /tmp/kq_anymal.s
The pass starts at the comment JM_OUTPUT_PASS_BEGIN leaves in the assembly (jm_quad.h) and runs to the end of the program.
Reported: private-memory (spill) instructions inside the pass, and the waits on the vector-memory counter that sit
between its first and its last global store -- such a wait also waits for every store issued before it.  Exit status 1
when either list is not empty."""
import re
import sys

MARK = "quad output pass"


def main():
    lines = open(sys.argv[1]).read().split("\n")
    marks = [i for i, l in enumerate(lines) if MARK in l]
    if not marks:
        sys.exit(f"no '{MARK}' marker in {sys.argv[1]}")
    start = marks[-1]
    end = max(i for i, l in enumerate(lines) if "s_endpgm" in l)
    # The block that holds the marker is laid out in front of the evaluation loop and ends in a branch to the rest of the
    # pass, which follows the loop: the region is that block plus everything from the branch target on.
    head_end = start
    for i in range(start, end):
        m = re.match(r"\s*s_branch (\S+)", lines[i])
        if m:
            tgt = lines.index(m.group(1) + ":")
            if tgt > i:
                head_end, start2 = i, tgt
                break
    else:
        head_end, start2 = end, end
    region = list(range(start, head_end + 1)) + [i for i in range(start2, end + 1) if i > head_end]
    spill = [(i + 1, lines[i].strip()) for i in region if re.search(r"\bscratch_(load|store)", lines[i])]
    stores = [i for i in region if "global_store" in lines[i] or "global_atomic" in lines[i]]
    waits = [(i + 1, lines[i].strip()) for i in region
             if "vmcnt" in lines[i] and stores and stores[0] < i < stores[-1]]
    loads = [(i + 1, lines[i].strip()) for i in region if "global_load" in lines[i]]
    print(f"output pass: lines {start + 1}..{head_end + 1} and {start2 + 1}..{end + 1}; {len(stores)} global stores, "
          f"first at {stores[0] + 1 if stores else '-'}, last at {stores[-1] + 1 if stores else '-'}")
    print(f"private-memory instructions in the pass: {len(spill)}")
    for x in spill:
        print("   ", *x)
    print(f"vmcnt waits between the first and the last store: {len(waits)}")
    for x in waits:
        print("   ", *x)
    print(f"global loads in the pass: {len(loads)}")
    for x in loads:
        print("   ", *x)
    sys.exit(1 if spill or waits else 0)


if __name__ == "__main__":
    main()
