#!/usr/bin/env python
"""Static check of the LDS / scalar-load waits of the evaluation loop of a k_quad instantiation in the compiler's assembly:
    python tools/kquad_asm.py anymal && python tools/loop_wait_check.py /tmp/kq_anymal.s [kernel substring] [-v]
Companion of tools/output_pass_check.py.  It walks the basic blocks of the largest loop of the kernel (the blocks LLVM
marks `in Loop: Header=...`, as tools/loop_stats.py does).  LDS operations and scalar loads count on one counter
(lgkmcnt); LDS operations return in order, so `s_waitcnt lgkmcnt(n)` waits for everything but the n youngest operations
in flight.  For every such wait the tool reports the class of the YOUNGEST operation it waits for (LDS read, LDS write,
scalar load) and the number of VALU instructions issued between that operation and the wait: the cover the wave gives
the latency by itself.  Only operations issued in the wait's own basic block are seen; a wait that finds none in flight
(its operations were issued in an earlier block) is listed as `earlier block`.  A scalar load returns out of order:
while one is in flight only lgkmcnt(0) is possible, and it drains every LDS read behind it as well -- those waits are
listed as `+smem`.

Summary line: the waits on reads (LDS reads and scalar loads) and how many sit below 8, 16 and 32 VALU instructions.
Exit status 1 when a wait inside the loop involves a scalar load, or when an LDS-read wait has fewer than 16 VALU
instructions of cover in a block that holds 16 or more (-v lists every wait; --allow N tolerates N such waits)."""
import re
import sys

NEAR = (8, 16, 32)


def functions(text):
    for m in re.finditer(r"; -- Begin function (\S+)\n(.*?); -- End function", text, re.S):
        yield m.group(1), m.group(2)


def loop_blocks(body):
    """[(label, header, [(line number in body, text)])] of the blocks of every loop"""
    blocks, cur = [], None
    for n, line in enumerate(body.splitlines()):
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", line)
        if m:
            cur = None
            c = m.group(2) or ""
            head = None
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", c)
            if h: head = h.group(1)
            if re.search(r"=>This .*Loop Header", c): head = m.group(1)[2:]
            if head is not None:
                cur = (m.group(1), head, [])
                blocks.append(cur)
            continue
        if cur is not None:
            cur[2].append((n, line))
    return blocks


def op_class(op):
    if op.startswith("ds_"):
        return "lds write" if ("write" in op or "store" in op) else "lds read"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "scalar load"
    return None


def block_waits(lines):
    """waits of one basic block: [(line, class, VALU between, involves a scalar load, text)], and the block's VALU count"""
    flight = []      # (class, VALU count at issue), oldest first
    valu = 0
    out = []
    for n, line in lines:
        m = re.match(r"^\t([a-z_0-9]+)\b(.*)", line)
        if not m or line.startswith("\t."):
            continue
        op, rest = m.group(1), m.group(2)
        if op.startswith("v_"):
            valu += 1
            continue
        c = op_class(op)
        if c is not None:
            flight.append((c, valu))
            continue
        if op != "s_waitcnt":
            continue
        w = re.search(r"lgkmcnt\((\d+)\)", rest)
        if not w:
            continue
        keep = int(w.group(1))
        smem = any(f[0] == "scalar load" for f in flight)
        if smem:
            keep = 0          # (out-of-order returns: the counter can only be waited down to zero)
        done = flight[:len(flight) - keep] if keep else flight
        if not done:
            out.append((n, "earlier block", -1, False, line.strip()))
        else:
            young = done[-1]
            cls = young[0]
            if smem and cls != "scalar load":
                cls += " +smem"
            out.append((n, cls, valu - young[1], smem, line.strip()))
        flight = flight[len(done):]
    return out, valu


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    verbose = "-v" in sys.argv
    allow = int(sys.argv[sys.argv.index("--allow") + 1]) if "--allow" in sys.argv else 0
    if "--allow" in sys.argv:
        args.remove(str(allow))
    text = open(args[0]).read()
    like = args[1] if len(args) > 1 else "k_quad"
    bad = 0
    for name, body in functions(text):
        if like not in name:
            continue
        blocks = loop_blocks(body)
        if not blocks:
            continue
        size = {}
        for _, head, lines in blocks:
            size[head] = size.get(head, 0) + len(lines)
        top = max(size, key=size.get)
        print(f"# {name[:100]}: loop {top}")
        waits = []
        for label, head, lines in blocks:
            if head != top:
                continue
            w, nvalu = block_waits(lines)
            waits += [(label, nvalu) + x for x in w]
        reads = [x for x in waits if x[3].startswith("lds read") or x[3].startswith("scalar load")]
        smem = [x for x in waits if x[5]]
        for x in waits:
            short = x in reads and x[4] < 16
            if verbose or short or x[5]:
                print(f"  {x[0]:12s} (VALU {x[1]:4d}) line {x[2] + 1:6d}  {x[3]:18s} {x[4]:4d} VALU behind   {x[6]}")
        by_class = {}
        for x in waits:
            by_class[x[3]] = by_class.get(x[3], 0) + 1
        print(f"  lgkmcnt waits in the loop: {len(waits)}  {by_class}")
        print(f"  waits on reads: {len(reads)}; " + ", ".join(f"below {n}: {sum(x[4] < n for x in reads)}" for n in NEAR)
              + f"; waits that involve a scalar load: {len(smem)}"
              + (f" ({min(x[4] for x in smem)}-{max(x[4] for x in smem)} VALU behind)" if smem else ""))
        # a block with fewer than 16 VALU instructions in all cannot cover a read issued in it
        exposed = [x for x in reads if not x[5] and x[4] < 16 and x[1] >= 16]
        print(f"  LDS-read waits below 16 VALU in blocks of 16 or more: {len(exposed)}")
        bad += len(smem) + max(0, len(exposed) - allow)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
