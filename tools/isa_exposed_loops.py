"""Innermost rolled loops of one kernel in a `hipcc -S -gline-tables-only` listing, with what one trip waits for: per loop the source lines it was compiled from,
and its memory instructions and s_waitcnt's in program order.  A loop whose trip is `load, wait, add` pays one memory round trip per addend; a batched loop shows
its loads back to back and one wait per chunk.

    usage: python tools/isa_exposed_loops.py FILE.s kernel-substring [source-file-substring [first-line last-line]]

The optional source filter keeps the loops with at least one instruction from that file (and line range).  Identical loops (same source lines, same sequence) are one row with their count.  Listing: the build line of mjh_inst.hip with
`-gline-tables-only -S --cuda-device-only -DMJH_INST_GROUP=g -DMJH_INST_REAL=double|float` (tools/kbuild.sh shows the flags)."""
import collections
import re
import sys

MEM = ("ds_", "global_load", "global_store", "global_atomic", "buffer_", "flat_", "scratch_", "s_load", "s_buffer_load")


def loops_of(text, i0, i1):
    labels = {}
    for i in range(i0, i1):
        m = re.match(r"^(\.LBB\w+):", text[i])
        if m:
            labels[m.group(1)] = i
    loops = []
    for i in range(i0, i1):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\w+)", text[i])
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    return [(a, b) for a, b in loops if not any((a2, b2) != (a, b) and a <= a2 and b2 <= b for a2, b2 in loops)]  # innermost only


def main():
    text = open(sys.argv[1]).read().split("\n")
    want = sys.argv[2]
    src = sys.argv[3] if len(sys.argv) > 3 else ""
    lo, hi = (int(sys.argv[4]), int(sys.argv[5])) if len(sys.argv) > 5 else (0, 1 << 30)
    starts = [(i, ln.split(":")[0]) for i, ln in enumerate(text) if re.match(r"^_Z\w+:", ln)]
    for n, (i0, name) in enumerate(starts):
        if want not in name:
            continue
        i1 = starts[n + 1][0] if n + 1 < len(starts) else len(text)
        inner = loops_of(text, i0, i1)
        shown = waits_per_trip = 0
        rows = []
        seen = {}
        for a, b in sorted(inner):
            where = collections.Counter()
            seq = []
            cur = None
            for ln in text[a:b + 1]:
                m = re.match(r"^\s+\.loc\s+\d+\s+(\d+)\s+\d+.*;\s*(\S+?):\d+:\d+", ln)
                if m:
                    cur = (m.group(2).split("/")[-1], int(m.group(1)))
                    continue
                if not ln.startswith("\t") or ln.strip().startswith((";", ".")):
                    continue
                op = ln.split()[0]
                if cur:
                    where[cur] += 1
                if op.startswith("s_waitcnt"):
                    seq.append("WAIT " + " ".join(ln.split(";")[0].split()[1:]))
                elif op.startswith(MEM):
                    seq.append(op)
            if src and not any(src in f and lo <= line <= hi for f, line in where):
                continue
            nwait = sum(1 for s in seq if s.startswith("WAIT"))
            nmem = len(seq) - nwait
            if nwait == 0 or nmem == 0:
                continue
            shown += 1
            waits_per_trip += nwait
            top = ", ".join(f"{f}:{line}" for (f, line), _ in where.most_common(3))
            # runs of the same instruction are folded: "8 x ds_read_b64"
            folded = []
            for s in seq:
                if folded and folded[-1][0] == s:
                    folded[-1][1] += 1
                else:
                    folded.append([s, 1])
            body = f"mem={nmem:3d} waits={nwait:2d}  [{top}]\n      " + "  ".join(s if c == 1 else f"{c} x {s}" for s, c in folded)
            if body in seen:  # the kernel holds several copies of a stage (its two stage orders, unrolled outer trips): one row per distinct loop
                seen[body][1] += 1
            else:
                seen[body] = [f"  L{a - i0:6d}..{b - i0:6d}", 1]
                rows.append(body)
        print(f"{name}: {len(inner)} innermost rolled loops, {shown} of them with memory instructions and waits in the trip" + (f" from {src} {lo}..{hi}" if src else "") + f", {waits_per_trip} waits over one trip of each")
        print("\n".join(f"{seen[r][0]}  copies={seen[r][1]:2d}  {r}" for r in rows))


if __name__ == "__main__":
    main()
