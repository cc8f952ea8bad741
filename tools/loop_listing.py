"""Instruction counts of a kernel's loops in a gfx950 assembly listing.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math \
      --cuda-device-only -S -o k.s compression_without_quantization_amd/csrc/cwq_kernels.hip
  python tools/loop_listing.py k.s k_encode_pruneILi32ELb1ELb0ELb1E [--blocks] [--all]

Instructions are classed by their prefix only: s_ scalar, v_ vector, ds_ LDS,
anything else "other".  A loop is a backward branch and the blocks from its
target to it; loops that hold another loop are left out.  For every loop the script prints the instructions in its range,
the lane moves and scratch accesses in it (there should be none), and the
fall-through path from the loop's head: no conditional branch taken, plain
branches followed, up to the first branch back to the head; in an unrolled loop it spans every
copy of the body, so divide by their number.  With the rare
branches placed out of line that path is the common one; --blocks prints each
block of the range with its counts and its branches, so that the path can be
checked and others summed by hand.  --all runs over every instance whose name
contains the given text and prints one line each: registers, scratch, and the
lane moves / scratch accesses inside loops.
"""
import re
import sys

LANE = ("v_readlane", "v_writelane")


def klass(op):
    if op.startswith("s_"):
        return "s"
    if op.startswith("v_"):
        return "v"
    if op.startswith("ds_"):
        return "lds"
    return "other"


def functions(path, want):
    """{name: lines} of the functions whose name contains `want`."""
    out, name, cur = {}, None, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            if want in m.group(1):
                name, cur = m.group(1), []
            continue
        if name is not None:
            cur.append(ln.rstrip("\n"))
            if ln.startswith("; Occupancy"):  # the last line of the kernel's resource comments
                out[name] = cur
                name = None
    return out


def meta(lines):
    d = {}
    for ln in lines:
        m = re.match(r";\s*(TotalNumSgprs|NumVgprs|ScratchSize|Occupancy|codeLenInByte)\s*[:=]\s*(\d+)", ln.strip())
        if m:
            d[m.group(1)] = int(m.group(2))
    return d


def blocks(lines):
    """[(label, [(op, operands)])] in layout order; the entry block is 'entry'."""
    bl = [("entry", [])]
    for ln in lines:
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            bl.append((m.group(1), []))
            continue
        if ln.startswith(".Lfunc_end"):
            break
        m = re.match(r"^\t([a-z_0-9]+)\s*(.*?)\s*(;.*)?$", ln)
        if m and not ln.startswith("\t."):
            bl[-1][1].append((m.group(1), m.group(2)))
    return bl


def counts(ins):
    c = {"s": 0, "v": 0, "lds": 0, "other": 0, "lane": 0, "scratch": 0}
    for op, _ in ins:
        c[klass(op)] += 1
        if op.startswith(LANE):
            c["lane"] += 1
        if op.startswith("scratch_"):
            c["scratch"] += 1
    return c


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def loops(bl):
    """[(head, last)]: a backward branch closes a loop when its target reaches
    it going forward (an out-of-line arm that branches back into the next copy
    of an unrolled body does not); one loop per head, the innermost only."""
    idx = {lab: i for i, (lab, _) in enumerate(bl)}
    succ = []
    for i, (_, ins) in enumerate(bl):
        t = {idx[arg] for op, arg in ins if op.startswith(("s_cbranch", "s_branch")) and arg in idx}
        if not (ins and ins[-1][0] in ("s_branch", "s_endpgm")):
            t.add(i + 1)
        succ.append(t)
    by_head = {}
    for i in range(len(bl)):
        for h in succ[i]:
            if h > i:
                continue
            seen, todo = {h}, [h]
            while todo:
                for n in succ[todo.pop()]:
                    if h < n <= i and n not in seen:
                        seen.add(n)
                        todo.append(n)
            if i in seen:
                by_head[h] = max(i, by_head.get(h, i))
    lp = sorted(by_head.items())
    inner = [(h, l) for h, l in lp if not any((h2, l2) != (h, l) and h <= h2 and l2 <= l for h2, l2 in lp)]
    return inner, idx


def is_scoring(ins_lists):
    """The screening and exact loops: at most 260 vector instructions per
    Philox block (18 or 19 v_mad_u64_u32: ten rounds of two, less the
    products whose high word nothing reads); the survivors' row scoring has more."""
    ops = [op for ins in ins_lists for op, _ in ins]
    mads = sum(op.startswith("v_mad_u64_u32") for op in ops)
    v = sum(klass(op) == "v" for op in ops)
    return mads >= 18 and v * 18 <= 260 * mads


def fall_path(bl, idx, head, last):
    """Blocks of the path from `head` that takes no conditional branch."""
    path, i, taken, seen = [], head, 0, set()
    while i not in seen and head <= i < len(bl):
        seen.add(i)
        path.append(i)
        nxt = i + 1
        for op, arg in bl[i][1]:
            if op == "s_branch" and arg in idx:
                nxt = idx[arg]
                taken += 1
        if nxt == head:
            return path, taken, True
        # a conditional branch at the end of the range that closes the loop
        ends = [arg for op, arg in bl[i][1] if op.startswith("s_cbranch") and arg in idx and idx[arg] == head]
        if i == last and ends:
            return path, taken + 1, True
        i = nxt
    return path, taken, False


def report(name, lines, show_blocks):
    md = meta(lines)
    bl = blocks(lines)
    lp, idx = loops(bl)
    print(name)
    print("  " + "  ".join("%s %d" % kv for kv in sorted(md.items())))
    for head, last in lp:
        tot = {"s": 0, "v": 0, "lds": 0, "other": 0, "lane": 0, "scratch": 0}
        for i in range(head, last + 1):
            tot = add(tot, counts(bl[i][1]))
        if not is_scoring([bl[i][1] for i in range(head, last + 1)]):
            continue
        path, taken, closed = fall_path(bl, idx, head, last)
        pc = {"s": 0, "v": 0, "lds": 0, "other": 0, "lane": 0, "scratch": 0}
        for i in path:
            pc = add(pc, counts(bl[i][1]))
        print("  loop %s .. %s: %d blocks, s %d v %d lds %d other %d; lane moves %d, scratch %d"
              % (bl[head][0], bl[last][0], last - head + 1, tot["s"], tot["v"], tot["lds"],
                 tot["other"], tot["lane"], tot["scratch"]))
        print("    fall-through path%s: %d blocks, s %d v %d lds %d other %d, branches taken %d"
              % ("" if closed else " (does not close)", len(path), pc["s"], pc["v"], pc["lds"],
                 pc["other"], taken))
        if show_blocks:
            for i in range(head, last + 1):
                c = counts(bl[i][1])
                br = ["%s %s" % (op, arg) for op, arg in bl[i][1] if op.startswith(("s_cbranch", "s_branch"))]
                print("      %-14s s %3d v %3d lds %2d other %2d%s  %s"
                      % (bl[i][0], c["s"], c["v"], c["lds"], c["other"],
                         " *" if i in path else "  ", "; ".join(br)))


def summary(name, lines):
    md = meta(lines)
    bl = blocks(lines)
    lp, _ = loops(bl)
    lane = scr = 0
    for head, last in lp:
        tot = {"s": 0, "v": 0, "lds": 0, "other": 0, "lane": 0, "scratch": 0}
        for i in range(head, last + 1):
            tot = add(tot, counts(bl[i][1]))
        if is_scoring([bl[i][1] for i in range(head, last + 1)]):
            lane += tot["lane"]
            scr += tot["scratch"]
    m = re.search(r"k_encode_prune\w*?(I\w+?E)Ev", name)
    print("%-28s vgpr %3d sgpr %3d scratch %3d occ %d code %6d  loops: lane moves %d scratch %d"
          % (m.group(1) if m else name, md.get("NumVgprs", -1), md.get("TotalNumSgprs", -1),
             md.get("ScratchSize", -1), md.get("Occupancy", -1), md.get("codeLenInByte", -1), lane, scr))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path, want = args[0], args[1]
    fs = functions(path, want)
    if not fs:
        sys.exit("no function named *%s* in %s" % (want, path))
    for name, lines in fs.items():
        if "--all" in sys.argv:
            summary(name, lines)
        else:
            report(name, lines, "--blocks" in sys.argv)


if __name__ == "__main__":
    main()
