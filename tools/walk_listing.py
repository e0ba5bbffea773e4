#!/usr/bin/env python3
"""Instruction classes per basic block of ONE kernel, from its listing (hipcc -S, device only, gfx950, the Makefile's flags).
For every block of the kernel: vector ALU, scalar ALU, scalar loads, branches, waits / no-ops, LDS, vector memory and whatever is
left, and whether the block lies on a cycle of the kernel's control-flow graph ("loop").  Classes are told apart by the
mnemonic's prefix; no particular instruction is looked for.
usage: tools/walk_listing.py query_kernels.hip <mangled kernel name> [--tree DIR] [--keep listing.s]
  --tree DIR: another checkout of this repository (its icon_amd/csrc is compiled); --keep: also write the kernel's listing."""
import argparse, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("valu", "salu", "smem", "branch", "wait", "lds", "vmem", "other")


def makefile_flags(csrc, src):
    """COMMON (+ EXACT where the unit's rule has it) as icon_amd/csrc/Makefile states them"""
    text = open(os.path.join(csrc, "Makefile")).read()
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
    obj = os.path.splitext(src)[0] + ".o"
    rule = re.search(r"^%s:.*\n\t(.*)$" % re.escape(obj), text, re.M)
    if not rule:
        sys.exit(f"{src}: no rule for {obj} in the Makefile")
    flags = expand(expand(rule.group(1))).split()
    hipcc = flags[0]
    keep = [f for f in flags[1:] if f not in ("-c", "$<", "-o", "$@")]
    return hipcc, keep


def listing(csrc, src):
    hipcc, flags = makefile_flags(csrc, src)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "x.s")
        cmd = [hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(csrc, src), "-o", out]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode:
            sys.exit(p.stdout[-3000:])
        return open(out).read()


def kernel_body(text, name):
    lines = text.splitlines()
    try:
        a = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    except StopIteration:
        names = sorted(set(re.findall(r"^(_Z\w+):", text, re.M)))
        sys.exit(f"no kernel {name}; the unit has:\n  " + "\n  ".join(names))
    b = next(i for i in range(a, len(lines)) if lines[i].strip().startswith(".end_amdhsa_kernel") or lines[i].strip().startswith(".Lfunc_end"))
    return lines[a + 1:b]


def classify(mn):
    if mn.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_endpgm")):
        return "branch"
    if mn.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier")):
        return "wait"
    if mn.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith("v_"):
        return "valu"
    return "other"


def blocks(body):
    """[(label, counts, targets, falls_through)]"""
    out, cur = [], {"label": "entry", "n": dict.fromkeys(CLASSES, 0), "to": [], "fall": True}
    for raw in body:
        line = raw.split(";")[0].strip()
        if not line or line.startswith("."):
            # a block starts at its label, or - a block only ever fallen into - at the assembler's "; %bb.N:" remark
            m = re.match(r"^(\.LBB\d+_\d+):", line) or re.match(r"^; (%bb\.\d+):", raw.strip())
            if m:
                out.append(cur)
                cur = {"label": m.group(1), "n": dict.fromkeys(CLASSES, 0), "to": [], "fall": True}
            continue
        mn = line.split()[0]
        cur["n"][classify(mn)] += 1
        if mn.startswith(("s_cbranch", "s_branch")):
            cur["to"].append(line.split()[-1])
            if mn.startswith("s_branch"):
                cur["fall"] = False
        if mn.startswith("s_endpgm"):
            cur["fall"] = False
    out.append(cur)
    return out


def on_cycle(bl):
    idx = {b["label"]: i for i, b in enumerate(bl)}
    succ = [[idx[t] for t in b["to"] if t in idx] + ([i + 1] if b["fall"] and i + 1 < len(bl) else []) for i, b in enumerate(bl)]

    def reach(src):
        seen, todo = set(), list(succ[src])
        while todo:
            v = todo.pop()
            if v not in seen:
                seen.add(v); todo.extend(succ[v])
        return seen
    return [i in reach(i) for i in range(len(bl))], succ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src"); ap.add_argument("kernel"); ap.add_argument("--tree", default=ROOT); ap.add_argument("--keep")
    a = ap.parse_args()
    body = kernel_body(listing(os.path.join(a.tree, "icon_amd", "csrc"), a.src), a.kernel)
    if a.keep:
        open(a.keep, "w").write("\n".join(body) + "\n")
    bl = blocks(body)
    loop, succ = on_cycle(bl)
    print(f"# {a.kernel}  ({a.src})")
    print(f"{'block':12s} {'loop':4s} " + " ".join(f"{c:>6s}" for c in CLASSES) + "  -> successors")
    tot = dict.fromkeys(CLASSES, 0)
    for i, b in enumerate(bl):
        if loop[i]:
            for c in CLASSES:
                tot[c] += b["n"][c]
        print(f"{b['label']:12s} {'*' if loop[i] else '':4s} " + " ".join(f"{b['n'][c]:6d}" for c in CLASSES) + "  -> " + " ".join(bl[j]["label"] for j in succ[i]))
    print(f"{'loop total':12s} {'':4s} " + " ".join(f"{tot[c]:6d}" for c in CLASSES))


if __name__ == "__main__":
    main()
