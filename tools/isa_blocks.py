"""Basic-block listing of one kernel: instruction counts per block, the source
lines each block maps to and its branch targets (static view of the hot loop).
Usage: python tools/isa_blocks.py <mangled-prefix> [asm] [labels for an op histogram]
       python tools/isa_blocks.py <mangled-prefix> asm --walk START --taken L1,L2,... [--where OP]
--walk: the issue cost of ONE path through the listing, e.g. the common path of the substep loop: from block START in
layout order, a branch is taken when its target is in --taken (the loop's back edge included: the walk ends when it
returns to START), every other branch falls through. Instructions are priced per wave at one wave per SIMD from
profiles/r01_issue_rate_microbench.txt: 4.5 cycles for a 4-byte encoding, 4.94 for an 8-byte one (VOP3, DPP, SDWA,
literals), 8.5 for a transcendental, 4.5 + 4 n for s_nop n, 6.5 for a branch not taken, 20.5 for one taken.
--where OP: the source lines of the path's instructions whose mnemonic starts with OP.
       python tools/isa_blocks.py <mangled-prefix> asm --dpp-hazards
--dpp-hazards: every DPP instruction of the kernel whose lane-permuted source register was written by a vector instruction
less than two wait states before it, in layout order (exit status 1 if there is one). The compiler keeps that distance for
its own instructions and cannot see into `asm` blocks: this is the check of the hand-written ones (csrc/octet.hpp)."""
import collections
import re
import sys

prefix = sys.argv[1]
path = sys.argv[2] if len(sys.argv) > 2 else "/tmp/isa4/g.s"
flags = {}
dpp_hazards = "--dpp-hazards" in sys.argv
if dpp_hazards:
    sys.argv.remove("--dpp-hazards")
for name in ("--walk", "--taken", "--where"):
    if name in sys.argv:
        i = sys.argv.index(name)
        flags[name] = sys.argv[i + 1]
        del sys.argv[i:i + 2]
txt = open(path).read().split("\n")
files = {}
for line in txt:
    m = re.match(r'\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', line)
    if m:
        files[int(m.group(1))] = m.group(2).split("/")[-1]
start = next(i for i, l in enumerate(txt) if l.startswith(prefix))
blocks = []  # (label, ops list, lines counter, targets)
cur = dict(label="entry", ops=[], lines=collections.Counter(), targets=[])
loc = ("?", 0)
for i in range(start + 1, len(txt)):
    l = txt[i].strip()
    if l.startswith(".Lfunc_end"):
        break
    m = re.match(r"(\.LBB\d+_\d+):", l)
    if m:
        blocks.append(cur)
        cur = dict(label=m.group(1), ops=[], lines=collections.Counter(), targets=[])
        continue
    m = re.match(r"\.loc\s+(\d+)\s+(\d+)", l)
    if m:
        loc = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
        continue
    if not l or l[0] in ";." or l.endswith(":"):
        continue
    op = l.split()[0]
    cur["ops"].append(op)
    cur.setdefault("text", []).append((l, loc))
    cur["lines"][loc] += 1
    if op.startswith("s_cbranch") or op == "s_branch":
        cur["targets"].append((op, l.split()[-1]))
        blocks.append(cur)
        cur = dict(label=cur["label"].split("+")[0] + "+", ops=[], lines=collections.Counter(), targets=[])
blocks.append(cur)
for b in blocks if "--walk" not in flags and not dpp_hazards else []:
    n = len(b["ops"])
    nv = sum(1 for o in b["ops"] if o.startswith("v_"))
    top = ", ".join(f"{f}:{ln}x{c}" for (f, ln), c in b["lines"].most_common(4))
    tg = " ".join(f"{o[10:]}->{t}" for o, t in b["targets"])
    print(f"{b['label']:12s} n={n:5d} valu={nv:5d}  [{tg}]  {top}")

if len(sys.argv) > 3:
    want = sys.argv[3].split(",")
    hist = collections.Counter()
    for b in blocks:
        if b["label"] in want:
            hist.update(b["ops"])
    print("--- op histogram of", want, "total", sum(hist.values()))
    for op, c in hist.most_common(40):
        print(f"  {op:28s} {c}")


TRANSCENDENTAL = ("v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_", "v_exp_", "v_log_")


def price(text):
    """Issue cycles of one instruction that is not a branch (see the module docstring)."""
    op = text.split()[0]
    if op == "s_nop":
        return 4.5 + 4.0 * int(text.split()[1], 0)
    if op.startswith(TRANSCENDENTAL):
        return 8.5
    if op.startswith(("v_", "s_")):
        wide = op.endswith(("_e64", "_dpp", "_sdwa", "_e64_dpp")) or op.startswith(("v_fma_", "v_mad_", "v_pk_", "v_readlane", "v_writelane", "v_accvgpr"))
        # a 32-bit literal operand makes any encoding 8 bytes long
        literal = any(re.fullmatch(r"(0x[0-9a-f]+|-?\d+\.\d+(e[-+]?\d+)?|-?\d{3,})", t.strip(",")) and not re.fullmatch(r"-?(0\.5|[124]\.0)", t.strip(","))
                      for t in text.split()[1:]) and not op.startswith(("s_waitcnt", "s_nop"))
        return 4.94 if wide or literal else 4.5
    return 4.5


if "--walk" in flags:
    taken = set(flags.get("--taken", "").split(","))
    index = next(i for i, b in enumerate(blocks) if b["label"] == flags["--walk"])
    first, total, visited = index, 0.0, []
    count = collections.Counter()
    where = collections.Counter()
    while True:
        b = blocks[index]
        visited.append(b["label"])
        jump = None
        for text, at in b.get("text", []):
            op = text.split()[0]
            count["instructions"] += 1
            if op.startswith("s_cbranch") or op == "s_branch":
                target = text.split()[-1]
                if op == "s_branch" or target in taken:
                    jump = target
                    count["branches taken"] += 1
                    total += 20.5
                else:
                    count["branches not taken"] += 1
                    total += 6.5
                continue
            total += price(text)
            count["VALU"] += op.startswith("v_")
            count["scalar"] += op.startswith("s_")
            count["s_nop"] += op == "s_nop"
            count["v_mov_b32_dpp"] += op == "v_mov_b32_dpp"
            count["other DPP"] += op.endswith("_dpp") and op != "v_mov_b32_dpp"
            count["SGPR spill moves"] += op.startswith(("v_readlane", "v_writelane"))
            count["scratch"] += op.startswith("scratch_")
            if "--where" in flags and op.startswith(flags["--where"]):
                where[at] += 1
        index = next(i for i, x in enumerate(blocks) if x["label"] == jump) if jump else index + 1
        if index == first or index >= len(blocks) or len(visited) > 2000:
            break
    print(f"path from {flags['--walk']}: {len(visited)} blocks, ends {'at its start (a loop)' if index == first else 'elsewhere'}")
    for name in ("instructions", "VALU", "scalar", "branches taken", "branches not taken", "s_nop", "v_mov_b32_dpp", "other DPP", "SGPR spill moves", "scratch"):
        print(f"  {name:20s} {count[name]}")
    print(f"  {'issue cycles':20s} {total:.0f}")
    for (f, ln), c in sorted(where.items()):
        print(f"  {flags['--where']} at {f}:{ln} x{c}")


def registers(operand):
    """VGPR numbers an operand names: v7, -v7, |v7|, v[4:7]."""
    m = re.fullmatch(r"[-|]*v(\d+)\|?", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


if dpp_hazards:
    found = 0
    recent = []  # (registers written, wait states the instruction is worth) of the instructions before, nearest last; kept
    # across block boundaries: a block's layout predecessor usually falls through into it (otherwise: a finding too many)
    for b in blocks:
        for text, at in b.get("text", []):
            op = text.split()[0]
            operands = [t.strip(",") for t in text.split()[1:]]
            if re.search(r"quad_perm|row_shl|row_shr|row_ror|row_bcast|row_mirror|row_half_mirror|wave_", text) and len(operands) > 1:
                source, states = registers(operands[1]), 0
                for written, worth in reversed(recent):
                    if states >= 2:
                        break
                    if written & source:
                        found += 1
                        print(f"{b['label']}: {text}   <- written {states} wait state(s) before ({at[0]}:{at[1]})")
                        break
                    states += worth
            written = registers(operands[0]) if op.startswith("v_") and operands and not op.startswith(("v_cmp", "v_readlane", "v_readfirstlane")) else set()
            recent.append((written, 1 + int(operands[0], 0) if op == "s_nop" else 1))
    print(f"{found} DPP read(s) too close to the write of their source")
    sys.exit(1 if found else 0)
