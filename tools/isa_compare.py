"""Compare the device assembly of two builds of the library, kernel by kernel.

Usage: python tools/isa_compare.py <dir of the old build's .s files> <dir of the new build's> [unit that must not differ ...]

Both directories hold one `<unit>.s` per translation unit, from hipcc with the library's flags (upkie_amd/lib.py: HIPCC_FLAGS
without --offload-compress) plus `-S --cuda-device-only`; tools/isa_stats.sh shows the command line of the step-kernel groups
(`-DUPKIE_INSTANCE_GROUP=g`, saved here as g<g>.s). A kernel's text runs from its label to its .Lfunc_end; the number of the
function inside its unit is taken out of the local labels, and .ident, .file and __hip_cuid_* lines never lie inside a kernel.
For every kernel whose text differs the table gives instruction counts and, from the .amdhsa_* lines of its descriptor, the
registers (next_free_vgpr counts AGPRs in), scratch and LDS of both builds. Exit status 1 when a kernel of a unit named on the
command line differs, when a kernel exists on one side only, or when a differing kernel uses more registers, scratch or LDS.
"""
import os
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    """{kernel name: (text lines, {resource: value})} of one .s file."""
    lines = open(path).read().split("\n")
    descriptors, name = {}, None
    for line in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name = m.group(1)
            descriptors[name] = {}
        elif name is not None:
            m = re.match(r"\s*\.amdhsa_(\w+)\s+(\d+)", line)
            if m and m.group(1) in RESOURCES:
                descriptors[name][m.group(1)] = int(m.group(2))
            if ".end_amdhsa_kernel" in line:
                name = None
    found, name, text = {}, None, []
    for line in lines:
        if name is None:
            m = re.match(r"(\w+):", line)
            if m and m.group(1) in descriptors:
                name, text = m.group(1), []
        elif line.startswith(".Lfunc_end"):
            found[name] = (text, descriptors[name])
            name = None
        else:
            text.append(re.sub(r"\.LBB\d+_", ".LBB_", line.rstrip()))
    return found


def instructions(text):
    return sum(1 for l in (t.strip() for t in text) if l and l[0] not in ";." and not l.endswith(":"))


def main():
    old_dir, new_dir, frozen = sys.argv[1], sys.argv[2], set(sys.argv[3:])
    bad = False
    for unit in sorted(f for f in os.listdir(old_dir) if f.endswith(".s")):
        old, new = kernels(os.path.join(old_dir, unit)), kernels(os.path.join(new_dir, unit))
        differ = [k for k in old if k in new and old[k][0] != new[k][0]]
        one_sided = sorted(set(old) ^ set(new))
        print(f"{unit}: {len(old)} kernels, {len(old) - len(differ) - len(set(old) - set(new))} identical, {len(differ)} differ" +
              (f", on one side only: {one_sided}" if one_sided else ""))
        bad = bad or bool(one_sided) or (bool(differ) and unit[:-2] in frozen)
        for k in differ:
            (to, ro), (tn, rn) = old[k], new[k]
            grew = [r for r in RESOURCES if rn.get(r, 0) > ro.get(r, 0)]
            bad = bad or bool(grew)
            print(f"  {k}\n    instructions {instructions(to)} -> {instructions(tn)}; " +
                  "; ".join(f"{r} {ro.get(r)} -> {rn.get(r)}" for r in RESOURCES) + (f"  GREW: {grew}" if grew else ""))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
