"""Dev tool (CPU): is the device code of two builds the same?  usage: tools/compare_isa.py <build dir A> <build dir B>

Reads every *-hip-amdgcn-amd-amdhsa-gfx950.s of both directories (make keeps them: -save-temps=obj) and compares, per kernel and device
function, the instruction text and the kernel descriptor (.amdhsa_kernel block) after dropping comments and .loc / .file lines and
the per-function numbers of local labels (.LBB<n>_, .Ltmp<n>, .Lfunc_begin<n>, .Lfunc_end<n>).  Then the per-kernel blocks of
resource_usage.txt (-Rpass-analysis=kernel-resource-usage) as a sorted set.  Symbols of slam_comm are compared like the others.
Exit status 0: same symbols, no kernel twice, every body and every resource block equal.
"""
import glob
import os
import re
import sys

LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+")


def clean(line):
    line = line.split(";", 1)[0].rstrip()
    s = line.strip()
    if not s or s.startswith((".loc", ".file")):
        return None
    return LABEL.sub(lambda m: "." + m.group(1), s)


def functions(build_dir):
    """name -> cleaned lines of the function (kernels: with their descriptor); kernels: names with a descriptor; dup: names that
    occur again with ANOTHER body (a device function that is not inlined is emitted, identically, by every unit that calls it)"""
    out, kernels, dup = {}, [], []
    for path in sorted(glob.glob(os.path.join(build_dir, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        name, body = None, []
        for raw in open(path):
            m = re.match(r"\s*\.type\s+(\S+),@function", raw)
            if m:
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            if re.match(r"\s*\.amdhsa_kernel\s", raw):
                kernels.append(name)
            if re.match(r"\s*\.Lfunc_end\d+:", raw):
                if name in out and (out[name] != body or name in kernels[:-1]):
                    dup.append(name)
                out[name] = body
                name = None
                continue
            c = clean(raw)
            if c is not None:
                body.append(c)
    return out, kernels, dup


def resource_blocks(build_dir):
    blocks, cur = [], None
    for raw in open(os.path.join(build_dir, "resource_usage.txt")):
        m = re.match(r"remark: \S+:\d+:\d+:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]", raw)
        if not m:
            continue
        text = m.group(1)
        if text.startswith("Function Name:"):
            cur = [text]
            blocks.append(cur)
        elif cur is not None:
            cur.append(text)
    return sorted("\n".join(b) for b in blocks)


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    (a, a_k, a_dup), (b, b_k, b_dup) = functions(a_dir), functions(b_dir)
    bad = 0
    for tag, dup in (("A", a_dup), ("B", b_dup)):
        for n in dup:
            print(f"{tag}: {n} is a kernel emitted twice, or a device function emitted with two bodies")
            bad += 1
    for n in sorted(set(a) - set(b)):
        print(f"only in A: {n}")
        bad += 1
    for n in sorted(set(b) - set(a)):
        print(f"only in B: {n}")
        bad += 1
    for n in sorted(set(a) & set(b)):
        if a[n] != b[n]:
            first = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
            print(f"differs: {n} ({len(a[n])} / {len(b[n])} lines, first difference at line {first})")
            bad += 1
    print(f"A: {len(a_k)} kernels, {len(a) - len(set(a_k))} device functions; B: {len(b_k)} kernels, {len(b) - len(set(b_k))} device functions")
    ra, rb = resource_blocks(a_dir), resource_blocks(b_dir)
    if ra != rb:
        print(f"resource_usage.txt differs: {len(ra)} / {len(rb)} blocks, {len(set(ra) ^ set(rb))} unmatched")
        bad += 1
    else:
        print(f"resource_usage.txt: {len(ra)} blocks, equal as a sorted set")
    print("SAME" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
