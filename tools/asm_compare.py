#!/usr/bin/env python3
"""Compare two device assembly files (hipcc -S --offload-device-only) function by function.

  tools/asm_compare.py parent.s new.s [substring of the functions to report resources for]

Prints the functions whose instruction text differs, the functions only one side has, and for the functions that match
the substring their resource lines (.vgpr_count, .sgpr_count, LDS, scratch, spills) and how many v_fma / v_mad / v_div
instructions they hold. Labels the compiler numbers per file (.LBB12_3) are compared by position, not by name."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            name, body = m.group(1), []
            out[name] = body
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        t = line.split(";")[0].strip()
        if t and not t.startswith("."):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
        elif t.startswith(".LBB"):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def resources(path):
    """{kernel: {key: value}} from the .amdgpu_metadata block"""
    out, cur = {}, None
    keys = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")
    blocks = open(path).read().split("  - .agpr_count:")
    for b in blocks[1:]:
        name = re.search(r"\.name:\s+(\S+)", b)
        if name:
            out[name.group(1)] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", b).group(1)) for k in keys if re.search(re.escape(k) + r":\s+(\d+)", b)}
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    want = sys.argv[3] if len(sys.argv) > 3 else None
    differ = sorted(n for n in a if n in b and a[n] != b[n])
    print("functions in both:", len([n for n in a if n in b]), "differing:", len(differ))
    for n in differ:
        print("  DIFFERS", n, len(a[n]), "->", len(b[n]), "lines")
    for n in sorted(set(a) - set(b)):
        print("  ONLY IN", sys.argv[1], n)
    for n in sorted(set(b) - set(a)):
        print("  ONLY IN", sys.argv[2], n)
    if want:
        res = resources(sys.argv[2])
        for n in sorted(b):
            if want in n:
                ops = {k: sum(1 for t in b[n] if t.startswith(k)) for k in ("v_fma", "v_mad", "v_div", "v_mul_f32", "v_cvt_i32_f32", "v_rndne", "scratch_", "buffer_")}
                print(n, len(b[n]), "lines", res.get(n), ops)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
