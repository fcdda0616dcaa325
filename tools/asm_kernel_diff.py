#!/usr/bin/env python
"""Compare the kernels of two device assembly files (hipcc ... --cuda-device-only -S) of one source before / after a refactor.

    python tools/asm_kernel_diff.py OLD.s NEW.s

Reads the two files, nothing else.  Reports kernels only one file has, per kernel the .amdhsa metadata that must not move
(.vgpr_count, .agpr_count, .sgpr_count, .private_segment_fixed_size, .group_segment_fixed_size) and whether the instruction
text is the same once label numbers, comments and debug directives are stripped.  Exit status 1 if a kernel set or a
metadata value differs; kernels whose text alone differs are listed (they are the ones to time) and do not fail the run.
"""
import re
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def metadata(text):
    """{kernel name: {key: value}} from the amdhsa.kernels YAML at the end of the file."""
    out = {}
    for block in re.split(r"\n  - ", text[text.find("amdhsa.kernels:"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in META
                                  if re.search(re.escape(k) + r":\s+(\d+)", block)}
    return out


def bodies(text):
    """{function name: normalised instruction lines}."""
    out = {}
    for m in re.finditer(r"^(\w+):\s+; @\1\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
        lines = []
        for line in m.group(2).split("\n"):
            line = line.split(";")[0].rstrip()
            if not line or re.match(r"\s*\.(loc|file|cfi_|p2align)", line):
                continue
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        out[m.group(1)] = lines
    return out


def main(old_path, new_path):
    old, new = open(old_path).read(), open(new_path).read()
    mo, mn = metadata(old), metadata(new)
    bo, bn = bodies(old), bodies(new)
    bad = False
    print("kernels: %d old, %d new" % (len(mo), len(mn)))
    for name in sorted(set(mo) - set(mn)):
        bad = True
        print("only in old: " + name)
    for name in sorted(set(mn) - set(mo)):
        bad = True
        print("only in new: " + name)
    text_differs = []
    for name in sorted(set(mo) & set(mn)):
        if mo[name] != mn[name]:
            bad = True
            print("metadata differs: %s\n  old %s\n  new %s" % (name, mo[name], mn[name]))
        if bo.get(name) != bn.get(name):
            text_differs.append((name, len(bo.get(name, ())), len(bn.get(name, ()))))
    same = len(set(mo) & set(mn)) - len(text_differs)
    print("metadata identical: %s" % ("no" if bad else "yes"))
    print("instruction text identical: %d kernels; differs: %d" % (same, len(text_differs)))
    for name, a, b in text_differs:
        print("  text differs (%d -> %d lines): %s" % (a, b, name))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
