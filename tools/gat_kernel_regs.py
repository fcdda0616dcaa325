#!/usr/bin/env python3
"""Register table of the second-generation GAT kernels (csrc/gat_*.hip: every gat2_kernel instantiation): VGPRs, SGPRs, scratch, LDS
and the wavefronts per SIMD the VGPR count allows, read from the assembly hipcc emits with the library's own flags (no GPU needed).

    python tools/gat_kernel_regs.py                 the whole table, one line per instantiation (tab separated, demangled key)
    python tools/gat_kernel_regs.py --save F        also write it to F
    python tools/gat_kernel_regs.py --against F     compare with a table saved from another commit: instantiations present in both
                                                    must agree in VGPRs, scratch and LDS (a trailing DROP = false parameter is ignored)"""
import concurrent.futures as cf
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAME = re.compile(r"gat2_kernelI(\w)(\w)Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])E(?:Lb([01])E)?EEv")


def key_of(symbol):
    m = NAME.search(symbol)
    if not m:
        return None
    xt, _, epv, lpr, nh, u, kind, inrow, trow, drop = m.groups()
    return "%s epv%s lpr%s nh%s u%s kind%s%s%s%s" % ("bf16" if xt == "t" else "f32", epv, lpr, nh, u, kind, " inrow" if inrow == "1" else "",
                                                    " trow" if trow == "1" else "", " drop" if drop == "1" else "")


def table():
    from dgll_amd.build import FLAGS

    srcs = sorted(glob.glob(os.path.join(ROOT, "dgll_amd", "csrc", "gat_*.hip")))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        def asm(src):
            dst = os.path.join(tmp, os.path.basename(src) + ".s")
            subprocess.run(["hipcc"] + [f for f in FLAGS if f not in ("-fPIC", "-pthread")] + ["-I", os.path.join(ROOT, "include"), "-S",
                           "--cuda-device-only", src, "-o", dst], check=True, stderr=subprocess.DEVNULL)
            return open(dst).read()

        with cf.ThreadPoolExecutor(max_workers=4) as ex:
            for txt in ex.map(asm, srcs):
                for blk in txt.split("  - .agpr_count")[1:]:
                    get = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1))      # noqa: E731
                    key = key_of(re.search(r"\.name:\s+(\S+)", blk).group(1))
                    if key:
                        v = get("vgpr_count")
                        out[key] = (v, get("sgpr_count"), get("private_segment_fixed_size"), get("group_segment_fixed_size"),
                                    min(8, 512 // ((v + 7) // 8 * 8)))
    return out


def main():
    tab = table()
    lines = ["%s\t%d\t%d\t%d\t%d\t%d" % ((k,) + v) for k, v in sorted(tab.items())]
    print("# instantiation\tvgpr\tsgpr\tscratch\tlds\twaves/simd")
    print("\n".join(lines))
    if "--save" in sys.argv:
        with open(sys.argv[sys.argv.index("--save") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")
    if "--against" in sys.argv:
        old = dict((l.split("\t")[0], tuple(int(x) for x in l.split("\t")[1:])) for l in open(sys.argv[sys.argv.index("--against") + 1]) if l.strip())
        both = [k for k in old if k in tab]
        changed = [k for k in both if (old[k][0], old[k][2], old[k][3]) != (tab[k][0], tab[k][2], tab[k][3])]
        for k in changed:
            print("CHANGED", k, old[k], tab[k])
        print("# %d instantiations in both tables, %d changed in VGPRs / scratch / LDS, %d new, %d gone"
              % (len(both), len(changed), len(set(tab) - set(old)), len(set(old) - set(tab))))
        return 1 if changed else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
