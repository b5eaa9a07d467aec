#!/usr/bin/env python3
"""Compares the device assembly of two builds of the same translation unit kernel by kernel: the instruction streams (labels and mangled names
aside) and the registers, LDS and scratch of the code-object metadata.

usage: compare_kernel_asm.py OLD.s NEW.s [--drop-leading-false N]

OLD.s / NEW.s: what `hipcc -S --cuda-device-only` (tools/kernel_resources.sh leaves such files behind) writes for the unit before and after a
change.  A kernel of NEW.s whose first N template arguments are `false` is matched with the kernel of OLD.s that lacks them: the way a
compile-time parameter added in front of a kernel's list is shown to leave the instantiations that existed before as they were.  Kernels of
NEW.s without a partner are listed as new.  Exit status 1 if a matched pair differs."""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if f".amdhsa_kernel {name}" not in text:
            continue
        lines = []
        for line in body.split("\n"):
            line = line.split(";")[0].rstrip()
            if not line.strip() or line.lstrip().startswith("."):   # comments, directives and local labels
                continue
            line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
            line = re.sub(r"_Z\w+", "SYM", line)
            lines.append(line.strip())
        meta = {}
        mm = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), text, re.S)
        for key in ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size"):
            v = re.search(r"\.amdhsa_%s\s+(\S+)" % key, mm.group(1))
            meta[key] = v.group(1) if v else None
        out[name] = (lines, meta)
    names = list(out)
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"\(.*$", "", p): out[n] for n, p in zip(names, plain)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    drop = int(sys.argv[sys.argv.index("--drop-leading-false") + 1]) if "--drop-leading-false" in sys.argv else 0
    args = args[:2]
    old, new = kernels(args[0]), kernels(args[1])
    bad = 0
    seen = set()
    for name in sorted(new):
        key = name
        for _ in range(drop):
            key = re.sub(r"<false, ", "<", key, count=1) if "<false, " in key else None
            if key is None:
                break
        if key is None and name in old:   # a kernel the parameter was not added to
            key = name
        if key is None or key not in old:
            print(f"new        {name}  vgpr {new[name][1]['next_free_vgpr']} lds {new[name][1]['group_segment_fixed_size']}")
            continue
        seen.add(key)
        same_isa, same_meta = old[key][0] == new[name][0], old[key][1] == new[name][1]
        bad += not (same_isa and same_meta)
        print(f"{'identical ' if same_isa and same_meta else 'DIFFERENT '} {name}  ({len(new[name][0])} instructions; registers {'same' if same_meta else 'differ'})")
    for key in sorted(set(old) - seen):
        print(f"gone       {key}")
        bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
