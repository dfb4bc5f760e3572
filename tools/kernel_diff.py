"""Per-kernel comparison of two device-side assembly listings of the library's HIP sources.

  hipcc <the flags of dl4ss_amd/build.py> -I dl4ss_amd/csrc --cuda-device-only -S a.hip -o a.s
  python tools/kernel_diff.py OLD NEW        (each a .s file or a directory of .s files)

For every kernel: the instruction stream, the kernel descriptor (.amdhsa_* block: VGPR / SGPR / AGPR
counts, scratch, static LDS, kernarg size), the compiler's "Kernel info" block and the code-object
metadata entry, one verdict per kernel.  Kernels are matched by mangled name with the enclosing
namespace dropped (a kernel may move between an anonymous and a named namespace), and basic-block /
function label numbers are normalised (they count a function's position in its file).  Exit status 1
when any kernel differs or is missing on one side."""
import difflib
import glob
import os
import re
import sys


def listing(path):
    files = sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]
    out = {}
    for f in files:
        out.update(kernels(open(f).read().split("\n")))
    return out


def kernels(lines):
    names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    # "<len><name>" of every namespace that encloses a kernel: _ZN<len><ns><len><kernel>...
    spaces = {m.group(1) + m.group(2)[:int(m.group(1))] for n in names
              if (m := re.match(r"_ZN(\d+)(.*)", n)) and m.group(2)[int(m.group(1)):][:1].isdigit()}
    ns = re.compile("|".join(sorted(map(re.escape, spaces), key=len, reverse=True))) if spaces else None

    def norm(ln):
        if ns:  # "L": the internal-linkage mark a const variable gets in a named namespace only
            ln = re.sub(r"(_ZN\?)L(?=\d)", r"\1", ns.sub("?", ln))
        ln = re.sub(r"BB\d+_(\d+)", r"BB#_\1", ln)  # .LBB<function>_<block>, and "Header=BB.." comments
        ln = re.sub(r"\.L(func_begin|func_end|JTI|tmp)\d+", r".L\1#", ln)
        return re.sub(r"\s+", " ", ln).rstrip()  # a comment's column moves with the label's length

    out = {norm(n): {"code": [], "descriptor": [], "info": [], "metadata": []} for n in names}
    cur, part = None, None
    for ln in lines:
        if m := re.match(r"\s*\.type\s+(\S+),@function", ln):
            cur, part = out.get(norm(m.group(1))), "code"
        elif re.match(r"\s*\.amdhsa_kernel\s", ln):
            part = "descriptor"
        elif re.match(r"\s*\.end_amdhsa_kernel", ln):
            part = "code"
        elif ln.startswith("; Kernel info:"):
            part = "info"
        elif part == "info" and not ln.startswith(";"):
            cur, part = None, None
        elif ln.startswith("amdhsa.kernels:"):
            cur, part = None, "metadata"
        elif part == "metadata" and ln.startswith("  - "):
            cur = {"metadata": []}
        elif part == "metadata" and ln[:1] not in (" ", ""):
            cur, part = None, None
        if cur is not None and part is not None and not re.match(r"\s*\.(section|text|p2align)\b", ln):
            cur[part].append(norm(ln))
            if part == "metadata" and (m := re.match(r"\s+\.name:\s+(\S+)", norm(ln))) and m.group(1) in out:
                out[m.group(1)]["metadata"] = cur["metadata"]
    return out


def main(a_path, b_path):
    a, b = listing(a_path), listing(b_path)
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k}: only in {'NEW' if k not in a else 'OLD'}")
            bad += 1
            continue
        notes = []
        for part in ("code", "descriptor", "info", "metadata"):
            if a[k][part] != b[k][part]:
                d = [x for x in difflib.unified_diff(a[k][part], b[k][part], lineterm="", n=0)
                     if x[:1] in "+-" and x[:3] not in ("+++", "---")]
                notes.append(f"{part}: {len(d)} lines differ of {len(a[k][part])} / {len(b[k][part])}")
                if part != "code" or "-v" in sys.argv:
                    notes += ["    " + x for x in d[:40]]
        print(f"{k}: {'identical' if not notes else 'DIFFERS'}")
        for n in notes:
            print("  " + n)
        bad += bool(notes)
    print(f"{len(set(a) | set(b))} kernels, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
