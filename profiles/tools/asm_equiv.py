#!/usr/bin/env python3
"""Compare two AMDGPU assembly files (hipcc -S --cuda-device-only) function by function.

    asm_equiv.py PARENT.s TREE.s [--all] [--demangle]

For a refactor that must not change the device code.  Every function of either file (kernels and called device functions) gets
one of three results:

  identical   the bodies are the same text, label numbers aside, and so are the kernel descriptors
  tier-2      the bodies differ, but the multiset of floating-point VALU opcodes is the same (encoding suffixes _e32 / _e64 / _dpp /
              _sdwa stripped, v_fmac_* counted as v_fma_*: no contraction or expansion decision changed) and scratch size, LDS size and
              occupancy are equal.  VGPR / SGPR counts are printed, not gated.
  different   anything else, a function present in one file only included; the reason is printed

Prints a Markdown table of the functions that are not identical (--all: of every function) and a summary line; exits 1 if any
function is different.  --demangle pipes the names through llvm-cxxfilt or c++filt when one is on PATH."""
import argparse
import collections
import re
import shutil
import subprocess
import sys

_TYPE = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
_END = re.compile(r"^\.Lfunc_end\d+:")
_LABEL = re.compile(r"\.L(BB|JTI)\d+_")            # .LBB<function number>_<block>: the function number is dropped
_FP = re.compile(r"^v_\w+_(f16|f32|f64|bf16)\b")
_SUFFIX = re.compile(r"(_e32|_e64|_dpp|_sdwa)+$")
_INFO = {"vgpr": r"; NumVgprs: (\d+)", "agpr": r"; NumAgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)", "scratch": r"; ScratchSize: (\d+)",
         "lds": r"; LDSByteSize: (\d+)", "occupancy": r"; Occupancy: (\d+)"}
GATED = ("scratch", "lds", "occupancy")


def functions(path):
    """{name: {"body": [instruction and label lines], "desc": [descriptor lines], vgpr, sgpr, scratch, lds, occupancy}} in file order"""
    out = collections.OrderedDict()
    lines = open(path, errors="replace").read().splitlines()
    k = 0
    while k < len(lines):
        m = _TYPE.match(lines[k])
        k += 1
        if not m:
            continue
        name, body, desc, in_desc = m.group(1), [], [], False
        while k < len(lines) and lines[k].split(";")[0].strip() != name + ":":
            k += 1
        k += 1
        while k < len(lines) and not _END.match(lines[k]):
            s = lines[k].strip()
            k += 1
            if s.startswith(".amdhsa_kernel"):
                in_desc = True
            elif s.startswith(".end_amdhsa_kernel"):
                in_desc = False
            elif in_desc:
                desc.append(s)
            elif s and not s.startswith((";", ".section", ".p2align", ".text")):
                body.append(_LABEL.sub(r".L\1_", s.split(";")[0].rstrip()))
        f = {"body": body, "desc": desc}
        # the resource remarks follow the function ("; Kernel info:" / "; Function info:"), before the next .type
        j = k
        while j < len(lines) and not _TYPE.match(lines[j]):
            for key, rx in _INFO.items():
                mm = re.match(rx, lines[j])
                if mm and key not in f:
                    f[key] = int(mm.group(1))
            j += 1
        out[name] = f
    return out


def fp_opcodes(body):
    c = collections.Counter()
    for s in body:
        op = s.split()[0] if s else ""
        if _FP.match(_SUFFIX.sub("", op)):
            c[_SUFFIX.sub("", op).replace("v_fmac_", "v_fma_").replace("v_pk_fmac_", "v_pk_fma_")] += 1
    return c


def compare(a, b):
    """(result, reason)"""
    if a is None or b is None:
        return "different", "only in the %s file" % ("second" if a is None else "first")
    if a["body"] == b["body"] and a["desc"] == b["desc"]:
        return "identical", ""
    why = []
    fa, fb = fp_opcodes(a["body"]), fp_opcodes(b["body"])
    if fa != fb:
        d = {op: fb[op] - fa[op] for op in set(fa) | set(fb) if fa[op] != fb[op]}
        why.append("fp opcodes " + ", ".join("%s %+d" % kv for kv in sorted(d.items())))
    for key in GATED:
        if a.get(key) != b.get(key):
            why.append("%s %s -> %s" % (key, a.get(key), b.get(key)))
    return ("different", "; ".join(why)) if why else ("tier-2", "")


def demangled(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("--all", action="store_true", help="list the identical functions too")
    ap.add_argument("--demangle", action="store_true")
    args = ap.parse_args(argv)
    A, B = functions(args.first), functions(args.second)
    names = list(A) + [n for n in B if n not in A]
    show = demangled(names) if args.demangle else {n: n for n in names}
    count = collections.Counter()
    print("| function | result | VGPR | SGPR | scratch | LDS | occupancy | fp VALU ops | reason |")
    print("|---|---|---|---|---|---|---|---|---|")
    for n in names:
        a, b = A.get(n), B.get(n)
        res, why = compare(a, b)
        count[res] += 1
        if res == "identical" and not args.all:
            continue

        def pair(key):
            x, y = (a or {}).get(key, "-"), (b or {}).get(key, "-")
            return str(x) if x == y else "%s -> %s" % (x, y)
        nfp = sum(fp_opcodes((b or a)["body"]).values())
        print("| `%s` | %s | %s | %s | %s | %s | %s | %d | %s |" % (show[n], res, pair("vgpr"), pair("sgpr"), pair("scratch"), pair("lds"),
                                                                  pair("occupancy"), nfp, why))
    print("\n%d functions: %d identical, %d tier-2, %d different" % (len(names), count["identical"], count["tier-2"], count["different"]))
    return 1 if count["different"] else 0


if __name__ == "__main__":
    sys.exit(main())
