#!/usr/bin/env python3
"""Second part of a code-object comparison (tools/cmp_code_objects.sh prints the first): every kernel or device function that
BOTH libraries have and whose code bytes differ, compared instruction by instruction (llvm-objdump -d --no-show-raw-insn).

    python tools/cmp_kernel_insns.py <libA.so> <libB.so>

Per function: the number of instructions, how many differ, whether the counts are equal, the opcodes of the differing lines
and the first two differing lines.  Exit status 0 when every difference is a literal of an s_add_u32 / s_addc_u32 (a
pc-relative address computation: the distance to .rodata or to a non-inlined function moved), 1 otherwise."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_objects(lib, d):
    fat = os.path.join(d, "fat.bin")
    subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(d, "stripped.so")], check=True)
    data = open(fat, "rb").read()
    idx = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]
    out = []
    for n, i in enumerate(idx):
        b = os.path.join(d, "b%02d.bin" % n)
        open(b, "wb").write(data[i:(idx[n + 1] if n + 1 < len(idx) else len(data))])
        co = os.path.join(d, "co%02d.co" % len(out))
        r = subprocess.run([LLVM + "/clang-offload-bundler", "--type=o", "--targets=" + TARGET, "--input=" + b, "--output=" + co, "--unbundle"],
                           stderr=subprocess.DEVNULL)
        if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co):
            out.append(co)
    return out


def functions(co):
    """name -> list of instructions (addresses and raw bytes stripped, branch targets kept as the disassembler prints them)"""
    txt = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co], stdout=subprocess.PIPE, text=True, check=True).stdout
    fns, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = fns.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = re.sub(r"\s*//.*$", "", line.strip())
        if ins:
            cur.append(ins)
    return fns


def main():
    la, lb = sys.argv[1:3]
    other = False
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ca, cb = code_objects(la, ta), code_objects(lb, tb)
        for k, (a, b) in enumerate(zip(ca, cb)):
            fa, fb = functions(a), functions(b)
            for name in sorted(set(fa) & set(fb)):
                x, y = fa[name], fb[name]
                if x == y:
                    continue
                diff = [(p, q) for p, q in zip(x, y) if p != q]
                ops = sorted({p.split()[0] for p, q in diff} | {q.split()[0] for p, q in diff})
                short = name.replace("_ZN2rt7k_stageIN3bbs", "")[:64]
                print("co%02d %-66s lines %d, differing %d, len equal %s, opcodes of differing lines: %s"
                      % (k, short, len(x), len(diff), len(x) == len(y), ops))
                for p, q in diff[:2]:
                    print("      A: %s | B: %s" % (p, q))
                if len(x) != len(y) or not set(ops) <= {"s_add_u32", "s_addc_u32"}:
                    other = True
    print("RESULT:", "differences OTHER than pc-relative literals" if other else "only literals of pc-relative address computations differ")
    sys.exit(1 if other else 0)


if __name__ == "__main__":
    main()
