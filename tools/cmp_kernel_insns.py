#!/usr/bin/env python3
"""Second part of a code-object comparison (tools/cmp_code_objects.sh prints the first): every kernel or device function that
BOTH libraries have and whose code bytes differ, compared instruction by instruction (llvm-objdump -d --no-show-raw-insn).

    python tools/cmp_kernel_insns.py <libA.so> <libB.so> [--renames FILE]

Per function: the number of instructions, how many differ, whether the counts are equal, the opcodes of the differing lines
and the first two differing lines.  Exit status 0 when every difference is a literal of an s_add_u32 / s_addc_u32 (a
pc-relative address computation: the distance to .rodata or to a non-inlined function moved), 1 otherwise.

--renames FILE: kernels that changed their name between A and B, one pair per line, `old stage -> new stage`, each the stage
type as the demangler prints it inside rt::k_stage<...> without the leading bbs:: (`#` starts a comment).  Every pair is
compared predecessor with successor: VGPRs (total), AGPRs, scratch bytes and the wavefronts per SIMD that follow from the
registers must be equal, and the instruction streams may differ only in scalar loads (the offsets and widths of kernel-argument
loads), in the s_waitcnt lines that wait for them, and in pc-relative literals.  A pair that is missing on either side, or
that differs in anything else, makes the exit status 1; its differing instructions are printed."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
PCREL = {"s_add_u32", "s_addc_u32"}


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


def functions(co, demangle=False):
    """name -> list of instructions (addresses and raw bytes stripped, branch targets kept as the disassembler prints them)"""
    txt = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn"] + (["--demangle"] if demangle else []) + [co],
                         stdout=subprocess.PIPE, text=True, check=True).stdout
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


def resources(co):
    """mangled kernel name -> (vgpr total, agpr, scratch bytes) from the metadata notes"""
    out, cur = {}, None
    txt = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], stdout=subprocess.PIPE, text=True, check=True).stdout
    for line in txt.splitlines():
        m = re.match(r"\s*(- )?\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        key, val = m.group(2), m.group(3)
        if key == "agpr_count":            # first field of a kernel's entry (the fields are sorted by name)
            cur = {}
        if cur is None:
            continue
        cur[key] = val
        if key == "name":
            out[val] = cur                 # (the fields behind .name are still to come)
    return {k: (int(v["vgpr_count"]), int(v["agpr_count"]), int(v["private_segment_fixed_size"])) for k, v in out.items()}


def waves_per_simd(vgpr_total):
    """gfx950: 512 registers per lane and SIMD (VGPRs and AGPRs together), allocated in blocks of 8, at most 8 wavefronts"""
    return min(8, 512 // max(8, (vgpr_total + 7) // 8 * 8))


def stage_of(demangled):
    m = re.match(r"^void rt::k_stage<bbs::(.+?), bbs::\w+Args<", demangled)
    return m.group(1) if m else None


def compare_renamed(pairs, ca, cb):
    bad = False
    where = [{}, {}]                        # stage -> (code object, mangled name, instructions)
    for side, cos in enumerate((ca, cb)):
        for co in cos:
            plain, dem = functions(co), functions(co, demangle=True)
            assert len(plain) == len(dem), "two symbols of %s demangle to one name" % co
            for (mangled, ins), d in zip(plain.items(), dem):
                st = stage_of(d)
                if st:
                    where[side][st] = (co, mangled, ins)
    res = {}
    print("\nrenamed kernels, predecessor (A) against successor (B):")
    for old, new in pairs:
        if old not in where[0] or new not in where[1]:
            print("  %s -> %s: MISSING in %s" % (old, new, "A" if old not in where[0] else "B"))
            bad = True
            continue
        (coa, ma, x), (cob, mb, y) = where[0][old], where[1][new]
        for co in (coa, cob):
            if co not in res:
                res[co] = resources(co)
        ra, rb = res[coa][ma], res[cob][mb]
        line = "  %s -> %s\n      vgpr (total) %d / %d, agpr %d / %d, scratch %d / %d B, wavefronts per SIMD %d / %d" % (
            old, new, ra[0], rb[0], ra[1], rb[1], ra[2], rb[2], waves_per_simd(ra[0]), waves_per_simd(rb[0]))
        ok = ra == rb
        diff = []
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, x, y, autojunk=False).get_opcodes():
            if tag != "equal":
                diff.append((x[i1:i2], y[j1:j2]))
        ops = sorted({l.split()[0] for p, q in diff for l in p + q})
        allowed = all(o.startswith("s_load_dword") or o == "s_waitcnt" or o in PCREL for o in ops)
        # (a pc-relative literal may change, never appear or vanish)
        allowed = allowed and all(len(p) == len(q) for p, q in diff if any(l.split()[0] in PCREL for l in p + q))
        print(line + "\n      instructions %d / %d, differing blocks %d, opcodes in them: %s -> %s" % (
            len(x), len(y), len(diff), ops, "ok" if ok and allowed else "DIFFERS"))
        if not (ok and allowed):
            bad = True
            for p, q in diff:
                print("      A: %s\n      B: %s" % (" ; ".join(p) or "-", " ; ".join(q) or "-"))
    return bad


def main():
    args = sys.argv[1:]
    pairs = None
    if "--renames" in args:
        k = args.index("--renames")
        pairs = []
        for line in open(args[k + 1]):
            line = line.split("#")[0].strip()
            if line:
                old, new = line.split("->")
                pairs.append((old.strip(), new.strip()))
        del args[k:k + 2]
    la, lb = args[:2]
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
                if len(x) != len(y) or not set(ops) <= PCREL:
                    other = True
        print("RESULT:", "differences OTHER than pc-relative literals" if other else "only literals of pc-relative address computations differ")
        renamed_bad = compare_renamed(pairs, ca, cb) if pairs is not None else False
    if pairs is not None:
        print("RESULT (renamed):", "a pair differs in MORE than argument loads" if renamed_bad else
              "every pair: equal registers, scratch and occupancy; only argument loads, their waits and pc-relative literals differ")
    sys.exit(1 if other or renamed_bad else 0)


if __name__ == "__main__":
    main()
