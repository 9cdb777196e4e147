#!/bin/bash
# compare the gfx950 code objects of two builds of the library: tools/cmp_code_objects.sh <libA.so> <libB.so>
#   per code object: .text, .rodata, the symbol table (without the __hip_cuid_<hash> marker) and the llvm-objdump -d output
#   per kernel     : code size, VGPR, AGPR, SGPR, private-segment (scratch) and LDS bytes from the metadata notes of both
#                    libraries, every difference flagged (a kernel of one library only: its own figures); the set of kernel
#                    symbols; the largest scratch of each library
# exit status 0: every code object identical; 1: something differs (resources or bytes); 2: usage / tool failure
set -e -o pipefail
[ $# -eq 2 ] || { echo "usage: $0 <libA.so> <libB.so>" >&2; exit 2; }
LLVM=${LLVM_BIN:-/opt/rocm/lib/llvm/bin}
libs=("$(readlink -f "$1")" "$(readlink -f "$2")")
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
for s in 0 1; do
    d=$tmp/$s; mkdir -p $d
    # unbundle as tools/kernel_meta.sh does: the fat binary is a sequence of offload bundles, one per translation unit
    $LLVM/llvm-objcopy --dump-section .hip_fatbin=$d/fat.bin "${libs[$s]}" $d/stripped.so
    python3 - $d <<'PY'
import re, sys
d = sys.argv[1]
data = open(d + '/fat.bin', 'rb').read()
idx = [m.start() for m in re.finditer(b'__CLANG_OFFLOAD_BUNDLE__', data)]
for n, i in enumerate(idx):
    open('%s/b%02d.bin' % (d, n), 'wb').write(data[i:(idx[n + 1] if n + 1 < len(idx) else len(data))])
PY
    k=0
    for b in $d/b*.bin; do
        co=$d/co$(printf %02d $k)
        $LLVM/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$b --output=$co.co --unbundle 2>/dev/null || continue
        [ -s $co.co ] || continue
        $LLVM/llvm-objcopy --dump-section .text=$co.text $co.co $co.tmp
        $LLVM/llvm-objcopy --dump-section .rodata=$co.rodata $co.co $co.tmp 2>/dev/null || : > $co.rodata
        rm -f $co.tmp
        $LLVM/llvm-readelf -s -W $co.co | grep -v __hip_cuid_ > $co.syms
        # (the marker's name moves other entries in the table: compared as a set -- value, size, type, binding, section, name)
        sed -E 's/^ *[0-9]+: *//' $co.syms | sort > $co.symset
        $LLVM/llvm-objdump -d $co.co | tail -n +3 > $co.dis       # (the first lines name the file)
        $LLVM/llvm-readelf --notes $co.co > $co.notes
        $LLVM/llvm-readelf -S -W $co.co | awk '$2 == ".text" || $3 == ".text" { for (i = 1; i <= NF; i++) if ($i == "PROGBITS") print $(i + 1) }' > $co.textaddr
        k=$((k + 1))
    done
    echo $k > $d/count
done
python3 - $tmp "${libs[0]}" "${libs[1]}" <<'PY'
import filecmp, os, re, subprocess, sys
tmp, la, lb = sys.argv[1:4]
print('A =', la)
print('B =', lb)
na, nb = (int(open('%s/%d/count' % (tmp, s)).read()) for s in (0, 1))
print('gfx950 code objects: A %d, B %d' % (na, nb))
differ = na != nb

def kernels(co):
    """name -> dict of the metadata note's fields, plus the size of the kernel's code from the symbol table"""
    out, cur = {}, None
    for line in open(co + '.notes'):
        m = re.match(r'\s*(- )?\.(\w+):\s*(\S+)\s*$', line)
        if not m:
            continue
        key, val = m.group(2), m.group(3)
        if key == 'agpr_count':            # first field of a kernel's entry (the fields are sorted by name)
            cur = {}
        if cur is None:
            continue
        cur[key] = val
        if key == 'name':
            out[val] = cur
    text = open(co + '.text', 'rb').read()
    base = int(open(co + '.textaddr').read().split()[0], 16)
    funcs = {}                             # every function of .text, kernels and non-inlined device functions: its bytes
    for line in open(co + '.syms'):
        f = line.split()
        if len(f) >= 8 and f[3] == 'FUNC':
            at = int(f[1], 16) - base
            funcs[f[7]] = text[at:at + int(f[2])]
    for k, v in out.items():
        v['size'] = len(funcs.get(k, b''))
    return out, funcs

FIELDS = (('size', 'size'), ('vgpr', 'vgpr_count'), ('agpr', 'agpr_count'), ('sgpr', 'sgpr_count'),
          ('scratch', 'private_segment_fixed_size'), ('lds', 'group_segment_fixed_size'))
max_scr = [0, 0]
all_k = [set(), set()]
text_delta = []
res_diff = []
for k in range(min(na, nb)):
    a, b = '%s/0/co%02d' % (tmp, k), '%s/1/co%02d' % (tmp, k)
    (ka, fa), (kb, fb) = kernels(a), kernels(b)
    all_k[0] |= set(ka); all_k[1] |= set(kb)
    same = {}
    for part in ('text', 'rodata', 'symset', 'dis'):
        same[part] = filecmp.cmp(a + '.' + part, b + '.' + part, shallow=False)
    ndis = ''
    if not same['dis']:
        r = subprocess.run(['diff', a + '.dis', b + '.dis'], stdout=subprocess.PIPE, text=True)
        ndis = ' (%d of %d lines)' % (sum(1 for l in r.stdout.splitlines() if l[:1] in '<>'), sum(1 for _ in open(a + '.dis')))
    names = sorted(ka)
    print('\ncode object %02d: %d kernels, first %s' % (k, len(ka), names[0][:70] if names else '-'))
    print('  .text %s  .rodata %s  symbols %s  disassembly %s%s' % tuple(
        ['identical' if same[p] else 'DIFFERS' for p in ('text', 'rodata', 'symset', 'dis')] + [ndis]))
    differ |= not all(same.values())
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            v = [int((ka.get(name) or kb[name]).get(f, -1)) for _, f in FIELDS]
            max_scr[0 if name in ka else 1] = max(max_scr[0 if name in ka else 1], v[4])
            print('  ONLY IN %s: %s' % ('A' if name in ka else 'B', name))
            print('  %-64s %s' % ('', ' '.join('%s=%d' % (lab, x) for (lab, _), x in zip(FIELDS, v))))
            differ = True
            continue
        va = [int(ka[name].get(f, -1)) for _, f in FIELDS]
        vb = [int(kb[name].get(f, -1)) for _, f in FIELDS]
        max_scr[0] = max(max_scr[0], va[4]); max_scr[1] = max(max_scr[1], vb[4])
        flags = [lab for (lab, _), x, y in zip(FIELDS, va, vb) if x != y]
        short = name.replace('_ZN2rt7k_stageIN3bbs', '')[:64]
        cell = lambda x, y: str(x) if x == y else '%d->%d' % (x, y)
        print('  %-64s %s%s' % (short, ' '.join('%s=%s' % (lab, cell(x, y)) for (lab, _), x, y in zip(FIELDS, va, vb)),
                                 ('   <-- ' + ','.join(flags)) if flags else ''))
        if fa[name] != fb[name]:
            text_delta.append((short, vb[0] - va[0]))
        hard = [f for f in flags if f not in ('size', 'sgpr')]      # (vgpr_count is the total: it includes the AGPRs)
        if hard:
            res_diff.append((short, hard))
    for name in sorted((set(fa) | set(fb)) - set(ka) - set(kb)):          # device functions that were not inlined
        x, y = fa.get(name), fb.get(name)
        print('  (function) %-53s size=%s%s' % (name[:53], len(x) if x is not None else '-', '' if x == y else '->%s   <-- code' % (len(y) if y is not None else '-')))
        if x != y:
            text_delta.append(('(function) ' + name[:53], (len(y) if y else 0) - (len(x) if x else 0)))
print('\nkernel symbols: A %d, B %d, %s' % (len(all_k[0]), len(all_k[1]), 'sets equal' if all_k[0] == all_k[1] else 'SETS DIFFER'))
print('largest scratch: A %d, B %d bytes%s' % (max_scr[0], max_scr[1], '' if max_scr[0] == max_scr[1] else '   <-- DIFFERS'))
print('kernels and functions whose code bytes differ: %d' % len(text_delta))
for n, d in text_delta:
    print('  %-64s %+d bytes' % (n, d))
print('kernels whose VGPR (total), AGPR, scratch or LDS differ: %d' % len(res_diff))
for n, f in res_diff:
    print('  %-64s %s' % (n, ','.join(f)))
print('RESULT:', 'code objects DIFFER' if differ else 'all code objects identical')
sys.exit(1 if differ else 0)
PY
