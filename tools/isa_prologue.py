#!/usr/bin/env python3
"""isa_prologue.py -- what stands in front of the first matrix instruction of a kernel, and whether two builds agree on what lies
between the first and the last one (the Winograd forward's block set-up).
Usage: isa_prologue.py <object | library.so> <kernel-name substring> [<other object | library> to compare the matrix window with]
Prints per matching kernel: VGPRs / scratch / LDS from the code object's metadata; the instruction count in front of the first MFMA and
behind the last one; where the first global load stands; vector-ALU reciprocals and v_readfirstlane in front of the first MFMA (the
signature of a uniform division done on the vector ALU); the rounds of `s_load` + wait; and, with a second file, whether the mnemonic
sequence from the first to the last MFMA (operands ignored: register names may differ) is the same in both."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = '/opt/rocm/lib/llvm/bin/'


def code_object(path):
    tmp = tempfile.mkdtemp()
    co = os.path.join(tmp, 'co')
    r = subprocess.run([LLVM + 'clang-offload-bundler', '--type=o', '--unbundle', '--input=' + path,
                        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co], capture_output=True, text=True)
    if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co):
        return co
    fat = os.path.join(tmp, 'fat')
    subprocess.run(['objcopy', '-O', 'binary', '--only-section=.hip_fatbin', path, fat], check=True)
    subprocess.run([LLVM + 'clang-offload-bundler', '--type=o', '--unbundle', '--input=' + fat,
                    '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co], check=True)
    return co


def kernels(path, pat):
    """{demangled name: {'ins': [(mnemonic, line)], 'vgpr', 'scratch', 'lds'}} of the kernels whose name contains pat"""
    co = code_object(path)
    txt = subprocess.run([LLVM + 'llvm-objdump', '-d', '--demangle', co], capture_output=True, text=True).stdout
    notes = subprocess.run([LLVM + 'llvm-readelf', '--notes', co], capture_output=True, text=True).stdout
    meta = {}
    for ent in re.split(r'\n\s+- \.', '\n' + notes):
        sym = re.search(r'\.symbol:\s+(\S+?)\.kd', ent)
        if not sym:
            continue
        def num(key):
            m = re.search(r'\.%s:\s+(\d+)' % key, ent)
            return int(m.group(1)) if m else None
        meta[sym.group(1).strip("'")] = (num('vgpr_count'), num('private_segment_fixed_size'), num('group_segment_fixed_size'))
    mangled = subprocess.run([LLVM + 'llvm-objdump', '-d', co], capture_output=True, text=True).stdout
    mnames = re.findall(r'\n[0-9a-f]+ <([^>]+)>:', mangled)
    out = {}
    for blk, mname in zip(re.split(r'\n(?=[0-9a-f]+ <)', txt)[1:], mnames):
        head = blk.split('\n', 1)[0]
        if pat not in head:
            continue
        ins = []
        for line in blk.split('\n')[1:]:
            m = re.match(r'\s+(\S+)\s.*//\s*[0-9A-Fa-f]+:', line) or re.match(r'\s+(s_\w+)\s+//', line)
            if m:
                ins.append((m.group(1), line.split('//')[0].strip()))
        v, s, l = meta.get(mname, (None, None, None))
        out[re.sub(r'^[0-9a-f]+ <|>:$', '', head)] = {'ins': ins, 'vgpr': v, 'scratch': s, 'lds': l}
    return out


def window(ins):
    mf = [i for i, (o, _) in enumerate(ins) if o.startswith('v_mfma')]
    return (mf[0], mf[-1]) if mf else (None, None)


def describe(name, k):
    ins = k['ins']
    first, last = window(ins)
    print('==', name[:170])
    print('   vgprs %s  scratch %s  lds %s  | %d instructions, first MFMA at %s, last at %s (%d behind it)' % (
        k['vgpr'], k['scratch'], k['lds'], len(ins), first, last, len(ins) - 1 - last))
    pro = ins[:first]
    gl = [i for i, (o, _) in enumerate(pro) if o.startswith('buffer_load') or o.startswith('global_load')]
    print('   in front of the first MFMA: first global load at %s, %d global loads; v_rcp* %d, v_readfirstlane %d' % (
        gl[0] if gl else None, len(gl), sum(1 for o, _ in pro if o.startswith('v_rcp')),
        sum(1 for o, _ in pro if o.startswith('v_readfirstlane'))))
    rounds, open_round = [], None
    for i, (o, t) in enumerate(pro):
        if o.startswith('s_load'):
            if open_round is None:
                open_round = i
            last_load = i
        elif o == 's_waitcnt' and 'lgkmcnt(0)' in t and open_round is not None:
            rounds.append((open_round, last_load, i))
            open_round = None
    print('   scalar-load rounds (first load, last load, wait):', rounds)
    if gl:
        waits = [i for i, (o, t) in enumerate(pro) if o == 's_waitcnt' and 'vmcnt' in t and i > gl[0]]
        print('   first wait on a global load at %s: %d instructions behind the last load of the first group' % (
            waits[0] if waits else None, (waits[0] - max(g for g in gl if g < waits[0]) - 1) if waits else -1))


def main():
    a = kernels(sys.argv[1], sys.argv[2])
    b = kernels(sys.argv[3], sys.argv[2]) if len(sys.argv) > 3 else None
    rc = 0
    for name, k in a.items():
        describe(name, k)
        if b is not None:
            if name not in b:
                print('   (not in %s)' % sys.argv[3])
                continue
            f0, l0 = window(k['ins'])
            f1, l1 = window(b[name]['ins'])
            wa = [o for o, _ in k['ins'][f0:l0 + 1]]
            wb = [o for o, _ in b[name]['ins'][f1:l1 + 1]]
            same = wa == wb
            print('   matrix window: %d instructions here, %d there: %s; vgprs there %s, lds there %s' % (
                len(wa), len(wb), 'SAME mnemonic sequence' if same else 'DIFFERENT', b[name]['vgpr'], b[name]['lds']))
            if not same:
                rc = 1
                import collections
                import difflib
                ca, cb = collections.Counter(wa), collections.Counter(wb)
                print('   only here: %s; only there: %s' % (dict(ca - cb), dict(cb - ca)))
                heavy = lambda w: [o for o in w if o.startswith(('v_mfma', 'ds_', 'buffer_', 'global_'))]
                print('   MFMA / LDS / global-memory instructions alone, in order: %s' % ('SAME' if heavy(wa) == heavy(wb) else 'DIFFERENT'))
                for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, wb, wa, autojunk=False).get_opcodes():
                    if tag != 'equal':
                        print('   %s: there [%d] %s | here [%d] %s' % (tag, i1, wb[i1:i2], j1, wa[j1:j2]))
    return rc


if __name__ == '__main__':
    sys.exit(main())
