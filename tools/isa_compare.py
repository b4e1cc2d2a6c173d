#!/usr/bin/env python3
"""Compare two hipcc -S --cuda-device-only listings kernel by kernel.  usage: tools/isa_compare.py [--by-template] a.s b.s

Of each kernel only the instruction lines count: comments, directives and the trailing `;` annotations are dropped and
.LBB labels replaced by a placeholder.  Every kernel lands in the first class that holds:
  identical     the same instruction stream
  regs-only     the same opcodes in the same order; operands equal once register numbers and the offsets from the
                kernel-argument pointer (scalar loads, the s_add_u32 towards the implicit arguments) are masked: what a
                changed kernel-argument list does
  opcode-seq    the same opcodes in the same order
  multiset      the same opcodes, in another order
  differ        anything else
--by-template pairs kernels by their demangled name without the argument list (for a changed kernel signature).
Exit status 0 when every kernel of both listings was paired and is identical (or, with --by-template, regs-only)."""
import collections
import re
import shutil
import subprocess
import sys


def kernels(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif ln.startswith('.Lfunc_end'):
            cur = None
        elif cur is not None and ln.startswith('\t') and not ln.strip().startswith(('.', ';')):
            cur.append(re.sub(r'\.LBB\d+_\d+', '.LBB', ln.split(';')[0].strip()))
    return out


def by_template(ks):
    names = list(ks)
    filt = shutil.which('llvm-cxxfilt') or shutil.which('llvm-cxxfilt', path='/opt/rocm/lib/llvm/bin') or 'c++filt'
    dem = subprocess.run([filt], input='\n'.join(names), capture_output=True, text=True, check=True)
    return {re.sub(r'\(.*', '', d): ks[n] for n, d in zip(names, dem.stdout.split('\n'))}


def masked(ins):
    ins = re.sub(r'\b([sva])\[\d+:\d+\]', r'\1[]', ins)
    ins = re.sub(r'\b([sva])\d+\b', r'\1#', ins)
    # offsets from the kernel-argument pointer: the scalar loads, and the add that forms the implicit arguments' pointer
    return re.sub(r'(0x[0-9a-f]+|\d+)$', '#', ins) if ins.startswith(('s_load_', 's_add_u32')) else ins


def classify(a, b):
    if a == b:
        return 'identical'
    oa, ob = [i.split()[0] for i in a], [i.split()[0] for i in b]
    if oa == ob:
        return 'regs-only' if [masked(i) for i in a] == [masked(i) for i in b] else 'opcode-seq'
    return 'multiset' if collections.Counter(oa) == collections.Counter(ob) else 'differ'


def main():
    args = [a for a in sys.argv[1:] if a != '--by-template']
    tmpl = len(args) != len(sys.argv) - 1
    a, b = kernels(args[0]), kernels(args[1])
    if tmpl:
        a, b = by_template(a), by_template(b)
    tally = collections.Counter()
    for name in sorted(set(a) & set(b)):
        c = classify(a[name], b[name])
        tally[c] += 1
        if c != 'identical' and not (tmpl and c == 'regs-only'):
            print(f'{c:12s} {len(a[name]):6d} {len(b[name]):6d}  {name}')
    for name in sorted(set(a) ^ set(b)):
        print(f"{'only in ' + ('a' if name in a else 'b'):12s} {name}")
    paired = len(set(a) & set(b))
    print(f'kernels: {len(a)} | {len(b)}, paired {paired}: ' + ', '.join(f'{k} {v}' for k, v in sorted(tally.items())))
    good = tally['identical'] + (tally['regs-only'] if tmpl else 0)
    sys.exit(0 if paired == len(a) == len(b) == good else 1)


if __name__ == '__main__':
    main()
