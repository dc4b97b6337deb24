#!/usr/bin/env python
"""Which kernels of a set of units compile to different device code in two source trees (no GPU needed).

    python tools/compare_kernel_asm.py OLD_TREE NEW_TREE [unit globs, comma-separated, default train_*.hip] [--md TABLE.md]

Each tree's units are compiled with the flags its own csrc/Makefile gives them (`make -n`), to device assembly.  The assembly is cut
into functions (`_Z...:` to its `.Lfunc_end`), comments and the function number of local labels dropped, and compared by mangled
name wherever the kernel lives in either tree, together with the values of the kernel's descriptor (`.amdhsa_*`: registers, LDS and scratch
sizes, kernarg size, ...).  Prints one line per kernel that differs, exists in one tree only or twice in one tree; exit status 1 if
any.  --md: also a table of every kernel (unit, instructions, registers, LDS, scratch, kernarg bytes, verdict) to that file.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

SHOWN = ('next_free_vgpr', 'next_free_sgpr', 'group_segment_fixed_size', 'private_segment_fixed_size', 'kernarg_size')


def kernels(tree, patterns):
    """{mangled name: (unit, code lines, {descriptor field: value}, times seen)}"""
    csrc = os.path.join(tree, 'panoptic-forecasting_amd', 'csrc')
    out = {}
    for src in sorted(s for p in patterns.split(',') for s in glob.glob(os.path.join(csrc, p))):
        unit = os.path.basename(src)[:-4]
        line = subprocess.run(['make', '-n', '-B', '-C', csrc, unit + '.o'], capture_output=True, text=True, check=True).stdout
        cmd = [ln for ln in line.split('\n') if ' -c ' in ln][0].split()
        cmd = cmd[:cmd.index('-c')] + ['--cuda-device-only', '-S', unit + '.hip', '-o']
        with tempfile.NamedTemporaryFile(suffix='.s') as f:
            subprocess.run(cmd + [f.name], cwd=csrc, check=True)
            text = open(f.name).read()
        desc = {m.group(1): dict(re.findall(r'^\s*\.amdhsa_(\S+)\s+(\S+)', m.group(2), re.M))
                for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel', text, re.M | re.S)}
        for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', text, re.M | re.S):
            body = [re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0]).rstrip() for ln in m.group(2).split('\n')]
            seen = out[m.group(1)][3] if m.group(1) in out else 0
            out[m.group(1)] = (unit, [ln for ln in body if ln], desc.get(m.group(1), {}), seen + 1)
    return out


def demangled(names):
    try:
        lines = subprocess.run(['c++filt'] + names, capture_output=True, text=True, check=True).stdout.split('\n')
        return dict(zip(names, (re.sub(r'\(.*', '', ln).replace('void ', '') for ln in lines)))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    argv = sys.argv[1:]
    md = argv.pop(argv.index('--md') + 1) if '--md' in argv else None
    argv = [a for a in argv if a != '--md']
    pattern = argv[2] if len(argv) > 2 else 'train_*.hip'
    old, new = kernels(argv[0], pattern), kernels(argv[1], pattern)
    pretty = demangled(sorted(set(old) | set(new)))
    rows = ['| kernel | unit | instructions | VGPRs | SGPRs | LDS | scratch | kernarg | against the old tree |', '|---|---|---|---|---|---|---|---|---|']
    bad = 0
    for name in sorted(set(old) | set(new), key=lambda n: pretty[n]):
        o, n = old.get(name), new.get(name)
        if not o or not n:
            verdict = 'ONLY IN %s (%s)' % ('OLD' if o else 'NEW', (o or n)[0])
        elif o[3] != 1 or n[3] != 1:
            verdict = 'TWICE IN ONE TREE (%s -> %s)' % (o[0], n[0])
        elif o[1] != n[1]:
            verdict = 'DIFFERS (%s -> %s, %d -> %d lines)' % (o[0], n[0], len(o[1]), len(n[1]))
        elif o[2] != n[2]:
            verdict = 'DESCRIPTOR DIFFERS (%s -> %s): %s' % (o[0], n[0], ', '.join('%s %s -> %s' % (f, o[2].get(f), n[2].get(f))
                                                                                  for f in sorted(set(o[2]) | set(n[2])) if o[2].get(f) != n[2].get(f)))
        else:
            verdict = None
        if verdict:
            print('%s: %s' % (verdict, name))
            bad += 1
        k = n or o
        count = len([ln for ln in k[1] if not ln.endswith(':') and not ln.lstrip().startswith('.')])
        rows.append('| `%s` | %s | %d | %s | %s |' % (pretty[name], k[0], count, ' | '.join(k[2].get(f, '') for f in SHOWN), verdict or 'same code, same descriptor'))
    summary = '%d kernels in the old tree, %d in the new, %d differ or are missing' % (len(old), len(new), bad)
    print(summary)
    if md:
        with open(md, 'w') as f:
            f.write('\n'.join(rows + ['', summary]) + '\n')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
