#!/usr/bin/env python
"""Which kernels of the training units compile to a different instruction stream in two source trees (no GPU needed).

    python tools/compare_kernel_asm.py OLD_TREE NEW_TREE [unit glob, default train_*.hip]

Each tree's units are compiled with the flags its own csrc/Makefile gives them (`make -n`), to device assembly.  The assembly is cut
into functions (`_Z...:` to its `.Lfunc_end`), comments and the function number of local labels dropped, and compared by mangled
name wherever the kernel lives in either tree.  Prints one line per kernel that differs or exists in one tree only; exit status 1 if any.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile


def kernels(tree, pattern):
    csrc = os.path.join(tree, 'panoptic-forecasting_amd', 'csrc')
    out = {}
    for src in sorted(glob.glob(os.path.join(csrc, pattern))):
        unit = os.path.basename(src)[:-4]
        line = subprocess.run(['make', '-n', '-B', '-C', csrc, unit + '.o'], capture_output=True, text=True, check=True).stdout
        cmd = [ln for ln in line.split('\n') if ' -c ' in ln][0].split()
        cmd = cmd[:cmd.index('-c')] + ['--cuda-device-only', '-S', unit + '.hip', '-o']
        with tempfile.NamedTemporaryFile(suffix='.s') as f:
            subprocess.run(cmd + [f.name], cwd=csrc, check=True)
            text = open(f.name).read()
        for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', text, re.M | re.S):
            body = [re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0]).rstrip() for ln in m.group(2).split('\n')]
            out[m.group(1)] = (unit, [ln for ln in body if ln])
    return out


def main():
    pattern = sys.argv[3] if len(sys.argv) > 3 else 'train_*.hip'
    old, new = kernels(sys.argv[1], pattern), kernels(sys.argv[2], pattern)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in new or name not in old:
            print('ONLY IN %s (%s): %s' % ('OLD' if name in old else 'NEW', (old.get(name) or new[name])[0], name))
        elif old[name][1] != new[name][1]:
            print('DIFFERS (%s -> %s, %d -> %d lines): %s' % (old[name][0], new[name][0], len(old[name][1]), len(new[name][1]), name))
        else:
            continue
        bad += 1
    print('%d kernels in the old tree, %d in the new, %d differ or are missing' % (len(old), len(new), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
