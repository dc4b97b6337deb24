#!/usr/bin/env python3
"""Write what pf_debug_net_choice answers for every case of tests/stem_ref64.py and tests/head_ref64.py, one markdown table row per
launch: the profile label, grid, workgroup size and dynamic LDS bytes, or the error code of a refusal.  No GPU involved.

    tools/dump_net_choice.py [--lib PATH/libpfhip.so] OUT.md

Two libraries whose files are equal launch these cases alike (profiles/net_kernels_split.md compares this tree with its parent, whose
launchers were given the same entry in a scratch copy).
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', help='the library to ask (default: the one of this tree)')
    ap.add_argument('out')
    args = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime must be mapped first, see lib.load)
    import head_ref64 as H
    import stem_ref64 as R
    from panoptic_forecasting_amd import lib as pflib
    L = ctypes.CDLL(args.lib or pflib.LIB_PATH)
    L.pf_debug_net_choice.restype = ctypes.c_int

    def ask(what, iargs, fargs=()):
        ia, fa = (ctypes.c_int * len(iargs))(*iargs), (ctypes.c_float * 4)(*fargs)
        label, out = ctypes.create_string_buffer(128), (ctypes.c_longlong * 8)()
        rc = L.pf_debug_net_choice(what, ia, len(iargs), fa if fargs else None, len(fargs), label, ctypes.c_size_t(128), out, 8)
        return '| `%s` | %d x %d x %d | %d | %d |' % (label.value.decode(), out[1], out[2], out[3], out[4], out[5]) if rc == 0 else '| refused: %d | | | |' % rc

    rows = ['| case | run | label | grid | lanes | LDS bytes |', '|---|---|---|---|---|---|']
    for c in R.CASES:
        for hop in R.HOPS:
            # (the parameter set matters to v4 under the depth hop only: the set with an infinite std too; dst_fmt = 1 once per case)
            for ps in (0, R.INF_STD_SET) if c.family == 'v4' and hop & R.PF_HOP_DEPTH_U16 else (0,):
                for fmt in (0, 1) if hop == 0 else (0,):
                    iargs = [c.T, c.n_cls, c.h, c.w, (c.h + 1) // 2, (c.w + 1) // 2, c.b, int(c.i64), hop, fmt, 1]
                    rows.append('| stem %s | hop %d, set %d, dst_fmt %d %s' % (c.name, hop, ps, fmt, ask(0, iargs, R.ALL_SETS[ps])))
    for c in H.HEAD_CASES:
        rows.append('| head %s B%d | %s' % (c.name, c.b, ask(1, [c.b, c.c, c.hin, c.win, c.ho, c.wo])))
    for c in H.LOSS_CASES + H.HEAD_CASES:
        rows.append('| loss %s B%d | %s' % (c.name, c.b, ask(2, [c.b, c.c, c.hin, c.win, c.ho, c.wo])))
    with open(args.out, 'w') as f:
        f.write('\n'.join(rows) + '\n')
    print('%d rows' % (len(rows) - 2))


if __name__ == '__main__':
    main()
