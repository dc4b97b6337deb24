#!/usr/bin/env python
"""Golden fixture G14 for the no-foreground ground truth, produced by the REFERENCE itself (build container only).

    python tests/golden/make_golden_gtprep.py

``scripts/preprocessing/remove_fg_from_gt.py`` of the reference is run unmodified through ``runpy`` on a tiny temporary tree of
``<city>/*_gtFine_labelTrainIds.png`` files.  ``cityscapesscripts.helpers.labels`` is absent: a stand-in module exposes the public
Cityscapes label table's ``trainId`` / ``hasInstances`` / ``ignoreInEval`` columns, which is all the script reads (as
make_golden_fg.py does for the trainId -> id table).  Only the input and output label maps are recorded:
  g14_gtprep.npz   inputs [4,16,32] u8 (every byte value occurs), outputs [4,16,32] u8
"""
import os
import runpy
import sys
import tempfile
import types
from collections import namedtuple

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402

SCRIPT = os.path.join(_ref_import.REF_ROOT, 'scripts', 'preprocessing', 'remove_fg_from_gt.py')

_Label = namedtuple('Label', ['id', 'trainId', 'hasInstances', 'ignoreInEval'])
#         id: (trainId, hasInstances, ignoreInEval) - the public table
_ROWS = {0: (255, 0, 1), 1: (255, 0, 1), 2: (255, 0, 1), 3: (255, 0, 1), 4: (255, 0, 1), 5: (255, 0, 1), 6: (255, 0, 1), 7: (0, 0, 0),
         8: (1, 0, 0), 9: (255, 0, 1), 10: (255, 0, 1), 11: (2, 0, 0), 12: (3, 0, 0), 13: (4, 0, 0), 14: (255, 0, 1), 15: (255, 0, 1),
         16: (255, 0, 1), 17: (5, 0, 0), 18: (255, 0, 1), 19: (6, 0, 0), 20: (7, 0, 0), 21: (8, 0, 0), 22: (9, 0, 0), 23: (10, 0, 0),
         24: (11, 1, 0), 25: (12, 1, 0), 26: (13, 1, 0), 27: (14, 1, 0), 28: (15, 1, 0), 29: (255, 1, 1), 30: (255, 1, 1),
         31: (16, 1, 0), 32: (17, 1, 0), 33: (18, 1, 0), -1: (-1, 0, 1)}


def install_stand_ins():
    cs = types.ModuleType('cityscapesscripts')
    csh = types.ModuleType('cityscapesscripts.helpers')
    csl = types.ModuleType('cityscapesscripts.helpers.labels')
    csl.labels = [_Label(i, t, bool(h), bool(g)) for i, (t, h, g) in _ROWS.items()]
    sys.modules.update({'cityscapesscripts': cs, 'cityscapesscripts.helpers': csh, 'cityscapesscripts.helpers.labels': csl})
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            t = types.ModuleType('tqdm')
            t.tqdm = lambda x, **k: x
            sys.modules['tqdm'] = t


def make_inputs():
    rng = np.random.default_rng(14)
    maps = np.zeros((4, 16, 32), np.uint8)
    maps[0] = np.arange(512, dtype=np.int64).reshape(16, 32) % 256                      # every byte value, twice
    maps[1] = rng.integers(0, 19, (16, 32))
    maps[2] = np.repeat(np.repeat(rng.integers(0, 20, (4, 8)), 4, 0), 4, 1)             # blocks; 19 is no trainId
    maps[2][maps[2] == 19] = 255
    maps[3] = np.where(rng.random((16, 32)) < 0.5, rng.integers(11, 19, (16, 32)), 255)   # things and void only
    return maps


def main():
    install_stand_ins()
    sys.dont_write_bytecode = True
    maps = make_inputs()
    names = [('aachen', 'aachen_000000_000019'), ('aachen', 'aachen_000001_000019'), ('bochum', 'bochum_000000_000313'),
             ('bochum', 'bochum_000001_000313')]
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, 'in'), os.path.join(tmp, 'out')
        for m, (city, name) in zip(maps, names):
            os.makedirs(os.path.join(src, city), exist_ok=True)
            Image.fromarray(m).save(os.path.join(src, city, name + '_gtFine_labelTrainIds.png'))
        argv, sys.argv = sys.argv, [SCRIPT, '--input_dir', src, '--output_dir', dst]
        try:
            runpy.run_path(SCRIPT, run_name='__main__')
        finally:
            sys.argv = argv
        outs = np.stack([np.array(Image.open(os.path.join(dst, city, name + '_gtFine_labelTrainIds.png'))) for city, name in names])
    assert outs.dtype == np.uint8 and outs.shape == maps.shape
    path = os.path.join(HERE, 'g14_gtprep.npz')
    np.savez_compressed(path, inputs=maps, outputs=outs)
    print('g14_gtprep.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
