"""Instance maps for the ground-truth preparation tests and tools/bench_gt_prep.py: hand-made 4x8 maps, one per rule, and a seeded
generator of blocky street-like maps with instances."""
import os

import numpy as np

THINGS = (24, 25, 26, 27, 28, 31, 32, 33)
STUFF = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23)
IGNORED = (0, 1, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18)


def hand_made():
    """{name: [4,8] int64 map}."""
    road = np.full((4, 8), 7, np.int64)
    out = {}
    m = road.copy(); m[1:3, 2:5] = 26                        # a car crowd region: v = 26, iscrowd 1
    out['crowd'] = m
    m = road.copy(); m[0, :3] = 7001; m[3, 5:] = 7001        # a stuff label with an instance part: listed, iscrowd 0
    out['stuff_instance'] = m
    m = road.copy(); m[0:2, 0:2] = 29003; m[2, 3:6] = 4; m[3, :] = 1; m[0, 6:] = 30000; m[1, 7] = 10   # unlisted, black, 255
    out['ignored'] = m
    m = road.copy(); m[1, 1:4] = 24999; m[2, 2:7] = 33999; m[0, 0] = 24000   # instance indices 0 and 999
    out['index_999'] = m
    m = road.copy(); m[2, 5] = 25001; m[0, 7] = 23           # one-pixel segments, one in a corner
    out['one_pixel'] = m
    m = np.full((4, 8), 26005, np.int64); m[1:3, 1:7] = 21   # a segment touching all four borders around another
    out['borders'] = m
    return out


def blocky(h, w, seed, n_things=40, block=16):
    """A street-like [h,w] int64 map: blocks of stuff and ignored labels in long runs, rectangles of thing instances over them
    (later ones cover earlier ones, so some boxes are cut or hidden), a crowd region and a stuff instance."""
    rng = np.random.default_rng(seed)
    pool = np.array(STUFF + IGNORED[:4])
    low = pool[rng.integers(0, len(pool), ((h + block - 1) // block, (w + block - 1) // block))]
    m = np.repeat(np.repeat(low, block, 0), block, 1)[:h, :w].astype(np.int64)
    m[: max(1, h // 3)] = 23                                  # sky: one long segment
    counts = {}
    for _ in range(n_things):
        label = int(THINGS[rng.integers(0, len(THINGS))])
        k = counts.get(label, 0)
        counts[label] = k + 1
        bh, bw = int(rng.integers(1, max(2, h // 4))), int(rng.integers(1, max(2, w // 6)))
        y, x = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
        m[y:y + bh, x:x + bw] = label * 1000 + k
    m[h - 1, : max(1, w // 5)] = 26                           # a car crowd
    m[h // 2, w // 2:] = 8001                                 # a stuff label with an instance part
    m[0, 0] = 29000 + 7                                       # a caravan
    return m


def worst_case_96x256():
    """[96,256]: 24 576 pixels, more than one workgroup's 16 384.  Segment 26001 frames the image (its box spans every workgroup),
    31001 and 31002 interleave row by row inside it (no run survives a lane's next unit), 24001 alternates pixel by pixel with road."""
    m = np.full((96, 256), 26001, np.int64)
    m[1:95:2, 1:255] = 31001
    m[2:95:2, 1:255] = 31002
    m[40:44, 8:200:2] = 24001
    m[40:44, 9:200:2] = 7
    return m


def many_ids(h, w, count):
    """[h,w] with `count` distinct listed ids, one run each, in descending order of value along the rows."""
    assert count <= h * w and count <= 19 * 1000
    listed = [l * 1000 + k for l in THINGS + STUFF for k in range(1000)][:count]
    flat = np.array(listed[::-1], np.int64)[np.arange(h * w) * count // (h * w)]
    return flat.reshape(h, w)


def write_tree(root, maps, set_name='val', bits=16):
    """<root>/<set>/<city>/<city>_<i>_000019_gtFine_instanceIds.png for each map, two cities; returns the files in sorted order."""
    from PIL import Image
    files = []
    for i, m in enumerate(maps):
        city = 'city%d' % (i % 2)
        os.makedirs(os.path.join(root, set_name, city), exist_ok=True)
        path = os.path.join(root, set_name, city, '%s_%06d_000019_gtFine_instanceIds.png' % (city, i))
        Image.fromarray(np.asarray(m).astype(np.uint16 if bits == 16 else np.int32)).save(path)
        files.append(path)
    return sorted(files)
