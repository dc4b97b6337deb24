"""File side of the ego chain: Cityscapes timestamps / vehicle JSON + the odometry forecaster's export.

What the reference reads before ``PCTransformModel.predict`` is entered (``data/datasets/pc_transform_dataset.py:103-186``):

  ``timestamp_sequence/{split}/{city}/{city}_{seq}_{fr:06d}_timestamp.txt``   one integer, nanoseconds
  ``vehicle_sequence/{split}/{city}/{city}_{seq}_{fr:06d}_vehicle.json``      ``speed`` [m/s], ``yawRate`` [rad/s]
  ``{odom_pred_dir}/{odom_name}_{split}.h5``                                  written by experiments/export_cityscapes_odom.py:37-54:
        dataset ``'%s/%s/%d/%d' % (city, seq, frame, start_frame)`` = ``[n_future, 2]`` rows ``[speed, yaw_rate]``

for the 30 frames ``frame-19 .. frame+10`` of a snippet whose annotated frame is ``frame`` (index 19).  ``OdometryFile``
opens the export (HDF5 through ``h5py`` when it is installed; the same keys in an ``.npz`` archive otherwise — this
image has no h5py, and ``convert_h5_to_npz`` is the one-liner to run where it exists); ``snippet_target_T`` turns one
snippet into the ``target_T [3,4,4]`` the warp consumes, through ``ego.target_T_predicted`` / ``ego.target_T_measured``.
Pinned by tests/golden/g1_odom.npz: outputs of the reference's own dataset constructor on a synthetic directory.
"""
import json
import os

import numpy as np

from . import ego

BASE_INPUT_INDS = np.array([0, 3, 6])       # pc_transform_dataset.py:81
TARGET_INDEX = 19                           # the annotated frame inside the 30-frame snippet (:80)


def odom_key(city, seq, frame, start_frame):
    """export_cityscapes_odom.py:52 / pc_transform_dataset.py:153 (frame is NOT zero-padded here, unlike the depth H5)."""
    return '%s/%s/%d/%d' % (city, seq, int(frame), int(start_frame))


def input_indices(gap_len, target=TARGET_INDEX):
    """pc_transform_dataset.py:94: indices (inside the snippet) of the three input frames."""
    return BASE_INPUT_INDS + target - (6 + gap_len)


class OdometryFile:
    """Read-only view of ``odometry_{split}.h5`` (or its ``.npz`` twin): ``rows(city, seq, frame, start_frame)``."""

    def __init__(self, path):
        self.path = path
        self._h5 = self._npz = None
        if path.endswith('.npz'):
            self._npz = np.load(path)
        else:
            try:
                import h5py
            except ImportError as e:
                twin = os.path.splitext(path)[0] + '.npz'
                if not os.path.exists(twin):
                    raise ImportError('%s is HDF5 and h5py is not installed; convert it once with odom_io.convert_h5_to_npz '
                                      '(needs h5py) or pass the .npz twin' % path) from e
                self._npz = np.load(twin)
            else:
                self._h5 = h5py.File(path, 'r')

    def rows(self, city, seq, frame, start_frame):
        key = odom_key(city, seq, frame, start_frame)
        src = self._h5 if self._h5 is not None else self._npz
        if key not in src:
            raise KeyError('%s has no odometry forecast %r' % (self.path, key))
        return np.asarray(src[key][:] if self._h5 is not None else src[key])

    def close(self):
        if self._h5 is not None:
            self._h5.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


SNIPPET_LEN = 30            # rows of ``odometry`` per snippet in ``{split}_3d_info.pkl``
WINDOW_ROWS = 18            # odom_dataset.py:76 (``np.arange(18)``, independent of input_len / output_len)


def odom_windows(odometry, input_len=9, output_len=9, test=True):
    """The odometry forecaster's windows of one snippet (``OdomDataset``, odom_dataset.py:73-83,94-121).

    ``odometry`` [30, >= 2] (columns ``[:, :2]`` = speed, yaw_rate are used).  Returns ``(inputs [N, input_len, 2],
    labels [N, output_len, 2], start_frames [N])`` as float32 / float32 / int64 in the dataset's order: ``start_ind`` 0 ..
    30 - input_len with ``test`` (the export's windows; rows ``start_ind + arange(18)`` clipped at 29; inputs = the first
    input_len rows, labels = the rest) or 0 .. 30 - input_len - output_len without (the training windows, :73-81: every
    label row is a measured one), then the two padded windows ``start_ind`` -1 and -2 (first row repeated; labels = the
    last output_len rows of ``arange(18)[:-k]``).  ``start_frames`` = snippet index of the last input row = the export
    key's last field.
    """
    odom = np.asarray(odometry)[:, :2].astype(np.float32)
    inds = np.arange(WINDOW_ROWS)
    wins = [(s, (s + inds).clip(max=SNIPPET_LEN - 1)) for s in range(SNIPPET_LEN - input_len + 1 - (0 if test else output_len))]
    wins += [(-1, inds[:-1]), (-2, inds[:-2])]
    inputs, labels, starts = [], [], []
    for start, cur in wins:
        o = odom[cur]
        if start < 0:
            inputs.append(np.concatenate([np.repeat(o[0:1], -start, 0), o[:input_len + start]]))
            labels.append(o[-output_len:])
            starts.append(cur[input_len - 1 + start])
        else:
            inputs.append(o[:input_len])
            labels.append(o[input_len:])
            starts.append(cur[input_len - 1])
    return np.stack(inputs), np.stack(labels), np.asarray(starts, dtype=np.int64)


FG_FUTURE_ROWS = (2, 5, 8)  # fg_scene_dataset.py:489: the forecast rows the fg model takes


def fg_odometry(inp_odom, odom_preds, inp_times):
    """The odometry ``FGModel`` consumes with predicted odometry (fg_scene_dataset.py:465-492), float32 [T_in + 3, 5].

    ``inp_odom`` [T_in, 5] measured rows of the input frames, ``odom_preds`` [>= 9, 2] this snippet's forecast (the export's
    rows), ``inp_times`` the timestamps of every frame from the first to the last input frame: each forecast row becomes
    ``[speed, yaw_rate, x, y, theta]`` with the planar motion of ``dt = mean(diff(inp_times))`` (``ego.planar_motion``),
    and rows 2, 5 and 8 follow the inputs.
    """
    times = np.asarray(inp_times)
    dt = np.mean(times[1:] - times[:-1])
    rows = []
    for speed, yaw_rate in np.asarray(odom_preds)[:, :2]:
        x, y, theta = ego.planar_motion(speed, yaw_rate, dt)
        rows.append(np.array([speed, yaw_rate, x, y, theta]))
    final = np.stack(rows)[list(FG_FUTURE_ROWS)]
    return np.concatenate([np.asarray(inp_odom), final]).astype(np.float32)


def write_npz(path, entries):
    """entries: {(city, seq, frame, start_frame): [n,2] array} -> .npz with the H5 key names."""
    np.savez_compressed(path, **{odom_key(*k): np.asarray(v, dtype=np.float32) for k, v in entries.items()})


def convert_h5_to_npz(h5_path, npz_path=None):
    import h5py
    out = {}
    with h5py.File(h5_path, 'r') as f:
        def visit(name, obj):
            if isinstance(obj, h5py.Dataset):
                out[name] = obj[:]
        f.visititems(visit)
    npz_path = npz_path or os.path.splitext(h5_path)[0] + '.npz'
    np.savez_compressed(npz_path, **out)
    return npz_path


def read_snippet(cityscapes_dir, split, city, seq, frame):
    """(times [30] seconds, speeds [30], yaw_rates [30]) of frames frame-19 .. frame+10 (:103-116,132-147)."""
    times, speeds, yaws = [], [], []
    for fr in range(frame - TARGET_INDEX, frame + 11):
        stem = '%s_%s_%06d' % (city, seq, fr)
        with open(os.path.join(cityscapes_dir, 'timestamp_sequence', split, city, stem + '_timestamp.txt')) as f:
            times.append(float(f.read()) / 1e9)
        with open(os.path.join(cityscapes_dir, 'vehicle_sequence', split, city, stem + '_vehicle.json')) as f:
            v = json.load(f)
        speeds.append(v.get('speed'))
        yaws.append(v.get('yawRate'))
    return np.asarray(times), speeds, yaws


def snippet_target_T(cityscapes_dir, split, city, seq, frame, gap_len, odom=None, target=TARGET_INDEX):
    """``target_T [3,4,4]`` float64 for one snippet.  ``odom``: an ``OdometryFile`` (predicted-odometry branch, the
    mid-/short-term *forecasting* configuration, :156-186) or None (measured odometry up to the target, :219-231)."""
    times, speeds, yaws = read_snippet(cityscapes_dir, split, city, seq, frame)
    inds = input_indices(gap_len, target)
    if odom is None:
        return ego.target_T_measured(speeds, yaws, times, inds, target)
    preds = odom.rows(city, seq, frame, inds[-1])
    return ego.target_T_predicted(speeds, yaws, times, preds, inds, target, gap_len)
