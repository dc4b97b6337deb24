#!/usr/bin/env python
"""Training driver for ``task: odom`` with the reference's flags — drop-in for ``experiments/train_model.py`` as launched by
``scripts/odom/run_odom_train.sh``:

    python -u panoptic-forecasting_amd/train_odom.py --config_file configs/odom/odom_train.yaml --working_dir experiments/odom/
    python -u panoptic-forecasting_amd/train_odom.py --continue_training --working_dir experiments/odom/

What it keeps from the reference loop (``training/train.py:66-305``): the ``training.*`` keys (``batch_size``,
``num_epochs``, ``steps_per_epoch``, ``lr``/``mom``/``wd``, ``use_adam`` / ``use_adamw``, ``clip_grad`` | ``clip_grad_norm``,
``accumulate_steps``, the learning-rate decay of ``train_bg.learning_rate``, ``val_interval``), the epoch structure (train,
validate, keep the best), the files in ``working_dir`` (``config.yaml``, ``model_checkpoint`` and ``best_model`` = bare
state_dicts with the reference's 8 keys, ``training_checkpoint`` = {epoch, optimizer, best_val_result, best_val_epoch,
step}) and the per-epoch reseeding.  The optimiser is ``torch.optim`` and clipping is torch's own; what is native is
``OdomModel.loss``: one launch for the forward and three for back-propagation through time (csrc/odom_train.hip).

Data: the training windows of every snippet of ``{data.data_dir}/{split}_3d_info.pkl`` (``odom_io.odom_windows(test=False)``
= ``OdomDataset``, 15 per snippet at 9 in / 9 out) stay resident on the GPU - a whole split is a few MB - and a batch is an
index_select: one ``randperm`` per pass with ``drop_last`` for training, sequential for validation.  The normalisation
parameters are the train split's (``odom_dataset.py:56-68``).  ``--synthetic N`` trains on N generated snippets (no
validation split: the train loss selects the best model, as the reference does without one).  One process per GPU;
``data.use_orbslam_odom`` and ``data.load_imgs`` are refused.
"""
import os
import sys
import time

import numpy as np
import torch
import yaml

_HERE = os.path.dirname(os.path.abspath(__file__))
if __package__ in (None, ''):                     # run as a script: make the package importable under its alias
    sys.path.insert(0, os.path.dirname(_HERE))
    import panoptic_forecasting_amd  # noqa: F401
    __package__ = 'panoptic_forecasting_amd'

from . import config as pfconfig   # noqa: E402
from . import odom_io              # noqa: E402
from .export_odom import check_data  # noqa: E402
from .registry import build_model  # noqa: E402
from .train_bg import learning_rate, seed_all  # noqa: E402

EXTRA_FLAGS = (
    ('--synthetic', dict(type=int, default=0, help='train on N generated snippets instead of {split}_3d_info.pkl')),
)


def synthetic_snippets(n, seed=0):
    """[n, 30, 5] float64: smooth speed / yaw-rate curves with noise in columns 0, 1 (the columns the forecaster reads)."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    t = np.arange(odom_io.SNIPPET_LEN)
    phase, amp = rng.uniform(0, 6.28, (n, 2, 1)), rng.uniform(0.5, 1.5, (n, 2, 1))
    speed = 6 + 4 * amp[:, 0] * np.sin(0.2 * t + phase[:, 0]) + rng.normal(0, 0.3, (n, len(t)))
    yaw = 0.08 * amp[:, 1] * np.sin(0.15 * t + phase[:, 1]) + rng.normal(0, 0.01, (n, len(t)))
    return np.concatenate([np.stack([speed, yaw], -1), rng.normal(0, 1, (n, len(t), 3))], -1)


def load_snippets(data_dir, split):
    import pandas as pd
    return np.stack(pd.read_pickle(os.path.join(data_dir, '%s_3d_info.pkl' % split))['odometry'])


def norm_params(snippets):
    """odom_dataset.py:56-68: mean / std (population, numpy's default) of the train split's [speed, yaw_rate] as float32."""
    odo = snippets.reshape(-1, snippets.shape[-1])[:, :2]
    return torch.from_numpy(odo.mean(0)).float(), torch.from_numpy(odo.std(0)).float()


class Windows:
    """Every training window of a split on the device: ``inputs`` [N, input_len, 2], ``labels`` [N, output_len, 2]."""

    def __init__(self, snippets, params, device):
        data = params['data']
        wins = [odom_io.odom_windows(s, data.get('input_len', 9), data.get('output_len', 9), test=False) for s in snippets]
        self.inputs = torch.from_numpy(np.concatenate([w[0] for w in wins])).to(device)
        self.labels = torch.from_numpy(np.concatenate([w[1] for w in wins])).to(device)

    def __len__(self):
        return self.inputs.shape[0]

    def _batch(self, idx):
        return {'odometry': self.inputs.index_select(0, idx)}, {'odometry': self.labels.index_select(0, idx)}

    def train_batches(self, batch_size, steps=None):
        """Random batches with drop_last: one randperm per pass; ``steps`` batches over as many passes as it takes
        (train.py:104-116), one pass otherwise."""
        per_pass = len(self) // batch_size
        if per_pass == 0:
            raise SystemExit('train_odom: %d windows are fewer than one batch of %d' % (len(self), batch_size))
        done = 0
        while True:
            perm = torch.randperm(len(self), device=self.inputs.device)
            for i in range(per_pass):
                yield self._batch(perm[i * batch_size:(i + 1) * batch_size])
                done += 1
                if steps is not None and done >= steps:
                    return
            if steps is None:
                return

    def val_batches(self, batch_size):
        order = torch.arange(len(self), device=self.inputs.device)
        for i in range(0, len(self), batch_size):
            yield self._batch(order[i:i + batch_size])


def build_optimizer(model, tr):
    """train.py:129-136 as written there: ``use_adam`` chooses between Adam and SGD after the ``use_adamw`` line, so
    ``use_adamw`` alone ends with SGD.  Kept: a config trains with what the reference ran."""
    lr, wd, mom = tr['lr'], tr.get('wd', 0.), tr.get('mom', 0.)
    model_params = [p for p in model.parameters() if p.requires_grad]
    if tr.get('use_adamw', False):
        opt = torch.optim.AdamW(model_params, lr=lr, weight_decay=wd)
    if tr.get('use_adam', False):
        opt = torch.optim.Adam(model_params, lr=lr, weight_decay=wd)
    else:
        opt = torch.optim.SGD(model_params, lr=lr, weight_decay=wd, momentum=mom)
    return opt


def main(argv=None):
    params = pfconfig.load_config(EXTRA_FLAGS, argv)
    if params.get('task', 'odom') != 'odom':
        raise SystemExit('train_odom.py trains task: odom (got %r)' % params.get('task'))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit('train_odom.py runs one process per GPU (multi-GPU odom training is not built)')
    if params.get('no_gpu'):
        raise SystemExit('train_odom.py needs a GPU (libpfhip.so has no CPU path)')
    params['task'] = 'odom'
    check_data(params)
    tr = params.setdefault('training', {})
    data = params.setdefault('data', {})
    wd_dir = params['working_dir']
    os.makedirs(wd_dir, exist_ok=True)
    if not params.get('continue_training'):                                  # misc.copy_config
        with open(os.path.join(wd_dir, 'config.yaml'), 'w') as f:
            yaml.safe_dump({k: v for k, v in params.items() if isinstance(v, (dict, list, str, int, float, bool, type(None)))}, f)
    seed_all(int(params.get('seed', 1)))

    device = torch.device('cuda')
    if params.get('synthetic'):
        train_snips, val_snips = synthetic_snippets(int(params['synthetic'])), None
    else:
        train_snips = load_snippets(data['data_dir'], 'train')
        val_snips = load_snippets(data['data_dir'], 'val') if 'val' in data.get('data_splits', ['train', 'val']) else None
    data['odom_norm_params'] = norm_params(train_snips)
    train = Windows(train_snips, params, device)
    val = Windows(val_snips, params, device) if val_snips is not None else None

    ckpt, best_path, train_path = (os.path.join(wd_dir, n) for n in ('model_checkpoint', 'best_model', 'training_checkpoint'))
    resume = bool(params.get('continue_training'))
    model = build_model(dict(params, load_best_model=False, load_model=None if resume else params.get('load_model')))
    opt = build_optimizer(model, tr)
    start_epoch, best_val, best_epoch, steps = 1, 10000000, -1, 0
    if resume:
        print('RESUMING TRAINING')
        model.load(ckpt)
        st = torch.load(train_path, map_location='cpu')
        start_epoch, best_val, best_epoch, steps = st['epoch'], st['best_val_result'], st['best_val_epoch'], st['step']
        opt.load_state_dict(st['optimizer'])
        print('STARTING EPOCH: ', start_epoch)
    batch_size = int(tr.get('batch_size', 1000))
    val_batch_size = int(tr.get('val_batch_size') or batch_size)
    num_epochs = int(tr.get('num_epochs', 100))
    val_interval = int(tr.get('val_interval', 1))
    accumulate = int(tr.get('accumulate_steps', 1))
    clip_grad, clip_grad_norm = tr.get('clip_grad'), tr.get('clip_grad_norm')
    spe = tr.get('steps_per_epoch')
    n_batches = int(spe) * accumulate if spe else len(train) // batch_size
    seed_all(start_epoch)
    for epoch in range(start_epoch, num_epochs + 1):
        t0 = time.time()
        for group in opt.param_groups:
            group['lr'] = learning_rate(tr, epoch)
        model.train()
        loss_sum, count = torch.zeros((), dtype=torch.float64, device=device), 0
        for batch_ind, (inputs, labels) in enumerate(train.train_batches(batch_size, int(spe) * accumulate if spe else None)):
            loss = model.loss(inputs, labels)['loss']
            count += loss.size(0)
            loss_sum += loss.detach().double().sum()
            (loss.mean() / accumulate).backward()
            if accumulate == -1 or (batch_ind + 1) % accumulate == 0:
                if clip_grad is not None:
                    torch.nn.utils.clip_grad_value_(model.parameters(), clip_grad)
                elif clip_grad_norm is not None:
                    torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad_norm)
                opt.step()
                steps += 1
                opt.zero_grad()
                if accumulate > 0 and accumulate > n_batches - batch_ind - 1:
                    break
        if (epoch + 1) % val_interval != 0:
            continue
        train_loss = loss_sum.item() / max(count, 1)
        epoch_loss = train_loss
        if val is not None:
            model.eval()
            opt.zero_grad()
            val_sum, val_count = torch.zeros((), dtype=torch.float64, device=device), 0
            for inputs, labels in val.val_batches(val_batch_size):
                with torch.no_grad():
                    val_sum += model.loss(inputs, labels)['loss'].double().sum()
                val_count += inputs['odometry'].shape[0]
            epoch_loss = val_sum.item() / max(val_count, 1)
        if epoch_loss < best_val:
            best_val, best_epoch = epoch_loss, epoch
            model.save(best_path)
        model.save(ckpt)
        tmp = train_path + '.tmp'
        torch.save({'epoch': epoch + 1, 'optimizer': opt.state_dict(), 'best_val_result': best_val, 'best_val_epoch': best_epoch,
                    'step': steps}, tmp)
        os.replace(tmp, train_path)
        print('EPOCH %d EVAL: train loss %.6f  %s loss %.6f  best %.6f @%d  (%.2f s, %d steps)'
              % (epoch, train_loss, 'val' if val is not None else 'train', epoch_loss, best_val, best_epoch, time.time() - t0, steps),
              flush=True)
        seed_all(epoch + 1)


if __name__ == '__main__':
    main()
