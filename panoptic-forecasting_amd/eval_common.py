"""What the evaluation drivers eval_panoptic.py and eval_semantic.py share: the batched reader, the staging of a batch, the
cross-rank sum and the shell of ``run`` / ``main``.  Flags, pairing, per-file checks, what a batch does, results and table are theirs."""
import json
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import dist as pfdist

LABEL_NAMES = ('road', 'sidewalk', 'building', 'wall', 'fence', 'pole', 'traffic light', 'traffic sign', 'vegetation', 'terrain',
               'sky', 'person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')
N_CLS = 19


class EvalError(RuntimeError):
    pass


def on_device(arr, device):
    """Host array -> the same bytes on the device (pinned staging, asynchronous copy)."""
    t = torch.from_numpy(arr)
    if torch.cuda.is_available():
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def for_each_batch(items, read, a, on_batch):
    """``read(item)`` -> a tuple of arrays, on a thread pool of a.num_workers, in the order of ``items``.  Consecutive results are
    collected while the first arrays have one shape, the last ones one dtype and there are fewer than a.batch_size of them;
    ``on_batch`` gets each collection stacked: one [B, ...] array per position of the tuple."""
    with ThreadPoolExecutor(max_workers=max(1, a.num_workers)) as pool:
        batch = []
        def flush():
            if batch:
                on_batch(*[np.stack(column) for column in zip(*batch)])
            del batch[:]
        for x in pool.map(read, items):
            if batch and (x[0].shape != batch[0][0].shape or x[-1].dtype != batch[0][-1].dtype or len(batch) >= a.batch_size):
                flush()
            batch.append(x)
        flush()


def gather_total(acc):
    """This rank's accumulators -> their sum over the ranks, on the host.  The exchange runs where the process group's
    backend has tensors: RCCL ("nccl") carries device tensors only, gloo host tensors (dist.gather_accumulators moves those itself)."""
    if pfdist.is_dist() and str(torch.distributed.get_backend()) != 'gloo':
        acc = acc.to(torch.device('cuda', torch.cuda.current_device()))
    return pfdist.gather_accumulators(acc).sum(0).cpu()


def rank_world():
    return (torch.distributed.get_rank(), torch.distributed.get_world_size()) if pfdist.is_dist() else (0, 1)


def require_matcher(a):
    if a.matcher == 'device' and not torch.cuda.is_available():
        raise EvalError('--matcher device needs a GPU (there is no fallback: pass --matcher host for the host path)')


def write_results(res, a, print_table):
    """Rank 0 writes a.results_file and prints the table."""
    if rank_world()[0] == 0:
        with open(a.results_file, 'w', encoding='utf-8') as f:
            json.dump(res, f, indent=4)
        print_table(res)
    return res


def main(name, parse_args, run, argv=None):
    a = parse_args(argv)
    pfdist.init_distributed_mode()
    try:
        run(a)
    except EvalError as e:                              # no barrier: the other ranks may not have failed
        sys.exit('%s: %s' % (name, e))
    if pfdist.is_dist():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
