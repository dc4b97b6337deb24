"""One gloo rank of eval_instances.py for tests/test_eval_instances_cli.py (spawned with torch.multiprocessing)."""
import os
import sys


def worker(rank, world, port, argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch
    from panoptic_forecasting_amd import dist as pfdist
    from panoptic_forecasting_amd import eval_instances
    r, w, _ = pfdist.init_distributed_mode(backend='gloo')
    assert (r, w) == (rank, world) and pfdist.is_dist()
    eval_instances.run(eval_instances.parse_args(argv))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def spawn_two(argv):
    """Runs the driver on two gloo ranks of this machine."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(worker, args=(2, port, argv), nprocs=2, join=True)
