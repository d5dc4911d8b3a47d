"""The spawned ranks of tests/test_pose_clusters.py: the clustered screen on two gloo ranks sharing cuda:0 (models and complex: screen_workers)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

REDOCK_CUTOFF = 2.0


def clustered_screen_worker(rank, world, port, outdir):
    """screen_workers.SCREEN with pose clustering at the cutoff the parent test left in <outdir>/cutoff.txt, two poses per launch."""
    import torch
    import torch.distributed as dist
    import screen_workers
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from ab_opt_amd import screen
        dev = torch.device('cuda:0')
        dock, design = screen_workers.models(dev)
        cutoff = float(open(os.path.join(outdir, 'cutoff.txt')).read())
        res = screen.optimize_antibody(dock, design, screen_workers.complex_(dev), poses_per_launch=2, cluster_cutoff=cutoff, redock_cutoff=REDOCK_CUTOFF,
                                       **screen_workers.SCREEN)
        torch.save({k: v.cpu() for k, v in res.items()}, os.path.join(outdir, f'clustered_{rank}.pt'))
    finally:
        dist.destroy_process_group()
