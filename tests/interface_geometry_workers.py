"""The spawned ranks of tests/test_interface_geometry.py: the screen with interface geometry on two gloo ranks sharing cuda:0 (models and complex: screen_workers)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

GEOM = dict(clash_cutoff=3.0, contact_cutoff=5.0, bond_max=2.0)


def geometry_screen_worker(rank, world, port, outdir):
    """screen_workers.SCREEN with the three cutoffs, two poses per launch: once as it is, once with cluster_cutoff = 0.0 (every pose its own cluster: the path
    that gathers the poses, pose_geom with them, BEFORE stage 2)."""
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
        for tag, extra in (('plain', {}), ('zero', dict(cluster_cutoff=0.0))):
            res = screen.optimize_antibody(dock, design, screen_workers.complex_(dev), poses_per_launch=2, **screen_workers.SCREEN, **GEOM, **extra)
            torch.save({k: v.cpu() for k, v in res.items()}, os.path.join(outdir, f'geometry_{tag}_{rank}.pt'))
    finally:
        dist.destroy_process_group()
