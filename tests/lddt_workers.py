"""The spawned ranks of tests/test_lddt.py: the screen with lDDT on two gloo ranks sharing cuda:0 (models and complex: screen_workers), and the options both
sides of that comparison run with."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

LDDT = dict(lddt_cutoff=15.0)


def _shared(device):
    import sequence_cluster_workers
    return dict(seq_mismatch=0, share_redocks=True, allowed_aa=sequence_cluster_workers.allowed(device))


# {tag: device -> keyword arguments on top of screen_workers.SCREEN and LDDT}: the plain screen, and shared re-docks (the versus-design fields are gathered per
# owner, redock_consistency per unit)
RUNS = dict(plain=lambda device: {}, shared=_shared)


def lddt_screen_worker(rank, world, port, outdir):
    """screen_workers.SCREEN with lddt_cutoff, two poses (units) per launch, once per entry of RUNS."""
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
        for tag, extra in RUNS.items():
            res = screen.optimize_antibody(dock, design, screen_workers.complex_(dev), poses_per_launch=2, **screen_workers.SCREEN, **LDDT, **extra(dev))
            torch.save({k: v.cpu() for k, v in res.items()}, os.path.join(outdir, f'lddt_{tag}_{rank}.pt'))
    finally:
        dist.destroy_process_group()
