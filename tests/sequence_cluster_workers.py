"""The spawned ranks of tests/test_sequence_clusters.py: the sequence-clustered screens on two gloo ranks sharing cuda:0 (models and complex: screen_workers),
and the options both sides of that comparison run with."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

# screen_workers.SCREEN redesigns the contig 33-39: seven positions.  One allowed type at four of them and two at the other three: at most 8 distinct designs
ALLOWED_AT = {33: 'A', 34: 'G', 35: 'S', 36: 'T', 37: 'AV', 38: 'LK', 39: 'DE'}
SEQ_MISMATCH = 4


def allowed(device):
    from ab_opt_amd.model import aa_allowed_mask
    return aa_allowed_mask(128, at=ALLOWED_AT).to(device)


def options(device):
    """{name: keyword arguments on top of screen_workers.SCREEN} of the two screens the launch-size / rank test compares."""
    return dict(diverse=dict(seq_mismatch=SEQ_MISMATCH, screen_by='diverse'),
                shared=dict(seq_mismatch=0, share_redocks=True, allowed_aa=allowed(device)))


def sequence_screen_worker(rank, world, port, outdir):
    """Both screens of `options`, two poses (units) per launch."""
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
        for name, extra in options(dev).items():
            res = screen.optimize_antibody(dock, design, screen_workers.complex_(dev), poses_per_launch=2, **dict(screen_workers.SCREEN, **extra))
            torch.save({k: v.cpu() for k, v in res.items()}, os.path.join(outdir, f'{name}_{rank}.pt'))
    finally:
        dist.destroy_process_group()
