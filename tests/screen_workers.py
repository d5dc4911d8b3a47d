"""Models, the complex and the spawned ranks of tests/test_screen.py (both ranks share cuda:0, the process group is gloo, so the gather goes
through host memory -- on a multi-GPU node the same code runs on backend 'nccl')."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

_DESIGN = {}

# the screen the GPU tests run: P poses, S designs, k screened, D re-docks of the LAYOUT_128 complex (CDR 31-42), redesign limited to a contig
SCREEN = dict(num_poses=5, designs_per_pose=3, redocks_per_design=3, screened_per_pose=2, contig='33-39', seed=17, screen_by='ppl')


def models(device):
    """(dock model, design model): AbDock flavour, 10 steps, hash-filled; the design model at backbone+CB (configs/test/seq_design.yml).
    The design model is built here and cached per device (synth.build_model only builds the full-atom resolution)."""
    from conftest import AttrDict, build_model
    from ab_opt_amd import get_model
    from ab_opt_amd.utils import synth
    key = str(device)
    if key not in _DESIGN:
        _DESIGN[key] = synth.fill_module_(get_model(AttrDict(synth.cfg_abdock(10, resolution='backbone+CB'))).eval(), seed=4).to(device)
    return build_model(10, 3, device=device), _DESIGN[key]


def complex_(device):
    from ab_opt_amd.utils import synth
    return {k: v.to(device) for k, v in synth.make_batch(1, synth.LAYOUT_128, seed=21).items()}


def screen_worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from ab_opt_amd import screen
        dev = torch.device('cuda:0')
        dock, design = models(dev)
        res = screen.optimize_antibody(dock, design, complex_(dev), poses_per_launch=2, **SCREEN)
        torch.save({k: v.cpu() for k, v in res.items()}, os.path.join(outdir, f'screen_{rank}.pt'))
    finally:
        dist.destroy_process_group()
