"""The spawned ranks of tests/test_interface_geometry.py: the screen with interface geometry on two gloo ranks sharing cuda:0 (scorer_harness.rank_worker)."""
from scorer_harness import rank_worker

GEOM = dict(clash_cutoff=3.0, contact_cutoff=5.0, bond_max=2.0)
# once as it is, once with cluster_cutoff = 0.0 (every pose its own cluster: the path that gathers the poses, pose_geom with them, BEFORE stage 2)
RUNS = dict(plain={}, zero=dict(cluster_cutoff=0.0))


def runs(device, outdir):
    return {f'geometry_{tag}': dict(GEOM, **extra) for tag, extra in RUNS.items()}


def geometry_screen_worker(rank, world, port, outdir):
    rank_worker(rank, world, port, outdir, runs)
