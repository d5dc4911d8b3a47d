"""The spawned ranks of tests/test_pose_clusters.py: the clustered screen on two gloo ranks sharing cuda:0 (scorer_harness.rank_worker)."""
import os

from scorer_harness import rank_worker

REDOCK_CUTOFF = 2.0


def runs(device, outdir):
    """pose clustering at the cutoff the parent test left in <outdir>/cutoff.txt"""
    cutoff = float(open(os.path.join(outdir, 'cutoff.txt')).read())
    return dict(clustered=dict(cluster_cutoff=cutoff, redock_cutoff=REDOCK_CUTOFF))


def clustered_screen_worker(rank, world, port, outdir):
    rank_worker(rank, world, port, outdir, runs)
