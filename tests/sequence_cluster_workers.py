"""The spawned ranks of tests/test_sequence_clusters.py: the sequence-clustered screens on two gloo ranks sharing cuda:0 (scorer_harness.rank_worker), and
the options both sides of that comparison run with."""
from scorer_harness import rank_worker

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


def runs(device, outdir):
    return options(device)


def sequence_screen_worker(rank, world, port, outdir):
    rank_worker(rank, world, port, outdir, runs)
