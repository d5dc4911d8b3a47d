"""hip._candidate_args, the shape contract hip.interface_geometry_grouped and hip.sasa_grouped share: one row per refusal, with the text it raises.  No device:
the tensors live on the CPU."""
import pytest
import torch

from ab_opt_amd import hip

POS, MASK, GROUP = torch.zeros(4, 6, 4, 3), torch.ones(4, 6, 4, dtype=torch.bool), torch.ones(2, 6, dtype=torch.int32)

REFUSALS = [
    (dict(mask=MASK[0]), 'f: expected pos (G*S, L, A, 3), mask (G*S or G, L, A) and group (G, L), got (4, 6, 4, 3), (6, 4) and (2, 6)'),
    (dict(group=GROUP[0]), 'f: expected pos (G*S, L, A, 3), mask (G*S or G, L, A) and group (G, L), got (4, 6, 4, 3), (4, 6, 4) and (6,)'),
    (dict(pos=POS[:3], mask=MASK[:3]), 'f: (3, 6, 4, 3) candidates are not whole groups of the 2 rows of group (2, 6)'),
    (dict(group=GROUP[:, :5]), 'f: (4, 6, 4, 3) candidates are not whole groups of the 2 rows of group (2, 5)'),
    (dict(pos=POS[..., :2]), 'f: (4, 6, 4, 2) candidates are not whole groups of the 2 rows of group (2, 6)'),
    (dict(pos=torch.zeros(4, 6, 16, 3), mask=torch.ones(4, 6, 16, dtype=torch.bool)), 'f: A=16 atoms per residue, expected 1 .. 15'),
    (dict(mask=MASK[:3]), 'f: mask (3, 6, 4) is neither per candidate nor per group'),
]


@pytest.mark.parametrize('kw,text', REFUSALS)
def test_refusal_texts(kw, text):
    kw = dict(dict(pos=POS, mask=MASK, group=GROUP), **kw)
    with pytest.raises(ValueError) as e:
        hip._candidate_args('f', kw['pos'], kw['mask'], kw['group'])
    assert str(e.value) == text


def test_accepted_shapes():
    assert hip._candidate_args('f', POS, MASK, GROUP) == (2, 2, 6, 4, False)
    assert hip._candidate_args('f', POS, MASK[:2], GROUP) == (2, 2, 6, 4, True)             # one mask per group
    assert hip._candidate_args('f', POS[:2], MASK[:2], GROUP) == (2, 1, 6, 4, True)         # S = 1: per group and per candidate are the same
    assert hip._candidate_args('f', POS[:0], MASK[:0], GROUP[:0]) == (0, 0, 6, 4, False)    # no groups
