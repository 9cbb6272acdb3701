"""ops.pack_ragged: per-pair dicts of different keypoint counts (what the reference's batch_size=1 loader yields, test.py:132) into one
padded batch with its count vectors.  Pure torch: no GPU."""
import numpy as np
import pytest
import torch

from mdgat_matcher_amd import ops, synth

COUNTS = [(40, 33), (17, 64), (64, 17), (8, 8)]


def _pairs(leading_axis, with_gt=True):
    pairs = []
    for b, (n, m) in enumerate(COUNTS):
        d = synth.make_batch(1, n, m, first_pair=b)
        rs = np.random.RandomState(b)
        d['gt_matches0'] = torch.from_numpy(rs.randint(-1, m + 1, size=(1, n)))
        d['gt_matches1'] = torch.from_numpy(rs.randint(-1, n + 1, size=(1, m)))
        d['T_gt'] = torch.from_numpy(rs.standard_normal((1, 4, 4)))
        if not with_gt:
            for k in ('gt_matches0', 'gt_matches1', 'T_gt'):
                del d[k]
        pairs.append(d if leading_axis else {k: v[0] for k, v in d.items()})
    return pairs


@pytest.mark.parametrize('leading_axis', [True, False])
def test_pack_ragged_pads_counts_and_ground_truth(leading_axis):
    pairs = _pairs(leading_axis)
    p = ops.pack_ragged(pairs)
    B, Np, Mp = len(COUNTS), max(n for n, _ in COUNTS), max(m for _, m in COUNTS)
    assert p['counts0_host'].tolist() == [n for n, _ in COUNTS] and p['counts1_host'].tolist() == [m for _, m in COUNTS]
    for f in '01':
        assert p['counts' + f].dtype == torch.int32 and p['counts' + f + '_host'].dtype == torch.int32
        assert p['counts' + f + '_host'].device.type == 'cpu' and torch.equal(p['counts' + f].cpu(), p['counts' + f + '_host'])
    P = {'0': Np, '1': Mp}
    for key, tail in (('keypoints', (3,)), ('scores', ()), ('descriptors', (33,))):
        for f in '01':
            t = p[key + f]
            assert t.dtype == torch.float64 and tuple(t.shape) == (B, P[f]) + tail
            for b, d in enumerate(pairs):
                src = d[key + f][0] if leading_axis else d[key + f]
                c = COUNTS[b][int(f)]
                assert torch.equal(t[b, :c], src.double()) and not t[b, c:].any()
    for f in '01':
        gt = p['gt_matches' + f]
        assert gt.dtype == torch.int64 and tuple(gt.shape) == (B, P[f])
        for b, d in enumerate(pairs):
            src = d['gt_matches' + f][0] if leading_axis else d['gt_matches' + f]
            c = COUNTS[b][int(f)]
            assert torch.equal(gt[b, :c], src.long()) and (gt[b, c:] == -1).all()
    assert tuple(p['T_gt'].shape) == (B, 4, 4) and p['T_gt'].dtype == torch.float64
    for b, d in enumerate(pairs):
        assert torch.equal(p['T_gt'][b], (d['T_gt'][0] if leading_axis else d['T_gt']).double())


def test_pack_ragged_without_ground_truth_and_mixed_ranks():
    pairs = _pairs(True, with_gt=False)
    pairs[1] = {k: v[0] for k, v in pairs[1].items()}          # one pair without the leading axis among pairs with it
    p = ops.pack_ragged(pairs)
    assert 'gt_matches0' not in p and 'gt_matches1' not in p and 'T_gt' not in p
    assert p['counts0_host'].tolist() == [n for n, _ in COUNTS]
    assert torch.equal(p['keypoints0'][1, :17], pairs[1]['keypoints0'].double())


def test_pack_ragged_refuses_what_it_cannot_pack():
    with pytest.raises(ValueError, match='no pairs'):
        ops.pack_ragged([])
    pairs = _pairs(True)
    pairs[2]['scores0'] = pairs[2]['scores0'][:, :-1]           # one saliency short of its keypoints
    with pytest.raises(ValueError, match='pair 2'):
        ops.pack_ragged(pairs)
    pairs = _pairs(True)
    pairs[0]['keypoints1'] = torch.cat([pairs[0]['keypoints1']] * 2)      # a real batch axis: not a per-pair record
    with pytest.raises(ValueError, match='keypoints1'):
        ops.pack_ragged(pairs)
