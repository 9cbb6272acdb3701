"""MDGAT.forward_ragged: what it refuses before it needs a device."""
import pytest
import torch

from mdgat_matcher_amd import MDGAT, ops, synth


def _net(dtype=torch.float64, **over):
    cfg = synth.default_config(L=2, k=[8, None, 8, None], sinkhorn_iterations=20, **over)
    net = MDGAT(cfg)
    net.load_state_dict(synth.make_state_dict(L=2, seed=1))
    return net.to(dtype).eval()


def _pairs(counts):
    return [synth.make_batch(1, n, m, first_pair=b) for b, (n, m) in enumerate(counts)]


def test_forward_ragged_runs_in_the_exact_mode_only():
    pairs = _pairs([(16, 16), (20, 12)])
    for net in (_net(torch.float32), _net(arithmetic='fp32'), _net().train(), _net(eval_loss=True)):
        with pytest.raises(NotImplementedError, match='exact mode only'):
            net.forward_ragged(pairs)


def test_forward_ragged_refuses_counts_its_kernels_do_not_hold():
    net = _net()
    with pytest.raises(ValueError, match='pair 1 has 20 x 7 keypoints: fewer than a dynamic layer keeps'):
        net.forward_ragged(_pairs([(16, 16), (20, 7), (9, 9)]))
    with pytest.raises(ValueError, match='pair 0 has 576 x 16 keypoints: ragged batches hold at most 575'):
        net.forward_ragged(_pairs([(576, 16), (16, 16)]))


def test_forward_ragged_has_no_cpu_fallback():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _net().forward_ragged(_pairs([(16, 16), (20, 12)]))


def test_forward_ragged_checks_a_packed_batch_before_the_library_reads_it():
    """The library reads keypoints [B][Np][3], saliency [B][Np] and FPFH [B][Np][33] through raw pointers: a packed batch of any other
    width, with tensors of different B / Np, or with count vectors of another length is refused first, as forward refuses a uniform one."""
    net = _net()
    good = ops.pack_ragged(_pairs([(16, 16), (20, 12), (9, 30)]))

    def bad(**over):
        return {**good, **over}

    wide = [{**p, 'descriptors0': torch.zeros(1, p['keypoints0'].shape[1], 32, dtype=torch.float64)} for p in _pairs([(16, 16), (20, 12)])]
    with pytest.raises(ValueError, match='33-D FPFH'):
        net.forward_ragged(wide)                                                     # another descriptor type: packed at its own width
    with pytest.raises(ValueError, match='keypoints \\[B, N, 3\\]'):
        net.forward_ragged(bad(keypoints1=good['keypoints1'][..., :2]))
    with pytest.raises(ValueError, match='scores0 has shape'):
        net.forward_ragged(bad(scores0=good['scores0'][:, :-1]))                     # Np comes from the keypoints
    with pytest.raises(ValueError, match='descriptors1 has shape'):
        net.forward_ragged(bad(descriptors1=good['descriptors1'][:2]))               # another B
    with pytest.raises(ValueError, match='one entry per pair'):
        net.forward_ragged(bad(counts1_host=good['counts1_host'][:2]))
    with pytest.raises(ValueError, match='keypoints0 has shape'):
        net.forward_ragged(bad(counts0_host=good['counts0_host'][:2], counts1_host=good['counts1_host'][:2], counts0=good['counts0'][:2],
                               counts1=good['counts1'][:2]))                         # B by the counts against the tensors' leading dimension
    with pytest.raises(ValueError, match='pair 1 has 21 x 12 keypoints in slots of 20 x 30'):
        net.forward_ragged(bad(counts0_host=torch.tensor([16, 21, 9], dtype=torch.int32)))
    with pytest.raises(ValueError, match='33-D FPFH'):
        net.evaluate_ragged(bad(descriptors0=good['descriptors0'][..., :32], gt_matches0=torch.zeros(3, 20), gt_matches1=torch.zeros(3, 30)))
