"""The unchanged-caller path: `from models.mdgat import MDGAT` (test.py:12, test_registration_metric.py:12) resolved by the
import-path shim under integration/, then the call sequence of test.py:134-214 - checkpoint dict saved by train.py:288-294
loaded with torch.load, DataParallel wrapper and its `module.` keys, net.double().eval() before every forward, the
collated loader dict (load_data.py:299-321: tensors plus the non-tensor `sequence`, the index tensor `idx0`, gt matches,
T_gt, rep) moved with .cuda() the way test.py:194-199 does, `pred = {**pred, **data}` and the per-pair numpy reads."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def models_mdgat():
    """`import models.mdgat` the way the reference's scripts do, with <repo>/integration ahead on sys.path."""
    shim = os.path.join(ROOT, 'integration')
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'models' or k.startswith('models.')}
    sys.path.insert(0, shim)
    try:
        yield importlib.import_module('models.mdgat')
    finally:
        sys.path.remove(shim)
        for k in [k for k in sys.modules if k == 'models' or k.startswith('models.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def _loader_batch(B, n, m, first_pair):
    """What DataLoader(SparseDataset) yields (load_data.py:299-321 after default collation), synthetic content."""
    from mdgat_matcher_amd import synth
    d = synth.make_batch(B, n, m, first_pair=first_pair)
    d['sequence'] = ['00'] * B                                   # strings: collated into a list
    d['idx0'] = torch.arange(first_pair, first_pair + B)         # ints: collated into an int64 tensor
    d['T_gt'] = torch.eye(4, dtype=torch.float64)[None].repeat(B, 1, 1)
    d['rep'] = torch.full((B,), n // 2, dtype=torch.int64)
    return d


def test_unchanged_caller_sequence_of_test_py(models_mdgat, golden_dir, tmp_path):
    from torch.autograd import Variable
    from mdgat_matcher_amd import synth
    MDGAT = models_mdgat.MDGAT                                   # test.py:12
    g = np.load(os.path.join(golden_dir, 'fwd_n64_L4_S20.npz'))
    B, n, m, L, S, seed, first_pair = [int(x) for x in g['meta']]
    k = [None if x < 0 else int(x) for x in g['k']]
    # the checkpoint train.py:288-294 writes: DataParallel state dict + bookkeeping
    ckpt = {'net': {'module.' + kk: v for kk, v in synth.make_state_dict(L=L, seed=seed).items()}, 'optimizer': {}, 'epoch': 3,
            'lr_schedule': 1e-4, 'loss': 0.5}
    path = os.path.join(tmp_path, 'best_model.pth')
    torch.save(ckpt, path)
    checkpoint = torch.load(path, map_location={'cuda:2': 'cuda:0'})          # test.py:135
    config = {'net': {'sinkhorn_iterations': S, 'match_threshold': 0.2, 'lr': 1e-4, 'loss_method': 'triplet_loss', 'k': k,
                      'descriptor': 'FPFH', 'mutual_check': False, 'triplet_loss_gamma': 0.5, 'train_step': 3, 'L': L}}
    net = MDGAT(config.get('net', {}))                                         # test.py:156
    torch.optim.Adam(net.parameters(), lr=config.get('net', {}).get('lr'))     # test.py:157 (parameters must be real leaves)
    net = torch.nn.DataParallel(net)                                           # test.py:158
    net.load_state_dict(checkpoint['net'])                                     # test.py:159
    device = torch.device('cuda:{}'.format(0))
    net.to(device)                                                             # test.py:172
    with torch.no_grad():
        for it in range(2):
            pred = _loader_batch(B, n, m, first_pair)
            net.double().eval()                                                # test.py:193
            for kk in pred:                                                    # test.py:194-199
                if kk != 'idx0' and kk != 'idx1' and kk != 'sequence':
                    if type(pred[kk]) == torch.Tensor:
                        pred[kk] = Variable(pred[kk].cuda().detach())
                    else:
                        pred[kk] = Variable(torch.stack(pred[kk]).cuda().detach())
            data = net(pred)                                                   # test.py:201
            pred = {**pred, **data}
            for b in range(len(pred['idx0'])):                                 # test.py:204-217
                kpts0, kpts1 = pred['keypoints0'][b].cpu().numpy(), pred['keypoints1'][b].cpu().numpy()
                matches, matches1, conf = (pred['matches0'][b].cpu().detach().numpy(), pred['matches1'][b].cpu().detach().numpy(),
                                           pred['matching_scores0'][b].cpu().detach().numpy())
                valid = matches > -1
                mkpts0, mkpts1, mconf = kpts0[valid], kpts1[matches[valid]], conf[valid]
                assert mkpts0.shape == mkpts1.shape and mconf.shape[0] == valid.sum()
                np.testing.assert_array_equal(matches, g['default_matches0'][b])
                np.testing.assert_array_equal(matches1, g['default_matches1'][b])
                assert np.abs(conf - g['default_mscores0'][b]).max() < 1e-4
                assert conf.dtype == np.float64
            assert float(pred['loss'].mean()) == 0.0                           # (train.py:245 takes the mean; inference: zero)


def test_unchanged_caller_meets_the_literal_bar(models_mdgat, golden_dir):
    """The unchanged-caller sequence - NO extra config key - at BASELINE configs[0]'s shape and the weights / pairs of the
    reference-held fixture cfg_n256_L4_S20 (8 pairs of 256 keypoints, L = 4, dynamic self layers).  `net.double()` (test.py:193) is
    the arithmetic request: the float64 module runs the reference-exact mode, so every pair is within the LITERAL 1e-4 on Z, the
    matches are identical and not one top-k row is selected differently from the fp64 oracle on the same trajectory.
    The checkpoint goes through DataParallel's load_state_dict into the FLOAT32 module and `.double()` afterwards exactly like
    test.py:156-193 - which rounds the weights to fp32 in the reference as well - so the expected values are the oracle's (pinned
    to the reference by tests/test_oracle_golden.py) on those rounded weights; the distance to the fixture itself (made from the
    unrounded weights) is printed."""
    from torch.autograd import Variable
    from mdgat_matcher_amd import synth
    from oracle import mdgat_oracle as O
    from parity_util import hip_forward_with_selection
    MDGAT = models_mdgat.MDGAT
    g = np.load(os.path.join(golden_dir, 'cfg_n256_L4_S20.npz'))
    B, n, m, L, S, seed, first_pair = [int(x) for x in g['meta']]
    k = [None if x < 0 else int(x) for x in g['k']]
    cfg = {'sinkhorn_iterations': S, 'match_threshold': 0.2, 'lr': 1e-4, 'loss_method': 'triplet_loss', 'k': k,
           'descriptor': 'FPFH', 'mutual_check': False, 'triplet_loss_gamma': 0.5, 'train_step': 3, 'L': L}      # test.py:137-151
    assert 'arithmetic' not in cfg and 'MDGAT_ARITHMETIC' not in os.environ
    sd = synth.make_state_dict(L=L, seed=seed, bin_score=float(g['bin_score']))
    net = torch.nn.DataParallel(MDGAT(cfg))                                                 # test.py:156-158 (a float32 module)
    net.load_state_dict({'module.' + kk: v for kk, v in sd.items()})                       # test.py:159: rounds to float32
    net.to(torch.device('cuda:0'))
    sd_ref = {kk: (v.float().double() if v.is_floating_point() else v) for kk, v in sd.items()}     # what .double() makes of that module
    with torch.no_grad():
        pred = _loader_batch(B, n, m, first_pair)
        cpu = {kk: v for kk, v in pred.items() if torch.is_tensor(v)}
        net.double().eval()                                                                 # test.py:193
        assert net.module.exact()                                                           # float64 module -> reference-exact mode
        for kk in pred:
            if kk not in ('idx0', 'idx1', 'sequence') and type(pred[kk]) == torch.Tensor:
                pred[kk] = Variable(pred[kk].cuda().detach())
        data = net(pred)                                                                    # test.py:201
        assert data['matches0'].dtype == torch.int64 and data['matching_scores0'].dtype == torch.float64
        # Z and the selections of the same module (the dict API does not return Z), then the oracle on the same trajectory
        (m0, m1, s0, s1, Z), forced = hip_forward_with_selection(net.module, pred)
        net.module.check('cuda:0')
        assert torch.equal(m0, data['matches0']) and torch.equal(m1, data['matches1'])
        ref_cfg = synth.default_config(L=L, k=k, sinkhorn_iterations=S)
        cap, capf = {}, {}
        ref = O.mdgat_forward(sd_ref, ref_cfg, cpu, cap)                                    # unforced: the reference's own run
        O.mdgat_forward(sd_ref, ref_cfg, cpu, capf, forced_topk=forced)
        rows = sum(r['rows'] for reps in capf.get('topk_report', {}).values() for r in reps)
        bad = sum(r['bad_count'] for reps in capf.get('topk_report', {}).values() for r in reps)
        err = (Z.cpu().double() - cap['Z']).abs().reshape(B, -1).max(1).values.numpy()
        Zc = Z.cpu().double().numpy()
        mine = np.concatenate([Zc[:, ::8, ::8].reshape(B, -1), Zc[:, -1, :], Zc[:, :, -1]], axis=1)
        fix = np.abs(mine - np.concatenate([g['Z_sub'].reshape(B, -1), g['Z_lastrow'], g['Z_lastcol']], axis=1)).max()
        print(f'[dropin] unchanged caller, float64 module: per-pair max|dZ| {np.array2string(err, precision=2)}; top-k rows differing {rows}; '
              f'against the fixture made from the unrounded weights: {fix:.2e}')
        assert (err < 1e-4).all(), err
        assert rows == 0 and bad == 0
        assert torch.equal(data['matches0'].cpu(), ref['matches0']) and torch.equal(data['matches1'].cpu(), ref['matches1'])
        assert (data['matching_scores0'].cpu() - ref['matching_scores0']).abs().max() < 1e-4
        assert (data['matching_scores1'].cpu() - ref['matching_scores1']).abs().max() < 1e-4
        # the same caller with a float32 module (no .double()) gets the throughput path: same matches here, Z to fp32-class error
        net.float()
        assert not net.module.exact()
        out32 = net({kk: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for kk, v in pred.items()})
        assert out32['matching_scores0'].dtype == torch.float32
        assert (out32['matches0'].cpu() != ref['matches0']).float().mean() < 0.01


def test_all_dustbin_batch_returns_integer_zero_scores(models_mdgat, golden_dir):
    """mdgat.py:465-467: when no frame-0 keypoint of the batch is matched the reference returns torch.zeros_like(indices) -
    INT64 zeros - for both score vectors (tests/golden/edge_cases.npz holds the reference's output)."""
    from mdgat_matcher_amd import synth
    g = np.load(os.path.join(golden_dir, 'edge_cases.npz'))
    assert bool(g['alldust_mscores_is_int'])
    net = models_mdgat.MDGAT(synth.default_config(L=1, k=[], sinkhorn_iterations=10))
    net.load_state_dict(synth.make_state_dict(L=1, seed=3, bin_score=50.0))
    net = net.double().eval().to('cuda:0')
    with torch.no_grad():
        out = net(synth.make_batch(1, 32, 32, device='cuda:0'))
    np.testing.assert_array_equal(out['matches0'].cpu().numpy(), g['alldust_matches0'])
    np.testing.assert_array_equal(out['matches1'].cpu().numpy(), g['alldust_matches1'])
    for key in ('matching_scores0', 'matching_scores1'):
        assert out[key].dtype == torch.int64 and not out[key].any()
    # with a match anywhere in the batch the scores are floating point again (module dtype)
    net.load_state_dict(synth.make_state_dict(L=1, seed=3, bin_score=1.0))
    with torch.no_grad():
        out = net.double().eval()(synth.make_batch(1, 32, 32, device='cuda:0'))
    assert out['matching_scores0'].dtype == torch.float64 and (out['matches0'] >= 0).any()


def test_free_functions_of_models_mdgat(models_mdgat, golden_dir):
    """attention / dynamic_attention / log_optimal_transport / knn / get_graph_feature under their reference names and
    signatures (mdgat.py:8-32, 190-210, 288-308), against the reference's outputs in tests/golden/op_vectors.npz."""
    g = np.load(os.path.join(golden_dir, 'op_vectors.npz'))
    dev = 'cuda:0'
    q, k, v = (torch.from_numpy(g[x]).to(dev) for x in ('att_q', 'att_k', 'att_v'))
    msg, prob = models_mdgat.attention(q, k, v)
    assert prob is None and msg.dtype == q.dtype and tuple(msg.shape) == tuple(g['att_full'].shape)
    assert np.abs(msg.cpu().numpy() - g['att_full']).max() < 1e-5
    for kk in (1, 8, 56):                                          # 56 = all keys, more than the 40 queries
        dyn, _ = models_mdgat.dynamic_attention(q, k, v, kk)
        assert np.abs(dyn.cpu().numpy() - g[f'att_dyn{kk}']).max() < 1e-5, kk
    with pytest.raises(RuntimeError):
        models_mdgat.dynamic_attention(q, k, v, 57)                # torch.topk raises there
    s = torch.from_numpy(g['sk_64x64_scores']).to(dev)
    iters, alpha = g['sk_64x64_meta']
    Z = models_mdgat.log_optimal_transport(s, torch.tensor(alpha, dtype=torch.float64), int(iters))
    assert Z.dtype == s.dtype and np.abs(Z.cpu().numpy() - g['sk_64x64_Z']).max() < 1e-5
    for Cc in (3, 128):
        x, src = torch.from_numpy(g[f'knn{Cc}_x']).to(dev), torch.from_numpy(g[f'knn{Cc}_s']).to(dev)
        np.testing.assert_array_equal(models_mdgat.knn(x, src, 9).cpu().numpy(), g[f'knn{Cc}_idx'])
        np.testing.assert_array_equal(models_mdgat.get_graph_feature(x, src, 9).cpu().numpy(), g[f'knn{Cc}_adj'])
    mlp = models_mdgat.MLP([4, 32, 64])
    assert [type(mm).__name__ for mm in mlp] == ['Conv1d', 'BatchNorm1d', 'ReLU', 'Conv1d']


def test_free_functions_of_models_mdgat_in_float32(models_mdgat, golden_dir):
    """The float32 route of the drop-in free functions (integration/models/mdgat.py): float32 q / k / v run the fp32-class kernels
    through a CROSS layer of the library's layout - the queries are frame 0, zero rows pad it up to k (``_to_lib(min_rows=k)``), the
    keys are frame 1.  Against the reference's outputs in tests/golden/op_vectors.npz cast to float32 (40 queries, 56 keys:
    attention_kernel<true, 4>; k = 56 = every key: frame 0 padded to 56, the dispatcher's full-attention shortcut), then against
    the fp64 oracle at lopsided shapes: k larger than the number of queries (zero-padded query rows; 900 keys:
    attention_topk_wide_kernel<4>, 2048 keys: <8>), k equal to the number of keys (that side keeps every key), rows whose k-th and
    (k+1)-th fp64 logits lie within 5e-6 excepted as in tests/test_gpu_ops.py.  Outputs are float32 in the reference's [B, dh, H, N]."""
    from oracle import mdgat_oracle as O
    g = np.load(os.path.join(golden_dir, 'op_vectors.npz'))
    dev = 'cuda:0'
    q, k, v = (torch.from_numpy(g[x]).float().to(dev) for x in ('att_q', 'att_k', 'att_v'))
    msg, prob = models_mdgat.attention(q, k, v)
    assert prob is None and msg.dtype == torch.float32 and tuple(msg.shape) == tuple(g['att_full'].shape)
    assert np.abs(msg.cpu().double().numpy() - g['att_full']).max() < 1e-5
    for kk in (1, 8, 56):
        dyn, _ = models_mdgat.dynamic_attention(q, k, v, kk)
        assert dyn.dtype == torch.float32 and tuple(dyn.shape) == tuple(g['att_full'].shape)
        assert np.abs(dyn.cpu().double().numpy() - g[f'att_dyn{kk}']).max() < 1e-5, kk
    with pytest.raises(RuntimeError):
        models_mdgat.dynamic_attention(q, k, v, 57)
    s = torch.from_numpy(g['sk_64x64_scores']).float().to(dev)
    iters, alpha = g['sk_64x64_meta']
    with torch.no_grad():
        Z = models_mdgat.log_optimal_transport(s, torch.tensor(alpha, dtype=torch.float32), int(iters))
    assert Z.dtype == torch.float32 and tuple(Z.shape) == tuple(g['sk_64x64_Z'].shape)
    assert np.abs(Z.cpu().double().numpy() - g['sk_64x64_Z']).max() < 1e-5

    rs = np.random.RandomState(17)
    for B, N, M, kk in ((2, 100, 900, 128), (2, 300, 200, 200), (1, 130, 2048, 64), (2, 50, 600, 600), (2, 700, 300, 8)):
        qd, kd, vd = (torch.from_numpy(rs.standard_normal((B, 32, 4, n)) * 1.3).float() for n in (N, M, M))
        ref_full, _ = O.attention(qd.double(), kd.double(), vd.double())
        full, _ = models_mdgat.attention(qd.to(dev), kd.to(dev), vd.to(dev))
        assert full.dtype == torch.float32 and tuple(full.shape) == (B, 32, 4, N)
        assert (full.cpu().double() - ref_full).abs().max() < 1e-5
        dyn, _ = models_mdgat.dynamic_attention(qd.to(dev), kd.to(dev), vd.to(dev), kk)
        assert dyn.dtype == torch.float32 and tuple(dyn.shape) == (B, 32, 4, N)
        ref, _ = O.dynamic_attention(qd.double(), kd.double(), vd.double(), kk)
        logits = torch.einsum('bdhn,bdhm->bhnm', qd.double(), kd.double()) / 32 ** 0.5
        if kk < M:
            top = logits.topk(kk + 1, dim=3).values
            near_tie = (top[..., kk - 1] - top[..., kk]) < 5e-6                  # [B, H, N]
        else:
            near_tie = torch.zeros(logits.shape[:3], dtype=torch.bool)
        assert near_tie.double().mean() < 2e-3
        err = (dyn.cpu().double() - ref).abs().amax(1)                            # [B, H, N]
        print(f'[dropin] float32 dynamic_attention {N} queries, {M} keys, k={kk}: near-tie rows {int(near_tie.sum())} of '
              f'{near_tie.numel()}, worst error {float(err[~near_tie].max()):.2e}')
        assert err[~near_tie].max() < 1e-5, (N, M, kk)
    s = torch.from_numpy(rs.standard_normal((2, 300, 900)) * 4.0)
    with torch.no_grad():
        Z = models_mdgat.log_optimal_transport(s.float().to(dev), 0.7, 30)
    assert Z.dtype == torch.float32 and tuple(Z.shape) == (2, 301, 901)
    assert (Z.cpu().double() - O.log_optimal_transport(s.float().double(), 0.7, 30)).abs().max() < 1e-4
