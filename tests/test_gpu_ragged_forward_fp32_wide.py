"""MDGAT.forward_ragged / evaluate_ragged / match_frames_ragged on a float32 module with config['ragged_slots_fp32'] = 'wide': the fp32-class
ragged forward on chunks with frames beyond 512 keypoints (mdgat_forward_ragged under mdgat_set_ragged_fp32_slots(1)), with the default
and the split Sinkhorn.  The structure and the yardsticks are tests/test_gpu_ragged_forward_fp32.py's: the fp64 oracle on every pair
ALONE, split by tests/ragged_decided.py into DECIDED pairs (matches identical, Z and scores within Z_TOL) and the others (PLAIN_MAX,
PLAIN_FRAC, a differing match a near tie by the path's own Z).  L = 1, 20 Sinkhorn iterations.

    W4   slots 544 x 520    k = [64, None]   (544, 130), (70, 520), (300, 257), (513, 513)    wide<4>, the windowed kernel, NC = 16
    W8   slots 1056 x 1040  k = [64, None]   (1056, 100), (90, 1040), (700, 1025)             wide<8>, NC = 32
    WF   slots 544 x 520    k = []           as W4                                            no dynamic layer: the strict bar

A pair of this size with a dynamic layer is practically never decided - among its thousands of rows some top-k gap falls below 4e-5 - so
W4 and W8 are held to the PLAIN bounds and the strict bar is carried by WF, whose ``first_pair`` seeds (FIRST_PAIR) were checked on the CPU:
the oracle alone decides the pairs written down in DECIDED.  The oracle's figures (smallest top-k gap, smallest arg-max margin on Z):

    W4   gaps 3.1e-6, 1.9e-5, 1.6e-5, 4.4e-7; margins 7.0e-5, 6.2e-3, 5.1e-3, 1.7e-3: none decided
    W8   gaps 6.0e-7, 2.2e-6, 5.9e-6; margins 2.2e-4, 5.1e-3, 3.5e-4: none decided
    WF   no dynamic layer; margins 6.6e-4, 6.1e-3, 3.6e-4, 1.8e-3: all four decided (first_pair = the pair's index, as in W4)"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdgat_matcher_amd import MDGAT, ops, synth  # noqa: E402
import ragged_decided as RD  # noqa: E402
from test_gpu_ragged_forward_fp32 import KEYS, _check_pair, _same  # noqa: E402

DEV = 'cuda:0'
W4 = ((544, 130), (70, 520), (300, 257), (513, 513))
W8 = ((1056, 100), (90, 1040), (700, 1025))
SETS = {'W4': (W4, [64, None]), 'W8': (W8, [64, None]), 'WF': (W4, [])}
FIRST_PAIR = {'W4': (0, 1, 2, 3), 'W8': (0, 1, 2), 'WF': (0, 1, 2, 3)}        # synth.make_batch(..., first_pair=): chosen on the CPU, from the oracle alone
DECIDED = {'W4': (), 'W8': (), 'WF': (0, 1, 2, 3)}
FORMS = ('pair', 'split')
WINDOWED, WIDE4, WIDE4_TAP, WIDE8, WIDE8_TAP = ops.RAGGED_WIDE_LAUNCHES[4:]
SK16, SK32, ITER, FINISH = ops.RAGGED_WIDE_LAUNCHES[:4]
ITERS = 20


def _cfg(name, **over):
    return synth.default_config(L=1, k=SETS[name][1], sinkhorn_iterations=ITERS, **over)


@functools.lru_cache(maxsize=None)
def _net(name, form='pair', ragged_arithmetic='auto', slots='wide', descriptor='FPFH'):
    net = MDGAT({**_cfg(name, descriptor=descriptor), 'ragged_arithmetic': ragged_arithmetic, 'ragged_slots_fp32': slots, 'ragged_sinkhorn_fp32': form})
    net.load_state_dict(synth.make_state_dict(L=1, seed=1, descriptor=descriptor))
    net = net.float().eval().to(DEV)
    assert net._ragged_fp32() and not net.exact() and net.ragged_slots_fp32 == slots
    return net


@functools.lru_cache(maxsize=None)
def _pairs(name, device=DEV):
    return tuple({k: v.to(device) for k, v in synth.make_batch(1, n, m, first_pair=s).items()} for (n, m), s in zip(SETS[name][0], FIRST_PAIR[name]))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """the oracle on every pair of the set alone, once: (outputs, Z, smallest top-k gap, smallest arg-max margin) per pair"""
    sd = synth.make_state_dict(L=1, seed=1)
    out = []
    for p in _pairs(name, 'cpu'):
        ref, cap, gap, margin = RD.oracle_pair(sd, _cfg(name), p)
        out.append((ref, cap['Z'], gap, margin))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _forward(name, form):
    """forward_ragged of the set with Z, and what the wide counters saw of it"""
    before = ops.ragged_wide_launches()
    with torch.no_grad():
        got = _net(name, form).forward_ragged(list(_pairs(name)), return_Z=True)
    _net(name, form).check(DEV)
    after = ops.ragged_wide_launches()
    return got, {k: after[k] - before[k] for k in after if after[k] != before[k]}


def test_the_decided_pairs_are_the_ones_written_down():
    for name in SETS:
        got = tuple(b for b, (_, _, gap, margin) in enumerate(_oracle(name)) if RD.decided(gap, margin))
        print(name, [(f'{gap:.2e}', f'{margin:.2e}') for _, _, gap, margin in _oracle(name)])
        assert got == DECIDED[name], (name, got)
    assert len(DECIDED['WF']) >= 1


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', list(SETS))
def test_forward_ragged_against_the_oracle_on_every_pair(name, form):
    got, launched = _forward(name, form)
    # one layer pair: a self and a cross layer; the dynamic one (layer 0 of k = [64, None]) on the wide kernel, the full ones windowed
    dyn = sum(k is not None for k in SETS[name][1])
    want = {WINDOWED: 2 - dyn}
    if dyn:
        want[WIDE4 if name == 'W4' else WIDE8] = dyn
    want.update({ITER: ITERS, FINISH: 1} if form == 'split' else {SK16 if name != 'W8' else SK32: 1})
    assert launched == want, (name, form, launched)
    for b, (o, (ref, Z, _, _)) in enumerate(zip(got, _oracle(name))):
        n, m = SETS[name][0][b]
        assert set(o) == set(KEYS) | {'Z'} and tuple(o['Z'].shape) == (1, n + 1, m + 1) and o['Z'].dtype == torch.float32
        assert o['matches0'].dtype == torch.int64 and tuple(o['matches0'].shape) == (1, n) and tuple(o['matches1'].shape) == (1, m)
        _check_pair(o, ref['matches0'], ref['matches1'], ref['matching_scores0'], ref['matching_scores1'], Z, b in DECIDED[name],
                    f'set {name} ({form}) pair {b} ({n} x {m})')


@pytest.mark.parametrize('name,form,orders', [('W4', 'pair', ([3, 1, 0, 2], [1, 0])), ('WF', 'split', ([2, 0, 3, 1], [0, 1, 3])), ('W8', 'pair', ([1, 0],))])
def test_results_do_not_depend_on_position_or_companions(name, form, orders):
    """equal slots (pairs 0 and 1 set them): permutations and subsets, as packed batches, give every pair the same bits"""
    net, pairs, ref = _net(name, form), list(_pairs(name)), _forward(name, form)[0]
    with torch.no_grad():
        for order in orders:
            got = net.forward_ragged(ops.pack_ragged([pairs[i] for i in order]), return_Z=True)
            for i, p in enumerate(order):
                _same(got[i], ref[p], (name, order, p))


@pytest.mark.parametrize('poison', [float('nan'), 1e300])
@pytest.mark.parametrize('name,form', [('W4', 'pair'), ('WF', 'split')])
def test_padding_reaches_nothing(name, form, poison):
    net, ref = _net(name, form), _forward(name, form)[0]
    packed = ops.pack_ragged(list(_pairs(name)))
    bad = dict(packed)
    for f, cnt in (('0', packed['counts0_host']), ('1', packed['counts1_host'])):
        for key in ('keypoints', 'scores', 'descriptors'):
            t = packed[key + f].clone()
            for b, c in enumerate(cnt.tolist()):
                t[b, c:] = poison
            bad[key + f] = t
    with torch.no_grad():
        got = net.forward_ragged(bad, return_Z=True)
    net.check(DEV)
    for b in range(len(ref)):
        _same(got[b], ref[b], (name, b))
        assert torch.isfinite(got[b]['Z']).all()


@pytest.mark.parametrize('form', FORMS)
def test_the_key_is_inert_on_narrow_slots(form):
    """SET_A of the 512-limited test: a module with the key and one without give the same bits, and no wide launch is counted"""
    import test_gpu_ragged_forward_fp32 as RF
    pairs = list(RF._pairs('A'))

    def net(slots):
        m = MDGAT({**RF._cfg('A'), 'ragged_arithmetic': 'auto', 'ragged_slots_fp32': slots, 'ragged_sinkhorn_fp32': form})
        m.load_state_dict(synth.make_state_dict(L=RF.SETS['A'][1], seed=1))
        return m.float().eval().to(DEV)
    before = ops.ragged_wide_launches()
    with torch.no_grad():
        wide = net('wide').forward_ragged(pairs, return_Z=True)
        narrow = net('narrow').forward_ragged(pairs, return_Z=True)
    assert ops.ragged_wide_launches() == before
    for b in range(len(pairs)):
        _same(wide[b], narrow[b], b)


def test_evaluate_ragged_equals_evaluate_matches_on_every_pairs_own_outputs():
    net = _net('W4')
    pairs = []
    for b, p in enumerate(_pairs('W4')):
        rs = np.random.RandomState(100 + b)
        th = 0.05 * rs.standard_normal()
        T = np.eye(4)
        T[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
        T[:3, 3] = 0.3 * rs.standard_normal(3)
        T = torch.from_numpy(T)[None].to(DEV)
        g0, g1, _ = ops.gt_matches(p['keypoints0'], p['keypoints1'], T1=T, threshold=1.5)
        pairs.append({**p, 'gt_matches0': g0, 'gt_matches1': g1, 'T_gt': T})
    with torch.no_grad():
        got = net.evaluate_ragged(pairs)
        fwd = net.forward_ragged(pairs)
    for b, p in enumerate(pairs):
        _same(got['pairs'][b], fwd[b], b)
        _same(fwd[b], {k: _forward('W4', 'pair')[0][b][k] for k in KEYS}, b)
        metrics, T, _ = ops.evaluate_matches(fwd[b]['matches0'], fwd[b]['matches1'], p['gt_matches0'], p['gt_matches1'], p['keypoints0'],
                                             p['keypoints1'], T_gt=p['T_gt'])
        assert got['metrics'][b].cpu().numpy().tobytes() == metrics[0].cpu().numpy().tobytes(), b
        assert got['T'][b].cpu().numpy().tobytes() == T[0].cpu().numpy().tobytes(), b


def _record(k, s, f):
    return np.concatenate([k, s[:, None], f], axis=1).astype(np.float32)


@pytest.mark.parametrize('form', FORMS)
def test_the_bank_entry_equals_forward_ragged_on_the_assembled_chunk(form):
    """a bank with frames beyond 512 under ragged_arithmetic = 'module': bit for bit forward_ragged on the chunk assembled from it"""
    frames = []
    for b, (n, m) in enumerate(W4):
        k0, s0, f0, k1, s1, f1 = synth.make_pair(n, m, b)
        frames += [_record(k0, s0, f0), _record(k1, s1, f1)]
    bank = ops.pack_frames(frames, DEV)
    idx0, idx1 = list(range(0, 2 * len(W4), 2)), list(range(1, 2 * len(W4), 2))
    net = _net('W4', form, 'module')
    before = ops.ragged_wide_launches()
    with torch.no_grad():
        got = net.match_frames_ragged(bank, idx0, idx1, return_Z=True)
    assert ops.ragged_wide_launches()[WIDE4] == before[WIDE4] + 1
    with torch.no_grad():
        ref = net.forward_ragged(ops.assemble_frames_ragged(bank, idx0, idx1), return_Z=True)
    for b in range(len(W4)):
        assert set(got[b]) == set(KEYS) | {'Z'}
        _same(got[b], ref[b], b)


def test_the_pooled_descriptor_runs_a_wide_chunk():
    """a float32 'FPFH_gloabal' module (its encoders in fp64, on the handle that runs them alone): a wide chunk through the wide kernels,
    every pair's bits independent of its companions"""
    net = _net('W4', 'pair', 'module', descriptor='FPFH_gloabal')
    pairs = list(_pairs('W4'))
    before = ops.ragged_wide_launches()
    with torch.no_grad():
        got = net.forward_ragged(pairs, return_Z=True)
        sub = net.forward_ragged([pairs[1], pairs[0]], return_Z=True)
    net.check(DEV)
    after = ops.ragged_wide_launches()
    assert after[WIDE4] == before[WIDE4] + 2 and after[SK16] == before[SK16] + 2
    for b, (n, m) in enumerate(W4):
        assert tuple(got[b]['Z'].shape) == (1, n + 1, m + 1) and torch.isfinite(got[b]['Z']).all()
    _same(sub[0], got[1], 1)
    _same(sub[1], got[0], 0)


def test_refusals_on_the_device():
    net, pairs = _net('W4'), list(_pairs('W4'))
    with pytest.raises(ValueError, match='pair 4 has 2049 x 64 keypoints: ragged batches hold at most 2048 per frame'):
        net.forward_ragged(pairs + [{k: v.to(DEV) for k, v in synth.make_batch(1, 2049, 64).items()}])
    with pytest.raises(ValueError, match='fewer than a dynamic layer keeps'):
        net.forward_ragged(pairs + [{k: v.to(DEV) for k, v in synth.make_batch(1, 63, 600).items()}])
    with pytest.raises(ValueError, match='at most 512 per frame'):
        _net('W4', slots='narrow').forward_ragged(pairs)
    with torch.no_grad():
        got = net.forward_ragged(pairs, return_Z=True)          # (and the module still runs)
    for b in range(len(pairs)):
        _same(got[b], _forward('W4', 'pair')[0][b], b)
