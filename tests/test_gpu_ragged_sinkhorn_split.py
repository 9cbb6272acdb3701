"""config['ragged_sinkhorn_fp32'] = 'split': the fp32-class ragged forward on the split form of the fp32 Sinkhorn (csrc/sinkhorn.hip: a
pair's rows over ceil(Np / 128) workgroups, one launch per iteration and a finishing one).  All cases: a float32 module with
``ragged_arithmetic='auto'`` (the bank case: 'module'), L = 1, ``forward_ragged`` with Z.

The chunks are tests/ragged_split_cases.py's - A: slot 130 x 70, the second slab holds 2, 0, 1 and 0 rows; B: slot 512 x 500, four slabs -
and the yardstick the fp64 oracle on every pair alone, split as tests/ragged_decided.py describes: a DECIDED pair (every arg-max margin of
the oracle's Z >= 1e-4; these networks have no dynamic layer) must give the oracle's matches and its Z within 1e-4; on the others no match
may differ from the default form's.  Which pairs are decided is written down in ragged_split_cases.DECIDED - at least half of each chunk,
at every iteration count - and held against the oracle on the CPU by test_ragged_sinkhorn_split.py.

Measured on an MI355X (the largest |dZ| over the pairs' own blocks; the default form's own figure against the oracle is 1.8e-5):
    chunk A   against the oracle 1.97e-5, 2.00e-5, 1.96e-5, 1.15e-5 at 1, 2, 3, 20 iterations; against the default form 7.6e-6
    chunk B   against the oracle 2.83e-5 (pair (512, 500)); against the default form 7.6e-6"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdgat_matcher_amd import MDGAT, _lib, ops, synth  # noqa: E402
from parity_util import Z_TOL  # noqa: E402
from prefilled import prefilled, refill_cached, same_bits, snapshot, spy  # noqa: E402
import ragged_split_cases as CASES  # noqa: E402

DEV = 'cuda:0'
KEYS = ('matches0', 'matches1', 'matching_scores0', 'matching_scores1', 'loss')


def _new_net(iters, form, ragged_arithmetic='auto'):
    over = {} if form is None else {'ragged_sinkhorn_fp32': form}
    net = MDGAT({**CASES.cfg(iters), 'ragged_arithmetic': ragged_arithmetic, **over})
    net.load_state_dict(CASES.state_dict())
    net = net.float().eval().to(DEV)
    assert net._ragged_fp32() and not net.exact() and net.ragged_sinkhorn_fp32 == (form or 'pair')
    return net


_net = functools.lru_cache(maxsize=None)(_new_net)


def _pairs(name):
    return list(CASES.pairs(name, DEV))


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


def _sinkhorn_launches(net, pairs):
    """mdgat_profile's launch count of the Sinkhorn class over one forward_ragged"""
    net.profile(DEV, True)
    try:
        with torch.no_grad():
            out = net.forward_ragged(pairs, return_Z=True)
        torch.cuda.synchronize()
    finally:
        prof = net.profile(DEV, False)
    return prof['sinkhorn'][1], out


# ---------------------------------------------------------------------------------------------------- 1. the form ran
@pytest.mark.parametrize('name,iters', [('A', 3), ('A', 20), ('B', 100)])
def test_a_slot_of_two_slabs_or_more_runs_one_launch_per_iteration(name, iters):
    pairs = _pairs(name)
    n_pair, _ = _sinkhorn_launches(_net(iters, None), pairs)
    n_split, _ = _sinkhorn_launches(_net(iters, 'split'), pairs)
    print(f'chunk {name}, {iters} iterations: Sinkhorn launches {n_pair} (pair), {n_split} (split)')
    assert n_pair >= 1 and n_split == n_pair + iters, (n_pair, n_split)


@pytest.mark.parametrize('counts', [((64, 64), (40, 33), (17, 64)), ((128, 100), (100, 64), (16, 70))])
def test_a_slot_of_one_slab_keeps_the_one_workgroup_kernel(counts):
    """slots of 64 x 64 and 128 x 100 have G = 1: the same launches, the same bits"""
    pairs = [{k: v.to(DEV) for k, v in synth.make_batch(1, n, m, first_pair=b).items()} for b, (n, m) in enumerate(counts)]
    n_pair, ref = _sinkhorn_launches(_net(20, None), pairs)
    n_split, got = _sinkhorn_launches(_net(20, 'split'), pairs)
    assert n_split == n_pair, (n_pair, n_split)
    for b in range(len(counts)):
        _same(got[b], ref[b], (counts, b))


# ---------------------------------------------------------------------------------------------------- 2. the smallest shapes that can go wrong
@pytest.mark.parametrize('name,iters', [(n, i) for n in sorted(CASES.CHUNKS) for i in CASES.ITERS[n]])
def test_against_the_oracle_on_every_pairs_own_rows(name, iters):
    pairs, counts = _pairs(name), CASES.CHUNKS[name]
    with torch.no_grad():
        got = _net(iters, 'split').forward_ragged(pairs, return_Z=True)
        default = _net(iters, None).forward_ragged(pairs, return_Z=True)
    _net(iters, 'split').check(DEV)
    worst_oracle = worst_default = 0.0
    for b, (o, d, (ref, Z, _, _)) in enumerate(zip(got, default, CASES.oracle(name, iters))):
        n, m = counts[b]
        what = f'chunk {name}, {iters} iterations, pair {b} ({n} x {m})'
        assert set(o) == set(KEYS) | {'Z'} and tuple(o['Z'].shape) == (1, n + 1, m + 1) and o['Z'].dtype == torch.float32, what
        assert torch.isfinite(o['Z']).all(), what
        err = float((o['Z'].cpu().double() - Z.reshape(o['Z'].shape)).abs().max())
        err_d = float((o['Z'].double() - d['Z'].double()).abs().max())
        worst_oracle, worst_default = max(worst_oracle, err), max(worst_default, err_d)
        decided = b in CASES.DECIDED[name, iters]
        print(f'{what}: decided {decided}; max |Z - oracle| = {err:.3e}, max |Z - default form| = {err_d:.3e}')
        if decided:
            for k in ('matches0', 'matches1'):
                assert torch.equal(o[k].cpu(), ref[k].long().reshape(o[k].shape)), (what, k)
            assert err < Z_TOL, (what, err)
        else:
            assert torch.equal(o['matches0'], d['matches0']) and torch.equal(o['matches1'], d['matches1']), what
    print(f'chunk {name}, {iters} iterations: largest |dZ| against the oracle {worst_oracle:.3e}, against the default form {worst_default:.3e}')


# ---------------------------------------------------------------------------------------------------- 3. independence, bit for bit
@functools.lru_cache(maxsize=None)
def _reference(name, iters):
    with torch.no_grad():
        return _net(iters, 'split').forward_ragged(_pairs(name), return_Z=True)


@pytest.mark.parametrize('name,iters,orders', [('A', 20, ([3, 0, 2, 1], [0, 3], [2, 0])), ('A', 3, ([1, 2, 0, 3],)), ('B', 100, ([2, 1, 0], [0, 2]))])
def test_results_do_not_depend_on_position_or_companions(name, iters, orders):
    """permutations, and subsets that keep the slot sizes (pair 0 sets both slots of either chunk)"""
    net, pairs, ref = _net(iters, 'split'), _pairs(name), _reference(name, iters)
    with torch.no_grad():
        for order in orders:
            got = net.forward_ragged(ops.pack_ragged([pairs[i] for i in order]), return_Z=True)
            for i, p in enumerate(order):
                _same(got[i], ref[p], (name, order, p))


@pytest.mark.parametrize('poison', [float('nan'), 1e300])
@pytest.mark.parametrize('name,iters', [('A', 20), ('B', 100)])
def test_padding_reaches_nothing(name, iters, poison):
    net, ref = _net(iters, 'split'), _reference(name, iters)
    packed = ops.pack_ragged(_pairs(name))
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


@pytest.mark.parametrize('name,iters', [('A', 2), ('A', 20), ('B', 100)])
def test_the_workspace_may_hold_anything(name, iters):
    """a fresh module whose every allocation starts as 0xFF bytes (NaN partials, NaN potentials), then the same module again with its
    cached workspace refilled with 0xFF: the bits of the reference.  The workspace asked for holds the split form's scratch."""
    pairs, ref = _pairs(name), snapshot(_reference(name, iters))
    lib = _lib.load()
    with spy(lib, ('mdgat_workspace_bytes', 'mdgat_forward_ragged')) as s, prefilled('ones') as p:
        net = _new_net(iters, 'split')
        with torch.no_grad():
            got = net.forward_ragged(pairs, return_Z=True)
        torch.cuda.synchronize()
    assert s.calls['mdgat_forward_ragged'] == 1 and s.most_asked() > 0 and p.saw_scratch(s.most_asked()), (s.calls, s.most_asked(), p.scratch_bytes)
    same_bits(ref, snapshot(got), f'chunk {name}: a fresh module under 0xFF')
    B, (Np, Mp) = len(pairs), CASES.CHUNKS[name][0]
    G = (Np + 127) // 128
    with spy(lib, ('mdgat_workspace_bytes',)) as s0:
        with torch.no_grad():
            _net(iters, None).forward_ragged(pairs)
    assert s.most_asked() >= s0.most_asked() + 4 * B * (2 * G * Mp * 2 + 2 * (Np + 1)), (s.most_asked(), s0.most_asked())
    assert refill_cached(net, DEV, 0xFF) > 0
    with prefilled('ones'), torch.no_grad():
        again = net.forward_ragged(pairs, return_Z=True)
        torch.cuda.synchronize()
    same_bits(ref, snapshot(again), f'chunk {name}: the same module, its workspace refilled with 0xFF')


def test_two_calls_in_a_row():
    for name, iters in (('A', 20), ('B', 100), ('A', 20)):
        net, pairs, ref = _net(iters, 'split'), _pairs(name), _reference(name, iters)
        with torch.no_grad():
            first = net.forward_ragged(pairs, return_Z=True)
            second = net.forward_ragged(pairs, return_Z=True)
        for b in range(len(pairs)):
            _same(first[b], ref[b], (name, b))
            _same(second[b], ref[b], (name, b))


# ---------------------------------------------------------------------------------------------------- 4. the bank entry
def _record(k, s, f):
    return np.concatenate([k, s[:, None], f], axis=1).astype(np.float32)


@pytest.mark.parametrize('name,iters', [('A', 20), ('B', 100)])
def test_the_bank_entry_equals_forward_ragged_on_the_assembled_chunk(name, iters):
    counts = CASES.CHUNKS[name]
    frames = []
    for b, (n, m) in enumerate(counts):
        k0, s0, f0, k1, s1, f1 = synth.make_pair(n, m, b)
        frames += [_record(k0, s0, f0), _record(k1, s1, f1)]
    bank = ops.pack_frames(frames, DEV)
    idx0, idx1 = list(range(0, 2 * len(counts), 2)), list(range(1, 2 * len(counts), 2))
    net = _net(iters, 'split', 'module')
    n_pair, _ = _sinkhorn_launches(_net(iters, None, 'module'), ops.assemble_frames_ragged(bank, idx0, idx1))
    net.profile(DEV, True)
    with torch.no_grad():
        got = net.match_frames_ragged(bank, idx0, idx1, return_Z=True)
    torch.cuda.synchronize()
    assert net.profile(DEV, False)['sinkhorn'][1] == n_pair + iters          # (the bank entry ran the split form too)
    with torch.no_grad():
        ref = net.forward_ragged(ops.assemble_frames_ragged(bank, idx0, idx1), return_Z=True)
    for b in range(len(counts)):
        assert set(got[b]) == set(KEYS) | {'Z'}
        _same(got[b], ref[b], (name, b))


def test_evaluate_ragged_agrees_with_the_matches():
    net = _net(20, 'split')
    pairs = []
    for b, p in enumerate(_pairs('A')):
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
    assert tuple(got['metrics'].shape) == (len(pairs), len(ops.EvalColumns))
    for b, p in enumerate(pairs):
        _same(got['pairs'][b], fwd[b], b)
        _same(fwd[b], {k: _reference('A', 20)[b][k] for k in KEYS}, b)
        metrics, T, _ = ops.evaluate_matches(fwd[b]['matches0'], fwd[b]['matches1'], p['gt_matches0'], p['gt_matches1'], p['keypoints0'],
                                             p['keypoints1'], T_gt=p['T_gt'])
        assert got['metrics'][b].cpu().numpy().tobytes() == metrics[0].cpu().numpy().tobytes(), b
        assert got['T'][b].cpu().numpy().tobytes() == T[0].cpu().numpy().tobytes(), b
