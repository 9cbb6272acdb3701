"""GPU parity of the evaluation scripts' per-pair record (csrc/eval_metrics.hip through ops.evaluate_matches, ops.EvalMeter,
MDGAT.evaluate) with the numpy restatement of test.py:212-342 and test_registration_metric.py:213-286 (tests/eval_ref.py, pinned to
the scripts' own outputs by tests/test_eval_ref.py) on the recorded cases of tests/golden/eval_cases.npz.  Counts, status bits and
ratios must be EQUAL (NaN matching NaN, inf matching inf: one fp64 division of the same two integers on both sides); the pose
columns stay within the tolerances tests/test_gpu_postproc.py uses for mdgat_pose (1e-9 on T and the translation error, 1e-7 on the
rotation error, 1e-12 on the inlier ratio, the inlier count equal)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_ref as E  # noqa: E402
from mdgat_matcher_amd import MDGAT, _lib, ops, synth  # noqa: E402

DEV = 'cuda:0'
COLS = ops.EvalColumns
BITS = {k: getattr(COLS, k) for k in ('BANNED', 'TOO_FEW_MATCHES', 'REGISTRATION_FAIL', 'RTE_OK', 'RRE_OK')}
POSE_COLS = ('inliers', 'inlier_ratio', 'trans_error', 'rot_error')
POSE_TOL = {'inliers': 0.0, 'inlier_ratio': 1e-12, 'trans_error': 1e-9, 'rot_error': 1e-7}      # tests/test_gpu_postproc.py:49-50
POSE_BITS = BITS['REGISTRATION_FAIL'] | BITS['RTE_OK'] | BITS['RRE_OK']


@pytest.fixture(scope='module')
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, 'eval_cases.npz'))


@pytest.fixture(scope='module')
def expected(cases):
    """name -> (inputs, [(row, pose_defined) per pair]): the restatement, computed once and shared."""
    out = {}
    for name in cases['groups']:
        g, _ = E.load_group(cases, name)
        out[name] = (g, [E.expected_row(E.as_pred(g, [b]), 0, COLS, BITS) for b in range(len(g['matches0']))])
    return out


def _run(g, pairs=None, T_gt=True):
    sel = slice(None) if pairs is None else list(pairs)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(g[k][sel])).to(DEV)      # noqa: E731
    m, T, cols = ops.evaluate_matches(t('matches0'), t('matches1'), t('gt0'), t('gt1'), t('kpts0'), t('kpts1'),
                                      T_gt=t('T_gt') if T_gt else None)
    assert cols is COLS and m.dtype == torch.float64 and tuple(m.shape) == (len(g['matches0'][sel]), len(COLS))
    return m.cpu().numpy(), T.cpu().numpy()


def _check_rows(name, got, want):
    for b, (row, pose_defined) in enumerate(want):
        for col, i in COLS.items():
            if col in POSE_COLS or col == 'status':
                continue
            assert np.array_equal(got[b, i], row[i], equal_nan=True), (name, b, col, got[b, i], row[i])
        gs, ws = int(got[b, COLS.status]), int(row[COLS.status])
        if not pose_defined:          # < 4 matches: the rank-deficient pose is the SVD routine's choice (test_gpu_postproc.py:110-114)
            assert gs & ~POSE_BITS == ws & ~POSE_BITS, (name, b, gs, ws)
            if row[COLS.n_valid] == 0:
                assert all(np.isnan(got[b, COLS[c]]) for c in POSE_COLS[1:]) and got[b, COLS.inliers] == 0 and gs & BITS['REGISTRATION_FAIL']
            continue
        assert gs == ws, (name, b, gs, ws)
        for col in POSE_COLS:
            assert abs(got[b, COLS[col]] - row[COLS[col]]) <= POSE_TOL[col], (name, b, col, got[b, COLS[col]], row[COLS[col]])


@pytest.mark.parametrize('name', ['rand17', 'n48m64', 'n300m500', 'rule_none', 'rule_three', 'rule_banned', 'rule_allneg', 'rule_perfect',
                                  'meter6'])
def test_rows_match_the_scripts(expected, name):
    g, want = expected[name]
    got, T = _run(g)
    _check_rows(name, got, want)
    for b, (row, pose_defined) in enumerate(want):
        if pose_defined:
            pred = E.as_pred(g, [b])
            valid = pred['matches0'][0] > -1
            Tr = E.solve_icp(pred['keypoints1'][0][pred['matches0'][0][valid]], pred['keypoints0'][0][valid])
            assert np.abs(T[b] - Tr).max() < 1e-9, (name, b)


def test_rule_cases_set_the_bits_the_scripts_act_on(expected):
    """What each rule case is there for, stated outright (the values themselves: test_rows_match_the_scripts)."""
    row = lambda name: _run(expected[name][0])[0][0]                             # noqa: E731
    r = row('rule_none')
    assert r[COLS.n_valid] == 0 and r[COLS.precision] == 0 and r[COLS.recall] == 0 and int(r[COLS.status]) & BITS['TOO_FEW_MATCHES']
    r = row('rule_three')
    assert r[COLS.n_valid] == 3 and int(r[COLS.status]) & BITS['TOO_FEW_MATCHES'] and not int(r[COLS.status]) & BITS['BANNED']
    assert not int(r[COLS.status]) & (BITS['RTE_OK'] | BITS['RRE_OK'])
    r = row('rule_banned')
    assert r[COLS.n_valid_gt] == 3 and int(r[COLS.status]) & BITS['BANNED']
    r = row('rule_allneg')          # the unguarded divisions: 0/0 and x/0 as numpy gives them
    assert r[COLS.n_valid_gt] == 0 and np.isnan(r[COLS.tp_rate]) and np.isnan(r[COLS.tp_rate2]) and np.isnan(r[COLS.tp_rate_reg])
    assert r[COLS.recall] == np.inf or np.isnan(r[COLS.recall])
    assert r[COLS.fp_rate] == r[COLS.n_valid] / 33
    r = row('rule_perfect')
    assert r[COLS.precision] == 1 and r[COLS.recall] == 1 and r[COLS.accuracy] == 1 and r[COLS.fp_rate] == 0 and r[COLS.tp_rate] == 1
    assert int(r[COLS.status]) == BITS['RTE_OK'] | BITS['RRE_OK']


def test_a_pair_does_not_depend_on_its_batch(expected):
    g, _ = expected['n48m64']
    alone, T_alone = _run(g, [1])
    h = {k: np.stack([v[0], v[1], v[0]]) for k, v in g.items()}
    batch, T_batch = _run(h)
    assert alone[0].tobytes() == batch[1].tobytes() and T_alone[0].tobytes() == T_batch[1].tobytes()


def test_bit_reproducible(expected):
    g, _ = expected['n300m500']
    a, Ta = _run(g)
    b, Tb = _run(g)
    assert a.tobytes() == b.tobytes() and Ta.tobytes() == Tb.tobytes()


def test_no_ground_truth_pose(expected):
    g, want = expected['n48m64']
    got, _ = _run(g, T_gt=False)
    ref, _ = _run(g)
    for b in range(2):
        assert np.isnan(got[b, COLS.trans_error]) and np.isnan(got[b, COLS.rot_error])
        assert int(got[b, COLS.status]) == BITS['REGISTRATION_FAIL']
        assert got[b, :COLS.trans_error].tobytes() == ref[b, :COLS.trans_error].tobytes()


def _raw(B, N, M, g, metrics, T, bad):
    t = lambda k, dt: torch.from_numpy(np.ascontiguousarray(g[k])).to(device=DEV, dtype=dt)      # noqa: E731
    keep = [t('matches0', torch.int64), t('matches1', torch.int64), t('gt0', torch.int64), t('gt1', torch.int64),
            t('kpts0', torch.float32), t('kpts1', torch.float32), t('T_gt', torch.float64)]
    rc = _lib.load().mdgat_eval_metrics(B, N, M, *[x.data_ptr() for x in keep], 1.0, metrics.data_ptr(), T.data_ptr(), bad.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_out_of_range_gt(expected):
    g, want = expected['n48m64']
    h = {k: v.copy() for k, v in g.items()}
    h['gt0'][1, 5] = 64 + 1
    metrics = torch.zeros((2, len(COLS)), dtype=torch.float64, device=DEV)
    T = torch.zeros((2, 4, 4), dtype=torch.float64, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _raw(2, 48, 64, h, metrics, T, bad) == _lib.OK
    assert int(bad.item()) == 1
    m = metrics.cpu().numpy()
    assert np.isnan(m[1]).all() and torch.isnan(T[1]).all()
    _check_rows('n48m64', m[:1], want[:1])                      # the other pair of the batch is untouched by it
    with pytest.raises(IndexError):
        _run(h)
    h = {k: v.copy() for k, v in g.items()}
    h['gt1'][0, 0] = -2
    with pytest.raises(IndexError):
        _run(h)


def test_empty_batch_writes_nothing(expected):
    g, _ = expected['n48m64']
    metrics = torch.full((1, len(COLS)), 7.0, dtype=torch.float64, device=DEV)
    T = torch.full((1, 4, 4), 7.0, dtype=torch.float64, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _raw(0, 48, 64, g, metrics, T, bad) == _lib.OK
    assert bool((metrics == 7.0).all()) and bool((T == 7.0).all()) and int(bad.item()) == 0
    m, T, _ = ops.evaluate_matches(*(torch.zeros((0, n), dtype=torch.int64, device=DEV) for n in (48, 64, 48, 64)),
                                   torch.zeros((0, 48, 3), device=DEV), torch.zeros((0, 64, 3), device=DEV))
    assert tuple(m.shape) == (0, len(COLS)) and tuple(T.shape) == (0, 4, 4)


def test_shape_limit():
    N = 2176
    z = torch.zeros((1, N), dtype=torch.int64, device=DEV)
    k = torch.zeros((1, N, 3), device=DEV)
    metrics = torch.zeros((1, len(COLS)), dtype=torch.float64, device=DEV)
    T = torch.zeros((1, 4, 4), dtype=torch.float64, device=DEV)
    rc = _lib.load().mdgat_eval_metrics(1, N, N, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), k.data_ptr(), k.data_ptr(), None, 1.0,
                                        metrics.data_ptr(), T.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_UNSUPPORTED and '2175' in _lib.last_error()
    with pytest.raises(RuntimeError):
        ops.evaluate_matches(z, z, z, z, k, k)


def test_largest_shape(expected):
    """N = M = 2175, the limit: every keypoint matched to itself, identity pose."""
    N = 2175
    rs = np.random.RandomState(5)
    k = torch.from_numpy((20 * rs.standard_normal((1, N, 3))).astype(np.float32)).to(DEV)
    ident = torch.arange(N, device=DEV)[None]
    m, T, _ = ops.evaluate_matches(ident, ident, ident, ident, k, k, T_gt=torch.eye(4, dtype=torch.float64)[None])
    r = m[0].cpu().numpy()
    assert r[COLS.n_valid] == N and r[COLS.true_positive] == N and r[COLS.precision] == 1 and r[COLS.inliers] == N
    assert r[COLS.trans_error] < 1e-9 and np.abs(T[0].cpu().numpy() - np.eye(4)).max() < 1e-9


def test_meter_agrees_with_the_scripts(cases, expected):
    """EvalMeter over the 6-pair batch (one banned, one with three matches, one whose pose fails) against the means and counters the
    scripts themselves printed for it (recorded in the fixture): equal, the two pose means within the pose tolerance."""
    g, rec = E.load_group(cases, 'meter6')
    got, _ = _run(g)
    status = got[:, COLS.status].astype(int)
    assert status[1] & BITS['BANNED'] and status[3] & BITS['TOO_FEW_MATCHES'] and status[4] & BITS['REGISTRATION_FAIL']
    meter = ops.EvalMeter()
    meter.update(np.zeros((0, len(COLS))))          # the recorded run starts with an empty batch (the scripts divide fail by i = 1)
    meter.update(torch.from_numpy(got).to(DEV))
    mine, want = meter.test_py(), rec['means_test_py']
    assert mine['fail'] == want['fail'] == 3 and mine['baned_data'] == want['baned_data'] == 1
    assert mine['fail_rate'] == want['fail'] / want['i'] and mine['baned_data_rate'] == want['baned_data'] / want['i']
    for k, w in (('precision_mean', 'precision_mean'), ('accuracy_mean', 'accuracy_mean'), ('recall_mean', 'recall_mean'),
                 ('repeatability_mean', 'repeatibilty_array_mean'), ('inliers_mean', 'inlier_mean'), ('inlier_ratio_mean', 'inlier_ratio_mean'),
                 ('fp_rate_mean', 'fp_rate_mean'), ('tp_rate_mean', 'tp_rate_mean'), ('tp_rate2_mean', 'tp_rate_mean2'),
                 ('true_positive_mean', 'tm'), ('false_positive_mean', 'fm')):
        assert mine[k] == want[w], (k, mine[k], want[w])
    assert abs(mine['trans_error_mean'] - want['trans_error_mean']) < 1e-9 and abs(mine['rot_error_mean'] - want['rot_error_mean']) < 1e-7
    mine, want = meter.registration(), rec['means_registration']
    assert mine['baned_data'] == want['baned_data'] == 1
    for k, w in (('rep', 'rep_a'), ('inlier', 'inlier_a'), ('inlier_ratio', 'inlier_ratio_a'), ('recall', 'recall_a'), ('tp_rate', 'tp_rate_a'),
                 ('fp_rate', 'fp_rate_a'), ('RR', 'RR'), ('F1', 'F1')):
        assert mine[k] == want[w], (k, mine[k], want[w])
    assert abs(mine['rte'] - want['rte_a']) < 1e-9 and abs(mine['rre'] - want['rre_a']) < 1e-7
    # and with the restatement's meters fed the same pairs
    _, means, fail_rate, _ = E.test_py_loop([E.EMPTY_BATCH, E.as_pred(g)])
    assert meter.test_py()['precision_mean'] == means['precision'] and meter.test_py()['fail_rate'] == fail_rate


def test_evaluate_end_to_end():
    """MDGAT.evaluate on the small synthetic checkpoint of the drop-in tests: 'metrics' is ops.evaluate_matches on the same forward's
    outputs, and forward's own outputs are what forward returns."""
    L, B, N = 2, 2, 64
    cfg = synth.default_config(L=L, k=[16, None, 8, None], sinkhorn_iterations=20)
    net = MDGAT(cfg).double()
    net.load_state_dict(synth.make_state_dict(L=L, seed=1))
    net = net.double().eval().to(DEV)
    data = synth.make_batch(B, N, N, device=DEV)
    rs = np.random.RandomState(11)
    gt0 = np.stack([rs.permutation(N) for _ in range(B)])
    gt1 = np.argsort(gt0, axis=1)
    drop = rs.uniform(size=(B, N)) < 0.3
    for b in range(B):
        gt1[b, gt0[b, drop[b]]] = -1
    gt0[drop] = -1
    data['gt_matches0'], data['gt_matches1'] = torch.from_numpy(gt0).to(DEV), torch.from_numpy(gt1).to(DEV)
    data['T_gt'] = torch.eye(4, dtype=torch.float64, device=DEV).repeat(B, 1, 1)
    with torch.no_grad():
        fwd = net(data)
        out = net.evaluate(data)
    for k, v in fwd.items():
        assert torch.equal(out[k], v), k
    m, T, _ = ops.evaluate_matches(fwd['matches0'], fwd['matches1'], data['gt_matches0'], data['gt_matches1'], data['keypoints0'],
                                   data['keypoints1'], T_gt=data['T_gt'])
    assert out['metrics'].cpu().numpy().tobytes() == m.cpu().numpy().tobytes() and torch.equal(out['T'].isnan(), T.isnan())
    assert torch.equal(torch.nan_to_num(out['T']), torch.nan_to_num(T))
    assert np.array_equal(gt0, data['gt_matches0'].cpu().numpy())          # the caller's tensors are not rewritten
    pred = {'keypoints0': data['keypoints0'].cpu().numpy().astype(np.float32).astype(np.float64),
            'keypoints1': data['keypoints1'].cpu().numpy().astype(np.float32).astype(np.float64),
            'matches0': fwd['matches0'].cpu().numpy(), 'matches1': fwd['matches1'].cpu().numpy(), 'gt_matches0': gt0, 'gt_matches1': gt1,
            'T_gt': data['T_gt'].cpu().numpy()}
    _check_rows('evaluate', m.cpu().numpy(), [E.expected_row(pred, b, COLS, BITS) for b in range(B)])
    assert ops.EvalMeter().update(out).batches == 1
