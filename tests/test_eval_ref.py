"""The numpy restatement of the evaluation scripts (tests/eval_ref.py) against what the reference itself computed: its pose
functions against tests/golden/aux_pose.npz (utils/utils_test.py run by tools/make_goldens_aux.py), its per-pair blocks and its
means against tests/golden/eval_cases.npz (the scripts' own loop bodies run by tools/make_goldens_eval.py).  No GPU."""
import os

import numpy as np
import pytest

import eval_ref as E

STATUS_BITS = {'BANNED': 1, 'TOO_FEW_MATCHES': 2, 'REGISTRATION_FAIL': 4, 'RTE_OK': 8, 'RRE_OK': 16}


@pytest.fixture(scope='module')
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, 'eval_cases.npz'))


def _same(a, b):
    """Bit-for-bit as values: equal, or both NaN."""
    a, b = np.float64(a), np.float64(b)
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


def test_pose_functions_match_the_reference_outputs(golden_dir):
    g = np.load(os.path.join(golden_dir, 'aux_pose.npz'))
    for name in g['names']:
        mk0, mk1, T_gt, st = g[f'{name}_mkpts0'], g[f'{name}_mkpts1'], g[f'{name}_T_gt'], g[f'{name}_stats']
        with np.errstate(invalid='ignore'):
            T, inlier, ratio, te, re = E.calculate_error(mk0, mk1, T_gt)
            T2, rte, rre = E.calculate_error2(mk0, mk1, T_gt)
        # the same LAPACK call on the same numbers; the matrix products replace torch's einsum / inverse: round-off only
        assert np.abs(T - g[f'{name}_T']).max() < 1e-12 and np.array_equal(T, T2), name
        assert int(inlier) == st[1] and ratio == st[2], name
        for got in (te, rte):
            assert abs(got - st[3]) < 1e-9, name
        for got in (re, rre):
            assert (np.isnan(got) and np.isnan(st[4])) or abs(got - st[4]) < 1e-7, name


def test_per_pair_blocks_match_the_scripts(cases):
    checked = 0
    for name in cases['groups']:
        g, rec = E.load_group(cases, name)
        for b in range(len(g['matches0'])):
            meter = E.TestPyMeter()
            out = E.test_py_pair(E.as_pred(g, [b]), 0, meter)
            want = {k: v[b] for k, v in rec['pair_test_py'].items()}
            assert meter.fail == want['fail'] and meter.baned_data == want['baned_data'], (name, b)
            for k, mine in (('repeatibilty', 'repeatibilty'), ('precision', 'precision'), ('recall', 'recall'), ('tm', 'tm'), ('fm', 'fm'),
                            ('matching_score', 'matching_score'), ('accuracy', 'accuracy'), ('fp_rate', 'fp_rate'), ('tp_rate', 'tp_rate'),
                            ('tp_rate2', 'tp_rate2'), ('inlier', 'inlier'), ('inlier_ratio', 'inlier_ratio')):
                assert (mine in out) == (not np.isnan(want[k])) or (mine in out and np.isnan(out[mine])), (name, b, k)
                if mine in out:
                    assert _same(out[mine], want[k]), (name, b, k, out[mine], want[k])
                    checked += 1
            if 'trans_error' in out:
                assert abs(out['trans_error'] - want['trans_error']) < 1e-9 and abs(out['rot_error'] - want['rot_error']) < 1e-7
            if (g['matches0'][b] > -1).sum() == 0:
                continue                       # the registration script has no guard against an empty match set: not recorded
            rmeter = E.RegistrationMeter()
            out = E.registration_pair(E.as_pred(g, [b]), 0, rmeter)
            want = {k: v[b] for k, v in rec['pair_registration'].items()}
            assert rmeter.baned_data == want['baned_data'], (name, b)
            if out.get('banned'):
                continue
            for k in ('repeatibilty', 'precision_inlier_ratio', 'recall', 'fp_rate', 'tp_rate', 'inlier', 'false_positive'):
                assert _same(out[k], want[k]), (name, b, k, out[k], want[k])
                checked += 1
            if (g['matches0'][b] > -1).sum() >= 4:          # (fewer: the null vector of a rank-deficient SVD is the routine's choice)
                assert abs(out['rte'] - want['rte']) < 1e-9 and abs(out['rre'] - want['rre']) < 1e-7, (name, b)
            assert rmeter.RR.sum == want['RR'], (name, b)
    assert checked > 200


def test_means_match_the_scripts(cases):
    """The whole loop on each group as one batch: np.mean over the lists (test.py:326-342), the running averages and F1
    (test_registration_metric.py:282-286).  The pose means are round-off away (matrix products for torch's), the others equal."""
    for name in cases['groups']:
        g, rec = E.load_group(cases, name)
        meter, means, fail_rate, baned_rate = E.test_py_loop([E.EMPTY_BATCH, E.as_pred(g)])
        want = rec['means_test_py']
        assert meter.fail == want['fail'] and meter.baned_data == want['baned_data'] and meter.i == want['i'], name
        for mine, k in (('precision', 'precision_mean'), ('accuracy', 'accuracy_mean'), ('recall', 'recall_mean'),
                        ('repeatibilty', 'repeatibilty_array_mean'), ('inlier', 'inlier_mean'), ('inlier_ratio', 'inlier_ratio_mean'),
                        ('fp_rate', 'fp_rate_mean'), ('tp_rate', 'tp_rate_mean'), ('tp_rate2', 'tp_rate_mean2'), ('tm', 'tm'), ('fm', 'fm')):
            assert _same(means[mine], want[k]), (name, k, means[mine], want[k])
        for mine, k, tol in (('trans_error', 'trans_error_mean', 1e-9), ('rot_error', 'rot_error_mean', 1e-7)):
            assert _same(means[mine], want[k]) or abs(means[mine] - want[k]) < tol, (name, k)
        if 'means_registration' not in rec:
            continue
        rmeter, report = E.registration_loop([E.EMPTY_BATCH, E.as_pred(g)])
        want = rec['means_registration']
        assert rmeter.baned_data == want['baned_data'], name
        for mine, k in (('rep', 'rep_a'), ('inlier', 'inlier_a'), ('inlier_ratio', 'inlier_ratio_a'), ('recall', 'recall_a'),
                        ('tp_rate', 'tp_rate_a'), ('fp_rate', 'fp_rate_a'), ('RR', 'RR'), ('F1', 'F1')):
            assert _same(report[mine], want[k]), (name, k, report[mine], want[k])
        assert abs(report['rte'] - want['rte_a']) < 1e-9 and abs(report['rre'] - want['rre_a']) < 1e-7, name


def test_expected_row_is_the_two_blocks(cases):
    """The row the GPU tests expect from the kernel holds, column by column, what the two blocks computed - wherever they got that far."""
    from mdgat_matcher_amd import _lib
    cols = {n: i for i, n in enumerate(_lib.EVAL_COLUMNS)}
    for name in cases['groups']:
        g, _ = E.load_group(cases, name)
        for b in range(len(g['matches0'])):
            pred = E.as_pred(g, [b])
            row, pose_defined = E.expected_row(pred, 0, cols, STATUS_BITS)
            status = int(row[cols['status']])
            a = E.test_py_pair(pred, 0, E.TestPyMeter())
            assert bool(status & 1) == bool(a.get('banned')) and _same(row[cols['repeatability']], a['repeatibilty'])
            if not a.get('banned'):
                assert bool(status & 2) == bool(a.get('too_few'))
            if 'precision' in a:
                for k, mine in (('precision', 'precision'), ('recall', 'recall'), ('true_positive', 'tm'), ('false_positive', 'fm'),
                                ('matching_score', 'matching_score'), ('accuracy', 'accuracy'), ('fp_rate', 'fp_rate'), ('tp_rate', 'tp_rate'),
                                ('tp_rate2', 'tp_rate2'), ('true_negative', 'true_negative'), ('inliers', 'inlier'),
                                ('inlier_ratio', 'inlier_ratio'), ('trans_error', 'trans_error'), ('rot_error', 'rot_error')):
                    assert _same(row[cols[k]], a[mine]), (name, b, k)
                assert bool(status & 4) == bool(a.get('registration_fail')) and pose_defined
            if (g['matches0'][b] > -1).sum() == 0:
                continue
            rmeter = E.RegistrationMeter()
            r = E.registration_pair(pred, 0, rmeter)
            if r.get('banned'):
                continue
            for k, mine in (('precision', 'precision_inlier_ratio'), ('recall', 'recall'), ('fp_rate_reg', 'fp_rate'), ('tp_rate_reg', 'tp_rate'),
                            ('true_positive', 'inlier'), ('false_positive_reg', 'false_positive'), ('false_negative', 'false_negative')):
                assert _same(row[cols[k]], r[mine]), (name, b, k)
            assert rmeter.RR.sum == (1 if (status & 8) and (status & 16) else 0)
            assert rmeter.rte_a.count == bool(status & 8) and rmeter.rre_a.count == bool(status & 16)


def test_eval_meter_on_restated_rows(cases):
    """ops.EvalMeter (host code) fed the restatement's rows reports what the scripts printed for every recorded group: the rules and
    the means are checked here without a GPU, the kernel's rows in tests/test_gpu_eval.py."""
    from mdgat_matcher_amd import _lib, ops
    cols = {n: i for i, n in enumerate(_lib.EVAL_COLUMNS)}
    for name in cases['groups']:
        g, rec = E.load_group(cases, name)
        pred = E.as_pred(g)
        rows = np.stack([E.expected_row(pred, b, cols, STATUS_BITS)[0] for b in range(len(g['matches0']))])
        meter = ops.EvalMeter().update(np.zeros((0, len(cols)))).update(rows)
        mine, want = meter.test_py(), rec['means_test_py']
        assert mine['fail'] == want['fail'] and mine['baned_data'] == want['baned_data'] and mine['fail_rate'] == want['fail'] / want['i'], name
        for k, w in (('precision_mean', 'precision_mean'), ('accuracy_mean', 'accuracy_mean'), ('recall_mean', 'recall_mean'),
                     ('repeatability_mean', 'repeatibilty_array_mean'), ('inliers_mean', 'inlier_mean'), ('inlier_ratio_mean', 'inlier_ratio_mean'),
                     ('fp_rate_mean', 'fp_rate_mean'), ('tp_rate_mean', 'tp_rate_mean'), ('tp_rate2_mean', 'tp_rate_mean2'),
                     ('true_positive_mean', 'tm'), ('false_positive_mean', 'fm')):
            assert _same(mine[k], want[w]), (name, k, mine[k], want[w])
        for k, tol in (('trans_error_mean', 1e-9), ('rot_error_mean', 1e-7)):
            assert _same(mine[k], want[k]) or abs(mine[k] - want[k]) < tol, (name, k)
        if 'means_registration' not in rec:
            continue
        mine, want = meter.registration(), rec['means_registration']
        assert mine['baned_data'] == want['baned_data'], name
        for k, w in (('rep', 'rep_a'), ('inlier', 'inlier_a'), ('inlier_ratio', 'inlier_ratio_a'), ('recall', 'recall_a'), ('tp_rate', 'tp_rate_a'),
                     ('fp_rate', 'fp_rate_a'), ('RR', 'RR'), ('F1', 'F1')):
            assert _same(mine[k], want[w]), (name, k, mine[k], want[w])
        assert abs(mine['rte'] - want['rte_a']) < 1e-9 and abs(mine['rre'] - want['rre_a']) < 1e-7, name
