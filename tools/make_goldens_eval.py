#!/usr/bin/env python3
"""Generate tests/golden/eval_cases.npz: synthetic matcher outputs and what the reference's two evaluation scripts make of them.

The scripts (test.py, test_registration_metric.py) keep their evaluation under ``if __name__ == '__main__'``, so nothing of it can
be imported.  At generation time only, this tool parses each script with ``ast``, takes the ``with torch.no_grad():`` block of the
main section - the accumulator initialisations, the loop over the loader and the means after it - drops from the loader loop
everything but the loop over the pairs of a batch (that is: the device copies and the forward; the synthetic ``pred`` dicts
already hold the matcher's output), and executes the result UNMODIFIED otherwise, with ``calculate_error`` / ``calculate_error2`` /
``AverageMeter`` imported from the reference's utils/utils_test.py as tools/make_goldens_aux.py imports them, visualisation off and
``print`` silenced.  Only inputs (seeded here) and the numbers the scripts computed are written; no reference text is.

Per pair (the script run on a loader holding that pair alone): every per-pair variable the block had assigned when it was left,
and the counters.  Per group (the script run on the group as one batch): the final means and counters.  The loader always starts
with an empty batch, so that the index ``i`` the scripts divide ``fail`` by is 1 and not 0.

Only runs where the reference tree exists (``MDGAT_REFERENCE``, default /root/reference)."""
import argparse
import ast
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from make_goldens_aux import REF, import_reference_aux, rigid  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'eval_cases.npz')

TEST_PY_VARS = ('repeatibilty', 'precision', 'recall', 'tm', 'fm', 'matching_score', 'accuracy', 'fp_rate', 'tp_rate', 'tp_rate2', 'inlier',
                'inlier_ratio', 'trans_error', 'rot_error')
TEST_PY_MEANS = ('precision_mean', 'accuracy_mean', 'recall_mean', 'trans_error_mean', 'rot_error_mean', 'repeatibilty_array_mean',
                 'inlier_mean', 'inlier_ratio_mean', 'fp_rate_mean', 'tp_rate_mean', 'tp_rate_mean2', 'tm', 'fm')
REG_VARS = ('repeatibilty', 'precision_inlier_ratio', 'recall', 'fp_rate', 'tp_rate', 'rte', 'rre')
REG_METERS = ('rep_a', 'rre_a', 'rte_a', 'inlier_a', 'inlier_ratio_a', 'recall_a', 'tp_rate_a', 'fp_rate_a', 'RR')


def loop_program(script):
    """The evaluation block of a script as a code object: see the module docstring."""
    path = os.path.join(REF, script)
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    main = [n for n in tree.body if isinstance(n, ast.If) and isinstance(n.test, ast.Compare)
            and getattr(n.test.left, 'id', None) == '__name__'][-1]
    block = [n for n in main.body if isinstance(n, ast.With)][-1]
    body = []
    for st in block.body:
        if isinstance(st, ast.For) and isinstance(st.target, ast.Tuple):           # for i, pred in enumerate(test_loader)
            st.body = [s for s in st.body if isinstance(s, ast.For) and getattr(s.target, 'id', None) == 'b']   # for b in range(len(pred['idx0']))
            assert len(st.body) == 1
        body.append(st)
    return compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, 'exec')


def run(program, UT, loader):
    ns = {'np': np, 'torch': torch, 'calculate_error': UT.calculate_error, 'calculate_error2': UT.calculate_error2,
          'AverageMeter': UT.AverageMeter, 'plot_match': None, 'print': lambda *a, **k: None,
          'opt': argparse.Namespace(calculate_pose=True, visualize=False, vis_line_width=0.2), 'test_loader': loader}
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        try:
            exec(program, ns)
        except ZeroDivisionError:        # test_registration_metric.py:282 when every pair was banned (both averages still the integer 0)
            assert 'F1' not in ns and ns['inlier_ratio_a'].count == 0
            ns['F1'] = np.nan
    return ns


def as_pred(g, pairs=None):
    """A group of the fixture as the merged `pred` dict the scripts see (fresh tensors: the scripts rewrite the gts in place)."""
    sel = slice(None) if pairs is None else list(pairs)
    t = lambda a, dt: torch.tensor(np.asarray(a)[sel], dtype=dt)                   # noqa: E731
    pred = {'keypoints0': t(g['kpts0'], torch.double), 'keypoints1': t(g['kpts1'], torch.double),
            'matches0': t(g['matches0'], torch.int64), 'matches1': t(g['matches1'], torch.int64),
            'matching_scores0': t(g['mscores0'], torch.double), 'scores0': t(g['scores0'], torch.double),
            'gt_matches0': t(g['gt0'], torch.int64), 'gt_matches1': t(g['gt1'], torch.int64), 'T_gt': t(g['T_gt'], torch.double)}
    B = pred['matches0'].shape[0]
    pred['idx0'], pred['idx1'], pred['sequence'] = list(range(B)), list(range(B)), ['10'] * B
    return pred


EMPTY = {'idx0': []}


# ------------------------------------------------------------------------------------------ synthetic matcher outputs
def make_pair(rs, N, M, frac_gt=0.6, frac_found=0.8, frac_wrong=0.1, frac_spurious=0.1, dustbin=False, noise=0.05, T_gt=None):
    """One pair: frac_gt of the frame-0 keypoints are re-observed in frame 1 (ground truth), the matcher finds frac_found of those,
    gets frac_wrong of the found ones wrong and matches frac_spurious of the keypoints without ground truth."""
    T_gt = rigid(rs) if T_gt is None else T_gt
    k0 = (20 * rs.standard_normal((N, 3))).astype(np.float32)
    k1 = (20 * rs.standard_normal((M, 3))).astype(np.float32)
    n_gt = int(round(frac_gt * min(N, M)))
    src, dst = rs.permutation(N)[:n_gt], rs.permutation(M)[:n_gt]
    Ti = np.linalg.inv(T_gt)
    k1[dst] = ((Ti[:3, :3] @ k0[src].astype(np.float64).T).T + Ti[:3, 3] + noise * rs.standard_normal((n_gt, 3))).astype(np.float32)
    gt0, gt1 = -np.ones(N, np.int64), -np.ones(M, np.int64)
    gt0[src], gt1[dst] = dst, src
    m0, m1 = -np.ones(N, np.int64), -np.ones(M, np.int64)
    found = rs.permutation(n_gt)[:int(round(frac_found * n_gt))]
    m0[src[found]] = dst[found]
    # mismatches are near misses - a frame-1 keypoint without ground truth, 0.3 to 1.5 m from where the right one would be - so that
    # the one-step pose (no outlier rejection in the reference) survives them and the inlier test has both outcomes
    wrong = src[found[:int(round(frac_wrong * len(found)))]]
    rest = np.setdiff1d(np.arange(N), src)
    spur = rest[rs.permutation(len(rest))[:int(round(frac_spurious * len(rest)))]]
    miss = np.concatenate([wrong, spur])
    free = np.setdiff1d(np.arange(M), dst)
    assert len(miss) <= len(free)
    tgt = free[rs.permutation(len(free))[:len(miss)]]
    off = rs.standard_normal((len(miss), 3))
    off *= (rs.uniform(0.3, 1.5, (len(miss), 1)) / np.linalg.norm(off, axis=1, keepdims=True))
    k1[tgt] = ((Ti[:3, :3] @ k0[miss].astype(np.float64).T).T + Ti[:3, 3] + off).astype(np.float32)
    m0[miss] = tgt
    for i in np.nonzero(m0 > -1)[0]:
        m1[m0[i]] = i
    if dustbin:                          # the loss rewrites -1 to the dustbin index in place (mdgat.py:519-520): mix both spellings
        un0, un1 = np.nonzero(gt0 == -1)[0], np.nonzero(gt1 == -1)[0]
        gt0[un0[::2]] = M
        gt1[un1[::2]] = N
    return dict(kpts0=k0, kpts1=k1, matches0=m0, matches1=m1, gt0=gt0, gt1=gt1, T_gt=T_gt,
                mscores0=rs.uniform(0, 1, N) * (m0 > -1), scores0=rs.uniform(0, 1, N))


def stack(pairs):
    return {k: np.stack([p[k] for p in pairs]) for k in pairs[0]}


def far_pose(rs):
    """A ground-truth pose 50 m and a quarter turn away: whatever rotation a degenerate match set yields, it fails both tests."""
    T = np.eye(4)
    T[:3, :3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = (50.0, 0.0, 0.0)
    return T


def three_matches(rs, N):
    """Exactly three predicted matches (too_few_matches), on coinciding points near the origin under far_pose: the rank-deficient
    pose is the SVD routine's choice, but every choice is more than 2 m and 5 degrees off (|t_gt| - 2 |centroid| > 40 m; trace of
    R^T R_gt <= 1), so test_registration_metric.py - which has no such rule - books the pair as a failure either way."""
    p = make_pair(rs, N, N, T_gt=far_pose(rs))
    keep = np.nonzero((p['matches0'] > -1) & (p['matches0'] == p['gt0']))[0][:3]
    m0 = -np.ones(N, np.int64)
    m0[keep] = p['matches0'][keep]
    p['kpts0'][keep] = (rs.uniform(-1, 1, (3, 3))).astype(np.float32)
    p['kpts1'][m0[keep]] = p['kpts0'][keep]
    m1 = -np.ones(N, np.int64)
    m1[m0[keep]] = keep
    p['matches0'], p['matches1'] = m0, m1
    return p


def groups():
    rs = np.random.RandomState(20261017)
    out = {}
    out['rand17'] = stack([make_pair(rs, 17, 17) for _ in range(3)])
    out['n48m64'] = stack([make_pair(rs, 48, 64, dustbin=True) for _ in range(2)])
    out['n300m500'] = stack([make_pair(rs, 300, 500) for _ in range(2)])
    N = 33
    p = make_pair(rs, N, N)
    p['matches0'][:], p['matches1'][:] = -1, -1
    out['rule_none'] = stack([p])
    out['rule_three'] = stack([three_matches(rs, N)])
    p = make_pair(rs, N, N, frac_gt=3 / N, frac_found=1.0, frac_wrong=0.0, frac_spurious=0.3)
    assert (p['gt0'] > -1).sum() == 3
    out['rule_banned'] = stack([p])
    p = make_pair(rs, N, N)
    p['gt0'][:], p['gt1'][:] = -1, -1
    out['rule_allneg'] = stack([p])
    p = make_pair(rs, N, N, frac_found=1.0, frac_wrong=0.0, frac_spurious=0.0)
    assert np.array_equal(p['matches0'], p['gt0'])
    out['rule_perfect'] = stack([p])
    # the meter's batch: three ordinary pairs, one banned, one with three matches, one whose pose fails (ground truth 50 m away)
    N = 40
    bad_pose = make_pair(rs, N, N)
    bad_pose['T_gt'] = far_pose(rs)
    banned = make_pair(rs, N, N, frac_gt=3 / N, frac_spurious=0.3)
    out['meter6'] = stack([make_pair(rs, N, N), banned, make_pair(rs, N, N), three_matches(rs, N), bad_pose, make_pair(rs, N, N)])
    return out


def main():
    _, UT = import_reference_aux()
    prog_test, prog_reg = loop_program('test.py'), loop_program('test_registration_metric.py')
    out = {'groups': np.array(list(groups()))}
    for name, g in groups().items():
        B = g['matches0'].shape[0]
        for k, v in g.items():
            out[f'{name}_{k}'] = v
        pair_test = np.full((B, len(TEST_PY_VARS) + 2), np.nan)
        pair_reg = np.full((B, len(REG_VARS) + 4), np.nan)
        for b in range(B):
            ns = run(prog_test, UT, [EMPTY, as_pred(g, [b])])
            # (tm / fm: test.py:337-338 reuse the names for the means; the pair's values are the sums they were assigned from, :284-285)
            pair_vars = {v: float(ns[v]) for v in TEST_PY_VARS if v in ns}
            for v, src in (('tm', 'true_positive'), ('fm', 'false_positive')):
                pair_vars.pop(v, None)
                if src in ns:
                    pair_vars[v] = float(np.sum(ns[src]))
            pair_test[b] = [pair_vars.get(v, np.nan) for v in TEST_PY_VARS] + [ns['fail'], ns['baned_data']]
            if (g['matches0'][b] > -1).sum() == 0:
                continue             # no match at all: calculate_error2 has no guard and takes the SVD of a NaN matrix
            ns = run(prog_reg, UT, [EMPTY, as_pred(g, [b])])
            banned = ns['baned_data'] == 1
            pair_reg[b] = [np.nan if banned else float(ns[v]) for v in REG_VARS] + \
                          [ns['inlier_a'].sum, np.nan if banned else float(ns['false_positive'].sum()), ns['RR'].sum, ns['baned_data']]
        out[f'{name}_pair_test_py'], out[f'{name}_pair_registration'] = pair_test, pair_reg
        ns = run(prog_test, UT, [EMPTY, as_pred(g)])
        out[f'{name}_means_test_py'] = np.array([float(ns[v]) for v in TEST_PY_MEANS] + [ns['fail'], ns['baned_data'], ns['i']], dtype=np.float64)
        if all((g['matches0'][b] > -1).sum() > 0 for b in range(B)):
            ns = run(prog_reg, UT, [EMPTY, as_pred(g)])
            out[f'{name}_means_registration'] = np.array([float(ns[m].avg) for m in REG_METERS] + [float(ns['F1']), ns['baned_data']])
        print(name, 'test.py fail', ns['baned_data'], out[f'{name}_means_test_py'][-3:], pair_test[:, [1, 12]].tolist())
    out['test_py_vars'], out['test_py_means'] = np.array(TEST_PY_VARS + ('fail', 'baned_data')), np.array(TEST_PY_MEANS + ('fail', 'baned_data', 'i'))
    out['registration_vars'] = np.array(REG_VARS + ('inlier', 'false_positive', 'RR', 'baned_data'))
    out['registration_means'] = np.array(REG_METERS + ('F1', 'baned_data'))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
