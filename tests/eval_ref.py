"""numpy restatement of what the reference's two evaluation scripts do with the matcher's output, statement by statement
(comprehensions included), so that it is visibly the same computation: the per-pair block of test.py:212-311, the one of
test_registration_metric.py:213-269, the means both print at the end, and the three functions of utils/utils_test.py they call.

Pinned by tests/test_eval_ref.py: the pose functions against the reference's recorded outputs (tests/golden/aux_pose.npz), the
blocks and the means against values recorded from the scripts' own loop bodies (tests/golden/eval_cases.npz, written by
tools/make_goldens_eval.py).  The GPU tests compare csrc/eval_metrics.hip and ops.EvalMeter with this file."""
import warnings

import numpy as np

try:
    import torch
except ImportError:          # the restatement itself needs numpy only
    torch = None


def _np(t):
    """`.cpu().detach().numpy()` of the scripts (one copy per tensor when it lives on a device)."""
    if torch is not None and isinstance(t, torch.Tensor):
        return t.cpu().detach().numpy()
    return np.asarray(t)


# ------------------------------------------------------------------------------------------ utils/utils_test.py
class AverageMeter:
    """utils_test.py:6-25."""

    def __init__(self):
        self.val, self.avg, self.sum, self.sq_sum, self.count = 0, 0, 0.0, 0.0, 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count
        self.sq_sum += val ** 2 * n
        self.var = self.sq_sum / self.count - self.avg ** 2


def solve_icp(P, Q):
    """utils_test.py:73-110."""
    up = P.mean(axis=0)
    uq = Q.mean(axis=0)
    P_centered = P - up
    Q_centered = Q - uq
    U, s, V = np.linalg.svd(np.dot(Q_centered.T, P_centered), full_matrices=True, compute_uv=True)
    R = np.dot(U, V)
    t = uq - np.dot(R, up)
    T = np.zeros((4, 4))
    T[0:3, 0:3] = R
    T[0:3, 3] = t
    T[3, 3] = 1.0
    return T


def calculate_error(mkpts0, mkpts1, T_gt, inlier_dist=1):
    """utils_test.py:41-71 (T_gt is pred['T_gt'][b] there; the torch einsums are matrix products)."""
    T = solve_icp(mkpts1, mkpts0)
    T_gt = np.asarray(_np(T_gt), dtype=np.float64)
    kp0_np = np.array([(kp[0], kp[1], kp[2], 1) for kp in mkpts0], dtype=np.float64)
    kp1_np = np.array([(kp[0], kp[1], kp[2], 1) for kp in mkpts1], dtype=np.float64)
    mkpts1w = (T @ kp1_np.T).T
    inlier = np.linalg.norm(mkpts1w[:, :3] - kp0_np[:, :3], axis=1) < inlier_dist
    inlier = inlier.sum()
    inlier_ratio = inlier.item() / len(kp0_np)
    T_error = np.linalg.inv(T) @ T_gt
    trans_error = np.linalg.norm(T_error[:3, 3])
    f_theta = (T_error[0, 0] + T_error[1, 1] + T_error[2, 2] - 1) * 0.5
    rot_error = np.arccos(f_theta)
    return T, inlier, inlier_ratio, trans_error, rot_error


def calculate_error2(mkpts0, mkpts1, T_gt):
    """utils_test.py:27-39."""
    T = solve_icp(mkpts1, mkpts0)
    T_gt = np.asarray(_np(T_gt), dtype=np.float64)
    T_error = np.linalg.inv(T) @ T_gt
    rte = np.linalg.norm(T_error[:3, 3])
    f_theta = (T_error[0, 0] + T_error[1, 1] + T_error[2, 2] - 1) / 2
    rre = np.arccos(f_theta)
    return T, rte, rre


# ------------------------------------------------------------------------------------------ test.py
class TestPyMeter:
    """The lists and counters of test.py:183-188 and the means of :326-342."""
    __test__ = False
    LISTS = ('precision', 'accuracy', 'recall', 'trans_error', 'rot_error', 'repeatibilty', 'inlier', 'inlier_ratio', 'fp_rate',
             'tp_rate', 'tp_rate2', 'tm', 'fm')

    def __init__(self):
        for name in self.LISTS:
            setattr(self, name + '_array', [])
        self.fail = 0
        self.baned_data = 0
        self.i = -1                   # enumerate(test_loader)'s index

    def means(self):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            out = {name: np.mean(getattr(self, name + '_array')) for name in self.LISTS}
        return out


def test_py_pair(pred, b, meter, calculate_pose=True):
    """test.py:212-311 for pair b of a batch, appending to `meter` as the script does.  Returns the pair's local values (those the
    script had computed when it left the block) for inspection."""
    out = {}
    kpts0, kpts1 = _np(pred['keypoints0'][b]), _np(pred['keypoints1'][b])
    matches, matches1, conf = _np(pred['matches0'][b]), _np(pred['matches1'][b]), _np(pred['matching_scores0'][b])
    valid = matches > -1
    mkpts0 = kpts0[valid]
    mkpts1 = kpts1[matches[valid]]
    mconf = conf[valid]                                                                  # noqa: F841 (visualisation only)

    matches_gt, matches_gt1 = _np(pred['gt_matches0'][b]).copy(), _np(pred['gt_matches1'][b]).copy()   # (the script rewrites in place)
    matches_gt[matches_gt == len(matches_gt1)] = -1
    matches_gt1[matches_gt1 == len(matches_gt)] = -1
    valid_gt = matches_gt > -1

    valid_num = np.sum(valid_gt)
    all_num = len(valid_gt)
    repeatibilty = valid_num / all_num
    meter.repeatibilty_array.append(repeatibilty)
    out['repeatibilty'] = repeatibilty

    if valid_gt.sum() < len(matches_gt) * 0.1:
        meter.baned_data += 1
        meter.fail += 1
        out['banned'] = True
        return out

    if len(mkpts0) < 4:
        meter.fail += 1
        out['too_few'] = True
        return out

    true_positive = [(matches[i] == matches_gt[i]) and (valid[i]) for i in range(len(kpts0))]
    true_negativate = [(matches[i] == matches_gt[i]) and not (valid[i]) for i in range(len(kpts0))]
    false_positive = [valid[i] and (matches_gt[i] == -1) for i in range(len(kpts0))]
    with np.errstate(invalid='ignore', divide='ignore'):
        precision = np.sum(true_positive) / np.sum(valid) if np.sum(valid) > 0 else 0
        recall = np.sum(true_positive) / np.sum(valid_gt) if np.sum(valid) > 0 else 0
        tm = np.sum(true_positive)
        fm = np.sum(false_positive)
        matching_score = np.sum(true_positive) / len(kpts0) if len(kpts0) > 0 else 0
        accuracy = (np.sum(true_positive) + np.sum(true_negativate)) / len(matches_gt)
        fp_rate = np.sum(false_positive) / np.sum(matches_gt == -1)
        tp_rate = np.sum([valid[i] and (matches_gt[i] > -1) for i in range(len(kpts0))]) / np.sum(matches_gt > -1)
        tp_rate2 = np.sum(true_positive) / np.sum(matches_gt > -1)
    out.update(precision=precision, recall=recall, tm=tm, fm=fm, matching_score=matching_score, accuracy=accuracy, fp_rate=fp_rate,
               tp_rate=tp_rate, tp_rate2=tp_rate2, true_negative=np.sum(true_negativate))

    if calculate_pose:
        with np.errstate(invalid='ignore'):
            T, inlier, inlier_ratio, trans_error, rot_error = calculate_error(mkpts0, mkpts1, pred['T_gt'][b])
        out.update(T=T, inlier=inlier, inlier_ratio=inlier_ratio, trans_error=trans_error, rot_error=rot_error)
        if trans_error > 2 or rot_error > 5 or np.isnan(trans_error) or np.isnan(rot_error):
            meter.fail += 1
            out['registration_fail'] = True
        else:
            meter.precision_array.append(precision)
            meter.accuracy_array.append(accuracy)
            meter.recall_array.append(recall)
            meter.trans_error_array.append(trans_error)
            meter.rot_error_array.append(rot_error)
            meter.inlier_array.append(inlier)
            meter.inlier_ratio_array.append(inlier_ratio)
            meter.fp_rate_array.append(fp_rate)
            meter.tp_rate_array.append(tp_rate)
            meter.tp_rate2_array.append(tp_rate2)
            meter.tm_array.append(tm)
            meter.fm_array.append(fm)
    return out


def test_py_loop(loader, calculate_pose=True):
    """test.py:190-342 without the forward: `loader` yields the merged pred dicts.  Returns (meter, means, fail / i, baned_data / i)."""
    meter = TestPyMeter()
    for i, pred in enumerate(loader):
        meter.i = i
        for b in range(len(pred['idx0'])):
            test_py_pair(pred, b, meter, calculate_pose)
    with np.errstate(invalid='ignore', divide='ignore'):
        i = np.float64(meter.i)
        return meter, meter.means(), meter.fail / i, meter.baned_data / i


test_py_pair.__test__ = False
test_py_loop.__test__ = False


# ------------------------------------------------------------------------------------------ test_registration_metric.py
class RegistrationMeter:
    """test_registration_metric.py:185-189 and what :282-286 print."""
    NAMES = ('rep', 'rre', 'rte', 'inlier', 'inlier_ratio', 'recall', 'tp_rate', 'fp_rate', 'RR')

    def __init__(self):
        for name in self.NAMES:
            setattr(self, name if name == 'RR' else name + '_a', AverageMeter())
        self.baned_data = 0

    def get(self, name):
        return getattr(self, name if name == 'RR' else name + '_a')

    def report(self):
        out = {name: self.get(name).avg for name in self.NAMES}
        if self.inlier_ratio_a.count == 0:       # every pair banned: both averages are still the integer 0 and :282 raises ZeroDivisionError
            out['F1'] = np.nan
            return out
        with np.errstate(invalid='ignore', divide='ignore'):
            out['F1'] = 2 * self.inlier_ratio_a.avg * self.recall_a.avg / (self.inlier_ratio_a.avg + self.recall_a.avg)
        return out


def registration_pair(pred, b, meter, calculate_pose=True):
    """test_registration_metric.py:213-269 for pair b of a batch."""
    out = {}
    kpts0, kpts1 = _np(pred['keypoints0'][b]), _np(pred['keypoints1'][b])
    matches, matches1, conf = _np(pred['matches0'][b]), _np(pred['matches1'][b]), _np(pred['matching_scores0'][b])
    valid = matches > -1

    mkpts0 = kpts0[valid]
    mkpts1 = kpts1[matches[valid]]
    mconf = conf[valid]                                                                  # noqa: F841

    matches_gt, matches_gt1 = _np(pred['gt_matches0'][b]).copy(), _np(pred['gt_matches1'][b]).copy()
    matches_gt[matches_gt == len(matches_gt1)] = -1
    matches_gt1[matches_gt1 == len(matches_gt)] = -1
    valid_gt = matches_gt > -1

    if valid_gt.sum() < len(matches_gt) * 0.1:
        meter.baned_data += 1
        out['banned'] = True
        return out

    repeatibilty = np.sum(valid_gt) / len(valid_gt)

    true_positive = (matches > -1) * (matches == matches_gt)
    false_positive = (matches > -1) * ((matches == matches_gt) == False)                 # noqa: E712
    true_negativate = (matches == -1) * (matches_gt == -1)
    false_negativate = (matches == -1) * (matches_gt > -1)

    with np.errstate(invalid='ignore', divide='ignore'):
        precision_inlier_ratio = np.sum(true_positive) / np.sum(valid) if np.sum(valid) > 0 else 0
        recall = np.sum(true_positive) / np.sum(valid_gt) if np.sum(valid) > 0 else 0
        fp_rate = np.sum(false_positive) / (np.sum(false_positive) + np.sum(true_negativate))
        tp_rate = np.sum(true_positive) / (np.sum(true_positive) + np.sum(false_negativate))

    meter.rep_a.update(repeatibilty), meter.fp_rate_a.update(fp_rate), meter.tp_rate_a.update(tp_rate)
    meter.recall_a.update(recall), meter.inlier_ratio_a.update(precision_inlier_ratio), meter.inlier_a.update(np.sum(true_positive))
    out.update(repeatibilty=repeatibilty, precision_inlier_ratio=precision_inlier_ratio, recall=recall, fp_rate=fp_rate, tp_rate=tp_rate,
               inlier=np.sum(true_positive), false_positive=np.sum(false_positive), false_negative=np.sum(false_negativate))

    if calculate_pose:
        with np.errstate(invalid='ignore'):
            T, rte, rre = calculate_error2(mkpts0, mkpts1, pred['T_gt'][b])
        out.update(T=T, rte=rte, rre=rre)
        if rte < 2:
            meter.rte_a.update(rte)
        if not np.isnan(rre) and rre < np.pi / 180 * 5:
            meter.rre_a.update(rre)
        if rte < 2 and not np.isnan(rre) and rre < np.pi / 180 * 5:
            meter.RR.update(1)
        else:
            meter.RR.update(0)
    return out


def registration_loop(loader, calculate_pose=True):
    """test_registration_metric.py:191-286 without the forward.  Returns (meter, report)."""
    meter = RegistrationMeter()
    for i, pred in enumerate(loader):
        for b in range(len(pred['idx0'])):
            registration_pair(pred, b, meter, calculate_pose)
    return meter, meter.report()


# ------------------------------------------------------------------------------------------ the kernel's row, from the restatement
def expected_row(pred, b, columns, status_bits):
    """What csrc/eval_metrics.hip writes for pair b: the statements of the two blocks above once more, without their early exits
    (banned, too few matches) - the kernel fills every column and reports the rules as status bits - and with the literal
    comprehensions, so the counts and ratios of a banned or too-few pair are those the scripts' own expressions give.
    tests/test_eval_ref.py checks this function against the two blocks on every recorded case.  `columns` is ops.EvalColumns (a
    name -> index mapping), `status_bits` the dict of its bits.  Returns (row [len(columns)] float64, pose_defined): with fewer than
    4 matches the pose depends on the SVD routine's choice of a null vector (tests/test_gpu_postproc.py), and without any match
    there is none (NaN)."""
    N = len(_np(pred['matches0'][b]))
    row = np.full(len(columns), np.nan)
    matches = _np(pred['matches0'][b])
    matches_gt = _np(pred['gt_matches0'][b]).copy()
    matches_gt[matches_gt == len(_np(pred['gt_matches1'][b]))] = -1
    valid, valid_gt = matches > -1, matches_gt > -1
    n_valid = int(np.sum(valid))
    status = 0
    if valid_gt.sum() < N * 0.1:
        status |= status_bits['BANNED']
    if n_valid < 4:
        status |= status_bits['TOO_FEW_MATCHES']

    # the inline block of test.py:277-290, the literal comprehensions (run whatever the rules say)
    kpts0 = _np(pred['keypoints0'][b])
    true_positive = [(matches[i] == matches_gt[i]) and (valid[i]) for i in range(len(kpts0))]
    true_negativate = [(matches[i] == matches_gt[i]) and not (valid[i]) for i in range(len(kpts0))]
    false_positive = [valid[i] and (matches_gt[i] == -1) for i in range(len(kpts0))]
    with np.errstate(invalid='ignore', divide='ignore'):
        row[columns['n_valid']] = np.sum(valid)
        row[columns['n_valid_gt']] = np.sum(valid_gt)
        row[columns['n_gt_negative']] = np.sum(matches_gt == -1)
        row[columns['true_positive']] = np.sum(true_positive)
        row[columns['true_negative']] = np.sum(true_negativate)
        row[columns['false_positive']] = np.sum(false_positive)
        row[columns['n_valid_and_gt_positive']] = np.sum([valid[i] and (matches_gt[i] > -1) for i in range(len(kpts0))])
        row[columns['repeatability']] = np.sum(valid_gt) / len(valid_gt)
        row[columns['precision']] = np.sum(true_positive) / np.sum(valid) if np.sum(valid) > 0 else 0
        row[columns['recall']] = np.sum(true_positive) / np.sum(valid_gt) if np.sum(valid) > 0 else 0
        row[columns['matching_score']] = np.sum(true_positive) / len(kpts0) if len(kpts0) > 0 else 0
        row[columns['accuracy']] = (np.sum(true_positive) + np.sum(true_negativate)) / len(matches_gt)
        row[columns['fp_rate']] = np.sum(false_positive) / np.sum(matches_gt == -1)
        row[columns['tp_rate']] = row[columns['n_valid_and_gt_positive']] / np.sum(matches_gt > -1)
        row[columns['tp_rate2']] = np.sum(true_positive) / np.sum(matches_gt > -1)
        # test_registration_metric.py:238-248
        fp_reg = (matches > -1) * ((matches == matches_gt) == False)                     # noqa: E712
        tn_reg = (matches == -1) * (matches_gt == -1)
        fn_reg = (matches == -1) * (matches_gt > -1)
        row[columns['false_positive_reg']] = np.sum(fp_reg)
        row[columns['false_negative']] = np.sum(fn_reg)
        row[columns['fp_rate_reg']] = np.sum(fp_reg) / (np.sum(fp_reg) + np.sum(tn_reg))
        row[columns['tp_rate_reg']] = np.sum(true_positive) / (np.sum(true_positive) + np.sum(fn_reg))

    trans_error = rot_error = np.nan
    row[columns['inliers']] = 0
    if n_valid > 0:
        mkpts0, mkpts1 = kpts0[valid], _np(pred['keypoints1'][b])[matches[valid]]
        with np.errstate(invalid='ignore'):
            if pred.get('T_gt') is not None:
                _, inlier, inlier_ratio, trans_error, rot_error = calculate_error(mkpts0, mkpts1, pred['T_gt'][b])
            else:
                _, inlier, inlier_ratio, _, _ = calculate_error(mkpts0, mkpts1, np.eye(4))
        row[columns['inliers']], row[columns['inlier_ratio']] = inlier, inlier_ratio
    row[columns['trans_error']], row[columns['rot_error']] = trans_error, rot_error
    if trans_error > 2 or rot_error > 5 or np.isnan(trans_error) or np.isnan(rot_error):
        status |= status_bits['REGISTRATION_FAIL']
    if trans_error < 2:
        status |= status_bits['RTE_OK']
    if not np.isnan(rot_error) and rot_error < np.pi / 180 * 5:
        status |= status_bits['RRE_OK']
    row[columns['status']] = status
    return row, n_valid >= 4


# ------------------------------------------------------------------------------------------ the recorded cases
GROUP_KEYS = ('kpts0', 'kpts1', 'matches0', 'matches1', 'gt0', 'gt1', 'T_gt', 'mscores0', 'scores0')


def load_group(golden, name):
    """One group of tests/golden/eval_cases.npz (`golden`: the opened file): the inputs as arrays [B, ...] and the recorded tables
    as dicts name -> column."""
    g = {k: golden[f'{name}_{k}'] for k in GROUP_KEYS}
    rec = {
        'pair_test_py': dict(zip(golden['test_py_vars'], golden[f'{name}_pair_test_py'].T)),
        'pair_registration': dict(zip(golden['registration_vars'], golden[f'{name}_pair_registration'].T)),
        'means_test_py': dict(zip(golden['test_py_means'], golden[f'{name}_means_test_py'])),
    }
    if f'{name}_means_registration' in golden:
        rec['means_registration'] = dict(zip(golden['registration_means'], golden[f'{name}_means_registration']))
    return g, rec


def as_pred(g, pairs=None):
    """A group as the merged `pred` dict the scripts index (float64 keypoints, as net.double() leaves them: test.py:193)."""
    sel = slice(None) if pairs is None else list(pairs)
    pred = {'keypoints0': g['kpts0'][sel].astype(np.float64), 'keypoints1': g['kpts1'][sel].astype(np.float64),
            'matches0': g['matches0'][sel], 'matches1': g['matches1'][sel], 'matching_scores0': g['mscores0'][sel],
            'scores0': g['scores0'][sel], 'gt_matches0': g['gt0'][sel], 'gt_matches1': g['gt1'][sel], 'T_gt': g['T_gt'][sel]}
    pred['idx0'] = list(range(len(pred['matches0'])))
    return pred


EMPTY_BATCH = {'idx0': []}          # the recorded runs start with an empty batch, so that the scripts' `fail / i` divides by 1
