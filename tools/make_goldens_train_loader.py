#!/usr/bin/env python3
"""Generate tests/golden/train_loader.npz by running the REAL reference loader in TRAIN mode: ``SparseDataset.__getitem__`` with
``ensure_kpts_num=True`` (train.py's default, which governs the validation set too; load_data.py:180-211: the saliency filter, the
truncation, the prepend loop that pads to ``max_keypoints``) and a small ``max_keypoints``, so that every branch of it is met by frames
of a few dozen records.

Like tools/make_goldens_aux.py it runs only where the reference exists (``MDGAT_REFERENCE``, default /root/reference), imports
``load_data.py`` UNMODIFIED behind an empty placeholder module named ``open3d`` (imported there, never called on this path) and writes
synthetic keypoint files in the KITTI layout (N x 37 float32) to a temporary ``keypoints_path``; poses, calibration and the pair list
are the reference's real files of sequence 10.  The fixture holds the records, the poses, the calibration and the loader's outputs
per item (the six inputs, gt_matches0/1, rep, T_gt) under both ``mutual_check`` settings.

Saliencies lie around the loader's threshold of 10: kept ones in (10, 20] with one at the float32 successor of 10, dropped ones in
[0, 10] with some at exactly 10.0, one NaN; a dropped record with an all-zero FPFH row and a dropped one with NaN coordinates show that
dropped records are not looked at.  Before the loader is called every frame is checked to keep at least one record: on a frame that
keeps none the reference's loop never ends."""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get('MDGAT_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden')
SEQ = 10

# set -> (max_keypoints, dataset items, frame -> (records, kept)); the pair list of sequence 10 starts (1, 30) (2, 20) (3, 28) (4, 24)
# (5, 31) (6, 20): items 1 and 5 share frame 20
SETS = {
    't40': (40, [0, 1, 2, 3, 5], {
        1: (70, 55),       # truncation
        30: (50, 40),      # exact fit
        2: (40, 29),       # one pad step (T/2 <= v < T)
        20: (20, 7),       # several pad steps: 7 -> 14 -> 28 -> 40; shared by items 1 and 5
        3: (12, 1),        # many pad steps: 1 -> 2 -> 4 -> .. -> 32 -> 40
        28: (150, 80),     # more than two waves of records, truncation
        4: (55, 41),       # truncation by one
        24: (50, 39),      # a pad step of one row
        6: (30, 20),       # v == T/2: one step doubles it
    }),
    't64': (64, [0, 1], {
        1: (80, 64),      # exact fit at a wave's width
        30: (70, 63),
        2: (45, 33),
        20: (90, 70),
    }),
}


def import_reference_loader():
    sys.modules.setdefault('open3d', types.ModuleType('open3d'))     # placeholder: never called
    sys.path.insert(0, REF)
    import load_data as LD            # noqa: E402  the reference, unmodified
    return LD


def saliency(rs, n, v):
    """n saliencies of which exactly v exceed 10, in a random arrangement, with the edge values"""
    s = np.empty(n, dtype=np.float32)
    keep = np.zeros(n, dtype=bool)
    keep[rs.permutation(n)[:v]] = True
    s[keep] = rs.uniform(10.01, 20.0, v)
    s[~keep] = rs.uniform(0.0, 10.0, n - v)
    kept, dropped = np.nonzero(keep)[0], np.nonzero(~keep)[0]
    if v >= 3:
        s[kept[v // 2]] = np.nextafter(np.float32(10.0), np.float32(np.inf))
    s[dropped[::5]] = 10.0                       # exactly the threshold: dropped
    assert int((s > 10).sum()) == v
    return s, keep, dropped


def make_records(rs, frames):
    """frame -> [n, 37] float32 records; kept keypoints of a pair's frames are re-observations of one another (noise straddling the 0.5 m
    threshold, relate below) so that the ground-truth matcher has something to find."""
    rec, keeps = {}, {}
    for idx, (n, v) in frames.items():
        r = np.zeros((n, 37), dtype=np.float32)
        r[:, :3] = rs.uniform(-30, 30, (n, 3)) * np.array([1.0, 1.0, 0.1])
        r[:, 3], keep, dropped = saliency(rs, n, v)
        r[:, 4:] = rs.uniform(0.0, 200.0, (n, 33))        # un-normalised FPFH histogram
        rec[idx], keeps[idx] = r, (keep, dropped)
    return rec, keeps


def relate(rs, rec, keeps, W, T, i0, i1):
    """overwrite some kept keypoints of frame i1 with noisy re-observations of kept keypoints of frame i0 (of the first T kept: the ones
    that survive the truncation)"""
    k0, k1 = np.nonzero(keeps[i0][0])[0][:T], np.nonzero(keeps[i1][0])[0][:T]
    nc = max(1, min(len(k0), len(k1)) // 2)
    src, dst = rs.permutation(k0)[:nc], rs.permutation(k1)[:nc]
    scale = rs.uniform(0.0, 0.45, (nc, 1))
    scale[0] = 0.05           # the first one is found whatever is drawn: a frame that keeps one record is 40 copies of a match
    w = (W[i0][:3, :3] @ rec[i0][src, :3].astype(np.float64).T).T + W[i0][:3, 3] + scale * rs.standard_normal((nc, 3))
    Wi = np.linalg.inv(W[i1])
    rec[i1][dst, :3] = (Wi[:3, :3] @ w.T).T + Wi[:3, 3]


def main():
    LD = import_reference_loader()
    txt = os.path.join(REF, 'KITTI', 'preprocess-random-full')

    def make_opt(path, T, mutual):
        return argparse.Namespace(train_path=os.path.join(REF, 'KITTI'), keypoints='USIP', keypoints_path=path, descriptor='FPFH',
                                  max_keypoints=T, threshold=0.5, ensure_kpts_num=True, mutual_check=mutual, memory_is_enough=False,
                                  txt_path=txt)

    out = {'sets': np.array(sorted(SETS)), 'threshold': np.array(0.5), 'min_saliency': np.array(10.0, dtype=np.float32)}
    for s, name in enumerate(sorted(SETS)):
        T, items, frames = SETS[name]
        rs = np.random.RandomState(20261019 + s)
        tmp = tempfile.mkdtemp(prefix='mdgat_train_kpts_')
        os.makedirs(os.path.join(tmp, '%02d' % SEQ))
        probe = LD.SparseDataset(make_opt(tmp, T, False), 'test')     # parses the real pose / calibration files
        pose, Tcv = probe.pose['%02d' % SEQ], probe.calib['%02d' % SEQ]
        pairs = [(probe.dataset[j]['anc_idx'], probe.dataset[j]['pos_idx']) for j in items]
        assert set(frames) == {i for p in pairs for i in p}, pairs
        W = {i: pose[i] @ Tcv for i in frames}
        rec, keeps = make_records(rs, frames)
        done = set()
        for i0, i1 in pairs:
            if i1 not in done:
                relate(rs, rec, keeps, W, T, i0, i1)
            else:
                relate(rs, rec, keeps, W, T, i1, i0)      # a shared frame stays as its first pair left it
            done.update((i0, i1))
        # what a dropped record holds is not looked at
        big = max(frames, key=lambda i: frames[i][0] - frames[i][1])
        dropped = keeps[big][1]
        rec[big][dropped[1], 3] = np.nan                       # NaN saliency: dropped (NaN > 10 is false)
        rec[big][dropped[2], 4:] = 0.0                         # an all-zero FPFH row, saliency below 10
        rec[big][dropped[3], :3] = np.nan                      # NaN coordinates, saliency below 10
        for i, (n, v) in frames.items():
            with np.errstate(invalid='ignore'):
                kept = int((rec[i][:, 3] > 10).sum())
            assert kept == v >= 1 and rec[i].shape == (n, 37), (i, kept, v)      # v == 0: the loader would never return
            rec[i].tofile(os.path.join(tmp, '%02d' % SEQ, '%06d.bin' % i))
        order = sorted(frames)
        out[f'{name}_max_keypoints'] = np.array(T)
        out[f'{name}_frames'] = np.array(order)
        out[f'{name}_pairs'] = np.array(pairs)
        for i in order:
            out[f'{name}_rec{i}'] = rec[i]
            out[f'{name}_pose{i}'] = pose[i]
        for mutual in (False, True):
            ds = LD.SparseDataset(make_opt(tmp, T, mutual), 'test')
            for j, item in enumerate(items):
                d = ds[item]
                tag = f'{name}_item{j}_' + ('mutual_' if mutual else '')
                assert d['idx0'] == pairs[j][0]
                for key in ('keypoints0', 'keypoints1', 'descriptors0', 'descriptors1', 'scores0', 'scores1', 'T_gt'):
                    assert d[key].dtype == torch.double
                    if key != 'T_gt':
                        assert d[key].shape[0] == T
                        # the fixture stores what float32 holds: every input is a widened float32
                        assert np.array_equal(d[key].numpy(), d[key].numpy().astype(np.float32).astype(np.float64)), key
                    if mutual and key != 'T_gt':
                        assert np.array_equal(d[key].numpy(), out[f'{name}_item{j}_{key}'])
                        continue                # the inputs do not depend on mutual_check: stored once
                    out[tag + key] = d[key].numpy().astype(np.float32) if key != 'T_gt' else d[key].numpy()
                out[tag + 'gt_matches0'] = np.asarray(d['gt_matches0'])
                out[tag + 'gt_matches1'] = np.asarray(d['gt_matches1'])
                out[tag + 'rep'] = np.array(d['rep'])
                print(f'{name} item {j} {pairs[j]} mutual={mutual}: v = {frames[pairs[j][0]][1]} x {frames[pairs[j][1]][1]} rep={d["rep"]} '
                      f'gt0>=0: {(np.asarray(d["gt_matches0"]) >= 0).sum()} gt1>=0: {(np.asarray(d["gt_matches1"]) >= 0).sum()}')
    out['T_cam0_velo'] = Tcv
    path = os.path.join(OUT, 'train_loader.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
