"""A host restatement of the loader's train-mode assembly (SparseDataset.__getitem__ with ensure_kpts_num), written from its rule, not
from its code: filter by saliency, truncate or pad to T by a closed-form slot map, normalise the FPFH rows in float32, widen.  The
yardstick of ops.assemble_frames_train at shapes tests/golden/train_loader.npz lacks; tests/test_train_frames_ref.py pins it against that
golden and against a literal run of the loader's prepend loop."""
import os

import numpy as np


def slot_map(v, T):
    """Which of the v kept rows stands in each of the T slots.  v >= T: the first T.  Else step k puts the first c_k = min(T - L_k, L_k) rows
    of the L_k there are in front of them (L_0 = v); walking the steps backwards, a slot behind what step k put in front (j >= c_k) lay
    c_k rows earlier before it."""
    if v < 1 or T < 1:
        raise ValueError(f'slot_map: v={v}, T={T}')
    steps, L = [], v
    while L < T:
        steps.append(min(T - L, L))
        L += steps[-1]
    j = np.arange(T)
    for c in reversed(steps):
        j = np.where(j >= c, j - c, j)
    return j


def prepend_loop(v, T):
    """The same by running the loop on the row numbers."""
    a = np.arange(v)
    if T < len(a):
        return a[:T]
    while T > len(a):
        a = np.concatenate((a[:T - len(a)], a))
    return a


def kept_rows(records, min_saliency=10.0):
    """rows with saliency > min_saliency, a float32 compare (NaN and min_saliency itself are dropped), in their order"""
    s = np.asarray(records, dtype=np.float32)[:, 3]
    with np.errstate(invalid='ignore'):
        return np.nonzero(s > np.float32(min_saliency))[0]


def assemble_frame(records, T, min_saliency=10.0, normalize=True):
    """One frame's [n, 37] float32 records -> dict(keypoints [T, 3], scores [T], descriptors [T, 33] float64, keypoints_f32 [T, 3],
    source [T] int32, salient int).  A frame that keeps no record raises ValueError (the loader's loop never ends)."""
    rec = np.asarray(records, dtype=np.float32)
    kept = kept_rows(rec, min_saliency)
    v = len(kept)
    if v == 0:
        raise ValueError('no record with saliency above min_saliency')
    source = kept[slot_map(v, T)]
    rows = rec[source]
    desc = rows[:, 4:]
    if normalize:
        norm = np.linalg.norm(desc, axis=1).reshape(T, 1)
        with np.errstate(divide='ignore', invalid='ignore'):
            desc = np.multiply(desc, 1 / norm)
    assert desc.dtype == np.float32
    return {'keypoints': rows[:, :3].astype(np.float64), 'scores': rows[:, 3].astype(np.float64), 'descriptors': desc.astype(np.float64),
            'keypoints_f32': rows[:, :3].copy(), 'source': source.astype(np.int32), 'salient': v}


# ---- the reference loader's recorded outputs ----
def load_golden(golden_dir):
    """tests/golden/train_loader.npz (tools/make_goldens_train_loader.py): (the file, set name -> max_keypoints T, its frames' numbers, its
    pairs of frame numbers, the frames' records and poses)"""
    g = np.load(os.path.join(golden_dir, 'train_loader.npz'))
    sets = {}
    for name in g['sets']:
        name = str(name)
        T = int(g[f'{name}_max_keypoints'])
        frames = [int(i) for i in g[f'{name}_frames']]
        sets[name] = {'T': T, 'frames': frames, 'pairs': [tuple(int(i) for i in p) for p in g[f'{name}_pairs']],
                      'rec': {i: g[f'{name}_rec{i}'] for i in frames}, 'pose': {i: g[f'{name}_pose{i}'] for i in frames}}
    return g, sets


def loader_inputs(g, name, j, f):
    """the loader's float64 tensors of frame f of item j (stored as the float32 they hold exactly)"""
    return {k: g[f'{name}_item{j}_{k}{f}'].astype(np.float64) for k in ('keypoints', 'scores', 'descriptors')}
