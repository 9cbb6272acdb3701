"""The inputs of tests/attention_f64_rows.py reach every branch of the fp64 row selects in every search form, and the reference is a fair
judge on every row of them - proved on the CPU with the model of tests/row_select_ref.py, on the fp32 roundings of the reference's own
fp64 logits.  (What the kernels then compute on these inputs: tests/test_gpu_attention_f64_forms.py.)"""
import collections
import functools

import numpy as np
import torch

import attention_f64_rows as R
import row_select_ref as S

MIN_ROWS = 8
MODELLED_ROWS = 72          # of a one-hot unit: rows 0 .. 71 hold every (column, pattern) once; the rows behind repeat them bit for bit


@functools.lru_cache(maxsize=None)
def _analysis():
    """[(case id, form, b, side, head, row, column name | 'dense', c_r | None, model's dict)] for the distinct rows of every case"""
    out = []
    for case in R.CASES:
        nk_max = max(case.N, case.M)
        zq = S.zq_of(case.k, nk_max)
        ref = case.reference()
        for b, side, h, (ql, nq), (kl, nk) in case.units():
            if case.k >= nk:
                continue                # (keep-all inside the dynamic kernel: no search)
            form = S.search_form(nk, nk_max)
            rows32 = ref[b, side][0][h].numpy().astype(np.float32)
            hot = h > 0 and R.one_hot(nk)
            for r in range(min(nq, MODELLED_ROWS)):
                d, _, c = R.pattern(r) if hot else (None, None, None)
                out.append((case.id, form, b, side, h, r, R.COLUMNS[d] if hot else 'dense', c, S.analyse(rows32[r], case.k, zq, form)))
    return out


def _table(key):
    t = collections.Counter()
    for _, form, *_, a in _analysis():
        k = key(a)
        if k is not None:
            t[form, k] += 1
    return t


def _show(t, kinds):
    return '\n'.join(f'{form:9s} ' + '  '.join(f'{kind} {t[form, kind]:5d}' for kind in kinds) for form in S.FORMS)


def test_every_search_form_starts_in_all_three_ways():
    t = _table(lambda a: a['start'] if a['robust'] else None)
    print(_show(t, S.STARTS))
    empty = [(f, s) for f in S.FORMS for s in S.STARTS if t[f, s] < MIN_ROWS]
    assert not empty, f'fewer than {MIN_ROWS} rows (robust against +- 0.05 sd) in {empty}:\n{_show(t, S.STARTS)}'


def test_every_search_form_meets_every_tie_mode():
    t = _table(lambda a: a['tie'])
    print(_show(t, S.TIES))
    empty = [(f, s) for f in S.FORMS for s in S.TIES if t[f, s] < MIN_ROWS]
    assert not empty, f'fewer than {MIN_ROWS} rows in {empty}:\n{_show(t, S.TIES)}'


def test_every_search_form_leaves_the_select_both_ways_and_through_a_narrow_level():
    t = _table(lambda a: a['exit'])
    n = _table(lambda a: 'narrow' if a['narrow'] else None)
    g = _table(lambda a: 'c_gt=0' if a['mode'] and a['c_gt'] == 0 else None)
    for f in S.FORMS:
        assert t[f, 'single'] >= MIN_ROWS and t[f, 'digits'] >= MIN_ROWS and n[f, 'narrow'] >= MIN_ROWS, (f, t, n)
        assert g[f, 'c_gt=0'] >= MIN_ROWS, (f, g)          # a tie group that holds the row maximum


def test_the_reference_is_a_fair_judge_on_every_row():
    """Outside the planted groups the k-th and (k+1)-th fp64 logits of EVERY row differ by more than 1e-12 of the row's largest |logit|;
    rows whose k-th and (k+1)-th are equal are the constant rows and the rows of the dup column, and there they are equal to the bit
    (so are all the copies); |logit| <= 256."""
    for case in R.CASES:
        ref = case.reference()
        for b, side, h, (ql, nq), (kl, nk) in case.units():
            logits = ref[b, side][0][h]
            assert float(logits.abs().max()) <= 256.0, (case.id, b, side, h)
            if case.k >= nk:
                continue
            top = logits.topk(case.k + 1, dim=-1).values
            gap = top[:, case.k - 1] - top[:, case.k]
            close = gap <= 1e-12 * logits.abs().amax(-1)
            hot = h > 0 and R.one_hot(nk)
            for r in np.nonzero(close.numpy())[0]:
                d, _, c = R.pattern(int(r)) if hot else (None, None, None)
                planted = (c == 0.0 or R.COLUMNS[d] == 'dup') if hot else r % R.DENSE_CONST_EVERY == R.DENSE_CONST_AT
                assert planted and float(gap[r]) == 0.0, (case.id, b, side, h, int(r), float(gap[r]))
                row = logits[r]
                tied = row[row == top[r, case.k]]
                bits = set((tied.numpy() + 0.0).view(np.int64).tolist())          # (+ 0.0: -0.0 and +0.0 are one value to every compare)
                assert len(tied) > S.A_LIST and len(bits) == 1, (case.id, b, side, h, int(r), len(tied), len(bits))


def test_list32_keys_are_distinct_in_fp64_equal_in_fp32_and_on_every_wave():
    seen = collections.Counter()
    for case in R.CASES:
        nk_max = max(case.N, case.M)
        ref = case.reference()
        for b, side, h, (ql, nq), (kl, nk) in case.units():
            if not (h > 0 and R.one_hot(nk)) or case.k >= nk:
                continue
            d = R.COLUMNS.index('list32')
            for r in range(d, min(nq, MODELLED_ROWS), 8):
                c = R.pattern(r)[2]
                row = ref[b, side][0][h][r].numpy()
                kth = np.sort(row)[::-1][case.k - 1]
                tied = np.nonzero(row.astype(np.float32) == np.float32(kth))[0]
                if c == 0.0 or (c < 0 and not R.list32_mirrored(nk, case.k)):
                    continue            # (a constant row, or the sign for which this frame had no room for the mirrored group)
                assert len(tied) == 32, (case.id, b, side, h, r, len(tied))
                assert len(set(row[tied].tolist())) == 32, (case.id, b, side, h, r)
                blocks = tied // 16
                assert len(set(blocks % 4)) == min(4, (nk + 15) // 16), (case.id, b, side, h, r, sorted(blocks))
                assert c < 0 or nk - 1 in tied, (case.id, b, side, h, r)          # (the frame's last key: the group above, c_r > 0)
                kept = ref[b, side][1][h][r].numpy()[tied]
                assert 0 < kept.sum() < 32, (case.id, b, side, h, r, int(kept.sum()))                     # the group straddles the k-th place
                seen[S.search_form(nk, nk_max)] += 1
    assert all(seen[f] >= MIN_ROWS for f in S.FORMS), seen


def test_reference_selection_is_topk_wherever_topk_is_specified():
    """The stable order keeps exactly k keys, every kept logit >= every dropped one, and among equal logits at the k-th place the lowest keys"""
    case = R.CASES[0]
    for (b, side), (logits, kept) in case.reference().items():
        assert bool((kept.sum(-1) == case.k).all())
        lo = logits.masked_fill(~kept, float('inf')).amin(-1)
        hi = logits.masked_fill(kept, float('-inf')).amax(-1)
        assert bool((lo >= hi).all())
        own = torch.zeros_like(kept).scatter_(-1, logits.topk(case.k, dim=-1).indices, True)
        assert torch.equal(own[lo > hi], kept[lo > hi])               # (no tie at the k-th place: torch.topk's keys exactly)
        for h, r in zip(*np.nonzero((lo == hi).numpy())):
            tied = np.nonzero((logits[h, r] == lo[h, r]).numpy())[0]
            k_tied = kept[h, r].numpy()[tied]
            assert not (~k_tied[:-1] & k_tied[1:]).any(), (b, side, h, r)          # kept ties are a prefix in key order
