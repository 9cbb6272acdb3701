"""tests/test_gpu_prefilled_ops.py's bar for the entries of include/mdgat_hip_wide.h (``_lib.WIDE_SIGNATURES``): each op must return the same
bits whatever its workspace and its outputs held before the call.  A case runs one op three times on the same inputs - every ``torch.empty``
tensor of the call prefilled with 0x00, with 0xFF, and with the final bytes of an earlier, LOUDER call of the same entry at the same shape
(inputs scaled by 4, pairs in reverse order) - and every returned tensor must be BIT-identical across the three (tests/prefilled.py).  Every
case also asserts that the C entries it names really ran and that the fill reached a uint8 allocation at least as large as the workspace the
library asked for.  What the runs compute is held to the oracle by the ops' own test files at the same shapes.

``ENTRIES`` / ``EXEMPT`` are to ``_lib.WIDE_SIGNATURES`` what tests/test_prefilled_table.py's tables are to ``_lib.SIGNATURES``;
tests/test_ragged_fp32_wide_refusals.py checks them without a GPU."""
import functools
from collections import namedtuple

import pytest
import torch

from mdgat_matcher_amd import _lib, ops
from prefilled import prefilled, same_bits, snapshot, spy

DEV = 'cuda:0'
THR = 0.01

# entry -> the query that sizes its workspace
WS_OF = {'mdgat_sinkhorn_ragged_wide': 'mdgat_sinkhorn_ragged_wide_workspace_bytes',
         'mdgat_sinkhorn_extract_ragged_wide': 'mdgat_sinkhorn_ragged_wide_workspace_bytes',
         'mdgat_attention_ragged_wide': 'mdgat_attention_workspace_bytes'}
# the symbols of the wide header that touch no device memory: C symbol -> (the reason, as test_prefilled_table.REASONS names them; what it is)
EXEMPT = {'mdgat_set_ragged_fp32_slots': ('a setter', 'the slot limit of a handle\'s fp32-class ragged plan'),
          'mdgat_sinkhorn_ragged_wide_workspace_bytes': ('a query', 'a size'),
          'mdgat_ragged_wide_launches': ('a counter', 'the launches only a wide ragged slot reaches, into a host array')}

Case = namedtuple('Case', 'entries make')
CASES = {}          # id -> Case; make(loud) -> run() -> a nest of tensors


def case(cid, entries):
    def register(make):
        assert cid not in CASES, cid
        CASES[cid] = Case(tuple(entries), make)
        return make
    return register


def _mk_sinkhorn(name, split, loud):
    """wide slots: 65 x 600 on the one-workgroup kernel (NC = 16), 600 x 65 on the split form (5 slabs: partials and potentials in scratch)"""
    import test_gpu_ragged_sinkhorn_fp32_wide as RW
    _, counts, alpha, _, _ = RW.SETS[name]
    order = list(range(len(counts)))[::-1] if loud else list(range(len(counts)))
    s = (RW._scores(name, order=order) * (4.0 if loud else 1.0)).to(DEV)            # NaN beyond every pair's counts
    kw = dict(counts=RW._cnt([counts[b] for b in order]), wide=True, split=split)

    def run():
        out = {'Z': ops.sinkhorn(s, alpha, RW.ITERS, **kw)}
        for mode in range(4):
            for want_Z in (False, True):
                out[f'extract{mode}{"+Z" if want_Z else ""}'] = ops.sinkhorn_extract(s, alpha, RW.ITERS, mode=mode, match_threshold=THR, want_Z=want_Z, **kw)
        return out
    return run


for _name, _split in (('cols', False), ('rows', True)):
    case(f'sinkhorn-ragged-wide-{_name}', ('mdgat_sinkhorn_ragged_wide', 'mdgat_sinkhorn_extract_ragged_wide'))(functools.partial(_mk_sinkhorn, _name, _split))


def _mk_attention(k, loud):
    """wide slots of 544 x 520: the windowed kernel's ragged instantiation, and wide<4>'s with and without the tap"""
    import test_gpu_ragged_attention_fp32_wide as RW
    (Np, Mp), counts = RW.SETS['w4']
    order = list(range(len(counts)))[::-1] if loud else list(range(len(counts)))
    x = (RW._qkv('w4', order=order) * (4.0 if loud else 1.0)).to(DEV)       # NaN beyond every pair's counts
    cnt = ([counts[b][0] for b in order], [counts[b][1] for b in order])

    def run():
        return {(cross, sel): ops.attention(x, Np, Mp, cross, topk=k, return_selection=sel, counts=cnt, wide=True) for cross in (False, True) for sel in (False, True)}
    return run


for _k in (0, 64):
    case(f'attention-ragged-wide-w4-k{_k}', ('mdgat_attention_ragged_wide',))(functools.partial(_mk_attention, _k))

# C symbol -> the cases that cover it
ENTRIES = {}
for _cid, _c in CASES.items():
    for _e in _c.entries:
        ENTRIES.setdefault(_e, []).append(_cid)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', sorted(CASES))
def test_prefilled(cid):
    c = CASES[cid]
    lib = _lib.load()
    sizes = sorted({WS_OF[e] for e in c.entries})
    runs = {name: c.make(False) for name in ('zero', 'ones', 'replay')}       # inputs are built outside the fills
    louder = c.make(True)
    try:
        with spy(lib, c.entries + tuple(sizes)) as s, prefilled('zero') as p0:
            kept = runs['zero']()
            torch.cuda.synchronize()
        zero = snapshot(kept)
        for e in c.entries:
            assert s.calls[e] >= 1, f'{cid}: {e} was never called'
        with prefilled('ones') as p1:
            ones = runs['ones']()
            torch.cuda.synchronize()
        ones = snapshot(ones)
        with prefilled('zero', record=True) as rec:
            louder()
        with prefilled('replay', source=rec) as p2:
            replay = runs['replay']()
            torch.cuda.synchronize()
        replay = snapshot(replay)
    finally:
        torch.cuda.synchronize()
    need = s.most_asked()
    print(f'{cid}: {p1.count} allocations, {p1.bytes} bytes prefilled, scratch {p1.scratch_bytes} for {need} asked; replayed {p2.replayed} of {p2.count}')
    assert zero, f'{cid}: the case returned no tensor'
    assert need > 0 and p0.count == p1.count == p2.count > 0
    assert p1.saw_scratch(need) and p2.saw_scratch(need), f'{cid}: the fill never reached a workspace of {need} bytes (largest: {p1.scratch_bytes})'
    assert p2.replayed == p2.count, f'{cid}: only {p2.replayed} of {p2.count} allocations found their recorded twin'
    same_bits(zero, ones, f'{cid}: 0xFF against 0x00')
    same_bits(zero, replay, f'{cid}: a louder call\'s bytes against 0x00')
