"""fp32-class attention (csrc/attention.hip, csrc/attention_stream.hip) at every LAUNCH GEOMETRY the batch size selects, op by op.

launch_attention takes the split of a (pair, frame, head)'s query tiles over workgroups from B.  tests/test_gpu_ops.py runs B <= 3, where
no workgroup of attention_kernel walks a second tile and no wave of attention_topk16_kernel claims a second one
(tests/test_attention_plan.py states that as a property).  From B = 22 on they do: the second pass of attention_kernel's tile loop
re-initialises the running maximum, the sums, the accumulators and the surplus bookkeeping and reuses the staged K and V^T; the waves
of the 16-query kernels draw tiles from a counter in LDS and prefetch the next tile's queries.  Every case below asserts BEFORE the
launch, by mdgat_attention_plan, the instantiation, the split and the tiles per workgroup it was written for, and AFTERWARDS, by the
launch counters, that exactly that instantiation ran.  Then, with tolerances tests/test_gpu_ops.py uses for the same operations:

(a) against the fp64 oracle, for every pair, frame and head: full attention within 1e-5; dynamic attention with the kernel's own
    selection forced into the oracle (exactly k keys on every row, every disagreement with the oracle's selection a near-tie below
    5e-6 of a logit, the message within 1e-5 on EVERY row), and the untapped instantiation within 1e-6 of the tapped one;
(b) batch independence, bit for bit: every pair's rows (and kept keys) are those of the pair run alone at B = 1;
(c) run-to-run determinism, bit for bit: the order in which waves claim tiles must not reach the result.

Every pair of a batch holds different data (one seeded draw per shape, shared by the cases of that shape and never written).

Measured when the file was written (MI355X; every case prints its own line), self | cross - largest message error; largest selection gap;
milliseconds of the untapped op (q/k/v split + attention) on the device.  Tapped and untapped messages: equal in every case.
    full<8> B = 64          3.5e-6 | 2.4e-6;  -;               0.45 | 0.24
    dyn<16> B = 64          1.7e-6 | 2.1e-6;  2.9e-7 | 0;      0.50 | 0.49       B = 40: ... 7e-8 | 0; 0.33 | 0.31      B = 24: ... 7e-8 | 0; 0.21 | 0.20
    topk16<512> B = 64      2.5e-6 | 2.7e-6;  6e-8 | 2.1e-7;   0.39 | 0.37       B = 40: 2.3e-6 | 2.7e-6; the same; 0.24 | 0.24
                B = 24      2.3e-6 | 2.7e-6;  0 | 0;           0.15 | 0.16
    topk16<256> B = 64      2.4e-6 | 3.2e-6;  0 | 3e-8;        0.15 | 0.15       B = 16: 2.2e-6 | 2.1e-6; the same; 0.06 | 0.06
    wide<4>, stream, full<8,windowed> (B = 9): 1.7e-6, 2.1e-6, 2.2e-6; 0; 0.18, 0.13, 0.08"""
import functools
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_forms as A  # noqa: E402
from mdgat_matcher_amd import ops  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

DEV = 'cuda:0'
BMAX = 64
CHUNK = 8      # pairs per oracle call: the fp64 logits of 8 pairs of 512 x 512 are 67 MB per frame

# (kernel, N, M, k, cross, B, split, tiles per workgroup)
CASES = [
    # attention_kernel<false, 8, false>: 2 tiles of 256 queries; frame 0's second tile has 44 queries (waves 2-7 skip it)
    ('full<8>', 300, 500, 0, False, 64, 1, 2), ('full<8>', 300, 500, 0, True, 64, 1, 2),
    # attention_kernel<true, 16, false> and its TAP twin: 4 tiles of 128 queries (frame 0: 3, the last of 44)
    ('dyn<16>', 300, 500, 64, False, 64, 1, 4), ('dyn<16>', 300, 500, 64, True, 64, 1, 4),
    ('dyn<16>', 300, 500, 64, False, 40, 2, 2), ('dyn<16>', 300, 500, 64, True, 40, 2, 2),
    ('dyn<16>', 300, 500, 64, False, 24, 3, 2), ('dyn<16>', 300, 500, 64, True, 24, 3, 2),      # workgroup 0: tiles 0 and 3
    # attention_topk16_kernel<., ., 512>: 32 tiles of 16 queries over 8 waves
    ('topk16<512>', 512, 512, 128, False, 64, 1, 32), ('topk16<512>', 512, 512, 64, True, 64, 1, 32),
    ('topk16<512>', 512, 512, 128, False, 40, 2, 16), ('topk16<512>', 512, 512, 64, True, 40, 2, 16),
    ('topk16<512>', 512, 512, 128, False, 24, 3, 11), ('topk16<512>', 512, 512, 64, True, 24, 3, 11),   # the last part: 10 tiles
    # attention_topk16_kernel<., ., 256>: 16 tiles
    ('topk16<256>', 256, 256, 128, False, 64, 1, 16), ('topk16<256>', 256, 256, 128, True, 64, 1, 16),
    ('topk16<256>', 256, 256, 128, False, 16, 2, 8), ('topk16<256>', 256, 256, 128, True, 16, 2, 8),
    # geometry independent of B: one case each keeps the table whole and the counters honest
    ('wide<4>', 700, 600, 100, False, 9, 11, 1),
    ('stream', 512, 448, 0, True, 9, 4, 1),
    ('full<8,windowed>', 600, 700, 0, False, 9, 3, 1),
]


def _id(c):
    return f'{c[0]}-{c[1]}x{c[2]}-k{c[3]}-{"cross" if c[4] else "self"}-B{c[5]}'


@functools.lru_cache(maxsize=None)
def _data(N, M):
    """BMAX pairs of N + M keypoints, as tests/test_gpu_ops.py::test_attention_full draws them (standard normal times 1.3), every pair its
    own seed.  Shared and read-only: the cases of a shape take the first B pairs."""
    qkv = np.stack([np.random.RandomState(1000 * N + M + 7919 * b).standard_normal((N + M, 3, 4, 32)) * 1.3 for b in range(BMAX)])
    return torch.from_numpy(qkv)


# the pairs alone, B = 1: (N, M, k, cross, tap) -> {pair: (message, selection masks or None)}, on the device
_ALONE = {}


def _alone(N, M, k, cross, tap, pair):
    memo = _ALONE.setdefault((N, M, k, cross, tap), {})
    if pair not in memo:
        x = _data(N, M)[pair:pair + 1].to(DEV)
        r = ops.attention(x, N, M, cross, topk=k, return_selection=tap)
        memo[pair] = r if tap else (r, None)
    return memo[pair]


@pytest.fixture(scope='module', autouse=True)
def _release_the_shared_data():
    """The draws, the pairs alone and the allocator's cache (about 2 GB on the device) go when the file is done."""
    yield
    _ALONE.clear()
    _data.cache_clear()
    torch.cuda.empty_cache()


def _sides(qkv, N, M, cross):
    """(lo, hi, q, k, v) per side: q [B, dh, H, n] of the side's own frame, k / v of its source frame (the other one in a cross layer)."""
    out = []
    for side, (lo, hi) in enumerate(((0, N), (N, N + M))):
        slo, shi = ((N, N + M) if side == 0 else (0, N)) if cross else (lo, hi)
        out.append((lo, hi, qkv[:, lo:hi, 0].permute(0, 3, 2, 1), qkv[:, slo:shi, 1].permute(0, 3, 2, 1), qkv[:, slo:shi, 2].permute(0, 3, 2, 1)))
    return out


def _lib_rows(msg):
    """oracle message [B, dh, H, n] -> library rows [B, n, H * dh]"""
    b, dh, h, n = msg.shape
    return msg.permute(0, 3, 2, 1).reshape(b, n, h * dh)


def _launch(x, N, M, k, cross, tap, want, what):
    """One watched launch: (message, selection masks or None, milliseconds of the op on the device)."""
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with A.watch() as w:
        t0.record()
        r = ops.attention(x, N, M, cross, topk=k, return_selection=tap)
        t1.record()
    torch.cuda.synchronize()
    A.assert_launched(w, want, what)
    msg, sel = r if tap else (r, None)
    return msg, sel, t0.elapsed_time(t1)


def _same(a, b):
    (ma, sa), (mb, sb) = a, b
    return torch.equal(ma, mb) and (sa is None or all(torch.equal(p, q) for p, q in zip(sa, sb)))


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_attention_at_the_geometry(case):
    name, N, M, k, cross, B, split, tiles = case
    what = _id(case)
    dyn = k > 0
    wall = time.perf_counter()
    # ---- before the launch: the plan names the instantiation and the geometry this case was written for ----
    taps = (True, False) if dyn else (False,)
    for tap in taps:
        assert A.plan(B, N, M, k, tap) == (A.index(name, tap), split, tiles), (what, tap, A.plan(B, N, M, k, tap))
        assert A.plan(1, N, M, k, tap)[0] == A.index(name, tap), (what, tap)        # (the pair alone: the same instantiation)
    qkv = _data(N, M)[:B]
    x = qkv.to(DEV)
    runs, ms = {}, {}
    for tap in taps:
        want = A.index(name, tap)
        # ---- the launch, and afterwards the counters: exactly that instantiation, once ----
        msg, sel, _ = _launch(x, N, M, k, cross, tap, want, what)
        assert torch.isfinite(msg).all(), what
        runs[tap] = (msg, sel)
        # ---- (c) a second launch gives the same bits ----
        msg2, sel2, ms[tap] = _launch(x, N, M, k, cross, tap, want, what)
        assert _same(runs[tap], (msg2, sel2)), f'{what} tap={tap}: two launches of the same batch differ'
        # ---- (b) every pair as the pair alone ----
        for b in range(B):
            with A.watch() as w:
                alone = _alone(N, M, k, cross, tap, b)
            assert not w.launched() or w.launched() == {A.NAMES[want]: 1}, (what, w.launched())
            mine = (msg[b:b + 1], None if sel is None else tuple(s[b:b + 1] for s in sel))
            assert _same(mine, alone), f'{what} tap={tap}: pair {b} in the batch of {B} differs from the pair alone'
    # ---- (a) the fp64 oracle on every pair, frame and head, a few pairs at a time ----
    msg, sel = runs[dyn]
    err = gap = 0.0
    d_tap = float((runs[True][0] - runs[False][0]).abs().max()) if dyn else 0.0
    for c0 in range(0, B, CHUNK):
        out = msg[c0:c0 + CHUNK].cpu().double()
        for side, (lo, hi, q, kk, v) in enumerate(_sides(qkv[c0:c0 + CHUNK], N, M, cross)):
            if dyn:
                rep = []
                ref, _ = O.dynamic_attention(q, kk, v, k, forced=sel[side][c0:c0 + CHUNK].cpu(), report=rep)
                assert rep[0]['bad_count'] == 0, (what, c0, side, rep[0]['bad_count'])
                gap = max(gap, rep[0]['max_gap'])
            else:
                ref, _ = O.attention(q, kk, v)
            err = max(err, float((out[:, lo:hi] - _lib_rows(ref)).abs().max()))
    wall = time.perf_counter() - wall
    print(f'[attention-geometry] {what} split {split} tiles {tiles}: max message error {err:.3e}, max selection gap {gap:.3e}, '
          f'tap vs shipped {d_tap:.1e}, op on the device {ms[False]:.3f} ms' + (f' (tap {ms[True]:.3f} ms)' if dyn else '')
          + f', test {wall:.1f} s')
    assert gap < 5e-6, (what, gap)
    assert err < 1e-5, (what, err)
    assert d_tap < 1e-6, (what, d_tap)


def _param_sets(fn, names):
    """The parameter sets of a parametrized test function, as dicts."""
    marks = [m for m in fn.pytestmark if m.name == 'parametrize']
    sets = [{}]
    for m in marks:
        keys = [s.strip() for s in m.args[0].split(',')]
        sets = [dict(s, **dict(zip(keys, v if len(keys) > 1 else (v,)))) for s in sets for v in m.args[1]]
    assert sets and all(set(names) <= set(s) for s in sets)
    return sets


def test_every_split_f16_instantiation_is_launched_by_a_test():
    """The mode-0 indices no test of this file or of tests/test_gpu_ops.py launches: none.  Taken from the tests' own parameter tables
    through the plan (the instantiation does not depend on B: tests/test_attention_plan.py) - each of those tests asserts by the launch
    counters that the planned instantiation is the one that ran."""
    import test_gpu_ops as T
    reached = set()
    for name, N, M, k, cross, B, split, tiles in CASES:
        reached |= {A.plan(B, N, M, k, tap)[0] for tap in ((True, False) if k else (False,))}
    for s in _param_sets(T.test_attention_full, ('N', 'M')):
        reached.add(A.plan(2, s['N'], s['M'])[0])
    for s in _param_sets(T.test_attention_topk, ('N', 'M', 'k')):
        reached.add(A.plan(2, s['N'], s['M'], s['k'])[0])
    for s in _param_sets(T.test_attention_topk_cross, ('N', 'M', 'k')):
        reached |= {A.plan(2, s['N'], s['M'], s['k'], tap)[0] for tap in (True, False)}
    never = [A.NAMES[i] for i in A.MODE0 if i not in reached]
    assert never == [], never
