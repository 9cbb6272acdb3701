"""The fp64 GEMM launcher's choice of instantiation (csrc/f64.hip: gemm_f64_plan, exported as mdgat_gemm_f64_plan) as a pure function:
no device.  Pins the shapes the GPU tests rely on to the forms they name at 256 CUs, the launcher's promises at 256 and at 32 CUs (a
CPX partition), and the whole rule against its restatement below."""
import itertools

import numpy as np
import pytest

import gemm_f64_forms as F

CUS = (256, 32)
SLOW2, FAST32, FAST64, SLOW4, FAST4 = range(5)


def _name(i):
    return 'none' if i < 0 else F.NAMES[i]


def test_plain_shapes_reach_their_forms_at_256_cus():
    for form, cands in F.PLAIN.items():
        M, N, K = cands[0]
        assert _name(F.plan(M, N, K)) == form, (form, cands[0])
    assert _name(F.plan(*F.WIDE_RAGGED[0])) == '<4,slow>'
    # every other candidate reaches the form on SOME device
    for form, cands in F.PLAIN.items():
        for M, N, K in cands[1:]:
            assert any(_name(F.plan(M, N, K, cus=c)) == form for c in (32, 64, 128, 256, 304)), (form, M, N, K)


def test_two_source_and_bnt_shapes_reach_their_forms_at_256_cus():
    for (K0, K1, rows), form in F.TWO_SOURCE.items():
        assert _name(F.plan(rows, 64, K0 + K1, K0)) == form, (K0, K1, rows)
    for name, (ch, rows, form) in F.BNT.items():
        assert F.plan(rows[0], ch[2], ch[1], bnt=True) == F.index(form, True), name
    # the products of the backward that the same runs check: dx0 [R][K0] and dx1 [R][K1] = dY [R][64] Wt^T, single source, K = 64
    assert _name(F.plan(64, 32, 64)) == '<2,slow>' and _name(F.plan(64, 64, 64)) == '<2,fast,64>'
    assert _name(F.plan(70, 40, 64)) == '<2,slow>' and _name(F.plan(64, 8, 64)) == '<2,slow>'
    # dA of the wide BNT stack: [R][32] = dY [R][512] Wt^T
    assert _name(F.plan(8256, 32, 512)) == '<2,slow>'


def test_batched_shapes_reach_their_forms_at_256_cus():
    for (B, N, M), (form, cands) in F.BATCHED.items():
        assert cands[0] == B
        assert _name(F.plan(N, M, 128, batch=B)) == form, (B, N, M)
        # final_proj of the same call: B N rows x 128 x 128, one product
        assert _name(F.plan(B * N, 128, 128)) in ('<2,fast,64>', '<2,fast,32>', '<4,fast>')


def test_candidate_lists_cover_the_partition_sizes():
    for cus in (32, 64, 128, 256, 304):
        for form, cands in list(F.PLAIN.items()) + [('<4,slow>', F.WIDE_RAGGED)]:
            F.pick(cands, F.index(form), cus, lambda s: dict(M=s[0], N=s[1], K=s[2]))
        for ch, rows, form in F.BNT.values():
            F.pick(rows, F.index(form, True), cus, lambda r: dict(M=r, N=ch[2], K=ch[1], bnt=True))
        for (B, N, M), (form, cands) in F.BATCHED.items():
            F.pick(cands, F.index(form), cus, lambda b: dict(M=N, N=M, K=128, batch=b))
    with pytest.raises(AssertionError, match='256 CUs'):
        F.pick([(64, 64, 64)], F.index('<4,fast>'), 256, lambda s: dict(M=s[0], N=s[1], K=s[2]))


def test_no_launch_and_refusals():
    assert F.plan(0, 64, 64) == -1 and F.plan(64, 0, 64) == -1 and F.plan(64, 64, 0) == -1 and F.plan(-1, 64, 64) == -1
    assert F.plan(64, 64, 64, cus=0) == -1
    assert F.plan(64, 64, 64, K0=32, bnt=True) == -1           # the operand transform takes a single source
    assert F.plan(64, 64, 64, K0=64, bnt=True) == 5 + FAST64


# shapes around every boundary of the rule: tile edges, chunk edges, one / many rounds of workgroups
_MS = (1, 63, 64, 65, 128, 512, 2100, 2112, 8250, 8256, 16384, 32768)
_NS = (1, 16, 32, 63, 64, 65, 96, 128, 129, 256, 384, 500, 512, 2048)
_KS = (1, 31, 32, 33, 36, 64, 96, 128, 256)
_BS = (0, 1, 2, 5, 17, 64)


def _grid():
    for M, N, K, batch in itertools.product(_MS, _NS, _KS, _BS):
        if (M + 63) // 64 * ((N + 63) // 64) * max(batch, 1) > 200000:
            continue
        for K0 in sorted({K, K + 7, K // 2, 32, 64, 8} - {0}):
            yield M, N, K, K0, batch


@pytest.mark.parametrize('cus', CUS)
def test_promises_of_the_dispatcher(cus):
    seen = set()
    for M, N, K, K0, batch in _grid():
        for bnt in (False, True):
            if bnt and K0 < K:
                continue
            got = F.plan(M, N, K, K0, batch, True, bnt, cus)
            assert 5 * bnt <= got < 5 * bnt + 5, (M, N, K, K0, batch, bnt)
            form = got - 5 * bnt
            seen.add(got)
            what = f'M={M} N={N} K={K} K0={K0} batch={batch} bnt={bnt} cus={cus}: {_name(got)}'
            wn = 4 if form in (SLOW4, FAST4) else 2
            if N <= 64:
                assert wn == 2, what
            # the tile width does not depend on alignment; without alignment nothing is fast
            loose = F.plan(M, N, K, K0, batch, False, bnt, cus) - 5 * bnt
            assert loose == (SLOW4 if wn == 4 else SLOW2), what
            # fast: every shape condition holds, and not one of them may fail
            whole = M % 64 == 0 and N % (32 * wn) == 0 and K % 32 == 0 and K0 % 32 == 0
            assert (form in (FAST32, FAST64, FAST4)) == whole, what
            if form == FAST64:      # deep implies fast (above), the narrow tile, whole chunks of 64 from one source each, at most a tile per CU
                tiles = (M + 63) // 64 * ((N + 63) // 64) * max(batch, 1)
                assert wn == 2 and K % 64 == 0 and (K0 >= K or K0 % 64 == 0) and tiles <= cus, what
    assert seen == set(range(10)), sorted(seen)


def _restated(M, N, K, K0, batch, aligned, cus):
    """The rule as DESIGN states it, in Python."""
    nb = max(batch, 1)
    rows = (M + 63) // 64
    wn = 2
    if N > 64:
        tw, tn = rows * nb * ((N + 127) // 128), rows * nb * ((N + 63) // 64)
        rw, rn = -(-tw // (3 * cus)), -(-tn // (4 * cus))
        wn = 2 if tw <= 6 * cus and rn * 55 < rw * 100 else 4
    fast = aligned and M % 64 == 0 and N % (32 * wn) == 0 and K % 32 == 0 and K0 % 32 == 0
    deep = fast and wn == 2 and K % 64 == 0 and (K0 >= K or K0 % 64 == 0) and rows * ((N + 63) // 64) * nb <= cus
    return (FAST4 if fast else SLOW4) if wn == 4 else FAST64 if deep else FAST32 if fast else SLOW2


@pytest.mark.parametrize('cus', CUS + (64, 128, 304))
def test_plan_is_the_stated_rule(cus):
    n = 0
    for M, N, K, K0, batch in _grid():
        for aligned in (True, False):
            assert F.plan(M, N, K, K0, batch, aligned, False, cus) == _restated(M, N, K, K0, batch, aligned, cus), (M, N, K, K0, batch, aligned)
            n += 1
    rs = np.random.RandomState(cus)
    for _ in range(2000):
        M, N, K = int(rs.randint(1, 70000)), int(rs.randint(1, 2100)), int(rs.randint(1, 520))
        if rs.randint(2):
            M, N, K = M // 64 * 64 + 64, N // 128 * 128 + 128, K // 32 * 32 + 32
        K0 = K if rs.randint(2) else int(rs.randint(1, K + 1)) // 32 * 32 + 32 * int(rs.randint(2))
        batch = int(rs.choice([1, 1, 2, 8, 64]))
        if K0 == 0:
            K0 = K
        assert F.plan(M, N, K, K0, batch, True, False, cus) == _restated(M, N, K, K0, batch, True, cus), (M, N, K, K0, batch)
    assert n > 1000
