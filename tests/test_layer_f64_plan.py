"""The fp64 layer-tail and encoder launchers' choice of form and grid (csrc/layer_f64.hip: layer_f64_plan, exported as
mdgat_layer_f64_plan) as a pure function: no device.  Holds the cases of tests/test_gpu_layer_f64_forms.py to the forms they name, sweeps
the rule's properties over every residue of R, and checks that the case table leaves no form and no edge of a form without a case.  Every threshold is formed
from the function's own inputs (R, cus); the only constant is the flag buffer's 256 blocks, which include/mdgat_hip.h states."""
import itertools

import pytest

import layer_f64_forms as F

MAX_CLUSTERS = 256      # include/mdgat_hip.h: nblk <= 256


def _ceil(a, b):
    return -(-a // b)


def _clustered(R, encoder, has_hid, chained, mode, cus):
    """The five conditions of the clustered form, and that it is a tail at all"""
    nblk = _ceil(R, 16)
    return not encoder and mode == 1 and bool(has_hid) and bool(chained) and 4 * nblk <= cus and nblk <= MAX_CLUSTERS


def _sweep_rows():
    """1 .. 20000 in steps that hit every residue mod 32 (33 is coprime to 32), and both sides of every threshold the sweep's CU counts
    put below 20000 rows"""
    rows = set(range(1, 200)) | set(range(1, 20001, 33))
    for cus in (64, 256, 304):
        for edge in (16 * (cus // 4), 32 * (2 * cus - 1), 16 * MAX_CLUSTERS):
            rows |= {r for r in range(edge - 33, edge + 34) if 1 <= r <= 20000}
    return sorted(rows)


@pytest.mark.parametrize('cus', (64, 256, 304))
def test_properties_of_the_plan(cus):
    seen = set()
    for R in _sweep_rows():
        nblk = _ceil(R, 16)
        for mode, encoder, has_hid, chained in itertools.product(F.MODES, (0, 1), (0, 1), (0, 1)):
            form, wg, rows = F.plan(R, encoder, has_hid, chained, mode, cus)
            what = (R, mode, encoder, has_hid, chained, form, wg, rows)
            seen.add(form)
            # mode 0 never returns a fused form, and no other mode an unfused one
            assert (form in (F.TAIL_GEMMS, F.ENC_GEMMS)) == (mode == 0), what
            if mode == 0:
                assert form == (F.ENC_GEMMS if encoder else F.TAIL_GEMMS) and (wg, rows) == (0, 0), what
                continue
            # an encoder launch takes an encoder form (never the clustered one), a tail a tail form
            assert (form in (F.ENC16, F.ENC32)) == bool(encoder) and (form in (F.TAIL16, F.TAIL32, F.CLUSTER)) == (not encoder), what
            # clustered <=> all five conditions hold
            assert (form == F.CLUSTER) == _clustered(R, encoder, has_hid, chained, mode, cus), what
            assert wg * rows >= R, what
            if form == F.CLUSTER:
                # whole groups of eight clusters of four workgroups; 4 nblk of them find rows
                assert rows == 16 and wg % 32 == 0 and wg == 32 * _ceil(nblk, 8) and 4 * nblk <= wg < 4 * nblk + 32, what
                continue
            # 32 rows <=> forced, or ceil(R / 32) >= 2 cus (and not forced to 16)
            want32 = mode == 32 or (mode != 16 and _ceil(R, 32) >= 2 * cus)
            assert rows == (32 if want32 else 16) and (form in (F.TAIL32, F.ENC32)) == want32, what
            assert wg == _ceil(R, rows), what
    assert seen == set(range(7)), sorted(seen)


def test_modes_are_read_as_the_setter_reads_them():
    for R, encoder in itertools.product((8, 531, 1024, 1040, 16384), (0, 1)):
        for other in (3, 7, 15, 17, 31, 33, 64, 1000):      # any other positive value: 1
            assert F.plan(R, encoder, mode=other) == F.plan(R, encoder, mode=1), (R, other)
    assert F.plan(0)[0] == -1 and F.plan(-5, True) == (-1, 0, 0)


def test_the_current_setting_is_the_negative_mode():
    try:
        for mode in F.MODES:
            with F.fusion(mode):
                for R in (8, 531, 1040, 16384):
                    assert F.plan(R, mode=-1) == F.plan(R, mode=mode) and F.plan(R, True, mode=-1) == F.plan(R, True, mode=mode), (R, mode)
    finally:
        F._lib().mdgat_set_f64_layer_fusion(-1)


def test_the_edges_worked_by_hand_at_256_cus():
    """64 blocks of 16 rows are a quarter of 256 CUs; 512 workgroups of 32 rows are two per CU."""
    assert F.plan(1024) == (F.CLUSTER, 256, 16) and F.plan(1025) == (F.TAIL16, 65, 16)
    assert F.plan(531) == (F.CLUSTER, 160, 16)          # 34 blocks -> 5 groups of 8 clusters: 160 workgroups, 136 with rows
    assert F.plan(8) == (F.CLUSTER, 32, 16)
    assert F.plan(1024, has_hid=False) == F.plan(1024, chained=False) == F.plan(1024, mode=2) == (F.TAIL16, 64, 16)
    assert F.plan(16352) == (F.TAIL16, 1022, 16) and F.plan(16353) == (F.TAIL32, 512, 32)
    assert F.plan(16352, True) == (F.ENC16, 1022, 16) and F.plan(16353, True) == (F.ENC32, 512, 32)
    assert F.plan(365, mode=32) == (F.TAIL32, 12, 32) and F.plan(365, mode=16) == (F.TAIL16, 23, 16)
    # beyond 256 blocks no device clusters, however many CUs it has
    assert F.plan(16 * 256, cus=4096)[0] == F.CLUSTER and F.plan(16 * 256 + 1, cus=4096)[0] == F.TAIL16


def test_the_cases_of_the_gpu_tests_reach_their_forms():
    assert len({c.id for c in F.CASES}) == len(F.CASES)
    for c in F.CASES:
        R = c.B * (c.n + c.m)
        want = {c.encoder_form: 1}
        if c.tail_form is not None:
            want[c.tail_form] = F.f64_layers(c)
        assert F.f64_layers(c) == (0 if c.tail_form is None else F.f64_layers(c)) and F.case_forms(c) == want, (c.id, F.named(F.case_forms(c)))
        assert F.case_forms(c, mode=0) == {F.ENC_GEMMS: 1, **({F.TAIL_GEMMS: F.f64_layers(c)} if F.f64_layers(c) else {})}, c.id
        assert all(k is None or k <= min(c.n, c.m) for k in c.k) and len(c.k) in (0, 2 * c.L), c.id
        assert not c.alone or c.B > 1, c.id
        if R <= F.ORACLE_MAX_ROWS:
            assert c.B * c.n * c.m <= 512 * 528, c.id       # (the CPU oracle stays quick)
    by_id = {c.id: c for c in F.CASES}
    # the edges the table is there for, in the plan's own terms
    assert F.plan(1024)[1] == 4 * 64 and by_id['cluster_full'].B * 1024 == 1024
    assert 4 * -(-1040 // 16) > F.CASE_CUS >= 4 * (1024 // 16)
    assert -(-531 // 16) % 8 == 2 and 531 % 16 == 3 and 365 % 32 == 13 and 365 % 16 == 13
    assert -(-16384 // 32) == 2 * F.CASE_CUS and -(-16320 // 32) == 2 * F.CASE_CUS - 2
    assert F.f64_layers(by_id['last_layer_cluster']) == 3 and F.f64_layers(by_id['encoders_only']) == 0


def _uncovered(cases):
    """The forms no row of `cases` reaches at CASE_CUS, by its own run or by its three-launch reference (mode 0)"""
    reached = set()
    for c in cases:
        reached |= set(F.case_forms(c)) | set(F.case_forms(c, mode=0))
    return set(range(len(F.NAMES))) - reached


def test_every_form_has_a_case():
    assert not _uncovered(F.CASES), [F.NAMES[i] for i in sorted(_uncovered(F.CASES))]


def _edges(cus=F.CASE_CUS):
    """The edges of the forms, each as a predicate over a row of the table (in the plan's terms at `cus` compute units)"""
    R = lambda c: c.B * (c.n + c.m)
    nblk = lambda c: _ceil(R(c), 16)
    form = lambda c: F.plan(R(c), mode=c.mode, cus=cus)[0] if F.f64_layers(c) else None
    hands_over = lambda c: c.tail == 'fp32' and 0 < F.f64_layers(c) < 2 * c.L        # a tail without a next q | k | v whose fp32 x is read
    return {
        'clustered, the most blocks a device takes, whole groups': lambda c: form(c) == F.CLUSTER and 4 * nblk(c) == cus and nblk(c) % 8 == 0,
        'mode 1, one block too many to cluster': lambda c: c.mode == 1 and form(c) == F.TAIL16 and 4 * (nblk(c) - 1) == cus,
        'clustered, surplus workgroups and a partial last block': lambda c: form(c) == F.CLUSTER and nblk(c) % 8 and R(c) % 16,
        'clustered, a single partial block': lambda c: form(c) == F.CLUSTER and nblk(c) == 1 and R(c) % 16,
        '32 rows by the default rule, exactly at the threshold': lambda c: c.mode == 1 and form(c) == F.TAIL32 and _ceil(R(c), 32) == 2 * cus,
        '16 rows by the default rule, at most two workgroups below it': lambda c: c.mode == 1 and form(c) == F.TAIL16 and 0 < 2 * cus - _ceil(R(c), 32) <= 2,
        '32 rows, the last second row block wholly beyond R': lambda c: form(c) == F.TAIL32 and 1 <= R(c) % 32 <= 16,
        '16 rows forced, a partial last block': lambda c: c.mode == 16 and form(c) == F.TAIL16 and R(c) % 16,
        'mode 2 at the largest launch mode 1 clusters': lambda c: c.mode == 2 and form(c) == F.TAIL16 and 4 * nblk(c) == cus,
        'the hand-over from the clustered tail': lambda c: hands_over(c) and form(c) == F.CLUSTER,
        'the hand-over from tail<1>': lambda c: hands_over(c) and form(c) == F.TAIL16,
        'the hand-over from tail<2>': lambda c: hands_over(c) and form(c) == F.TAIL32,
        'the hand-over from encoder<1>': lambda c: c.tail == 'fp32' and F.f64_layers(c) == 0 and c.encoder_form == F.ENC16,
        'the hand-over from encoder<2>': lambda c: c.tail == 'fp32' and F.f64_layers(c) == 0 and c.encoder_form == F.ENC32,
        'pair 0 alone: clustered ragged, 32 rows by the rule, 32 rows with a half block': lambda c: c.alone,
    }


def test_every_edge_has_a_case():
    for what, reaches in _edges().items():
        assert any(reaches(c) for c in F.CASES), what
    alone = [c for c in F.CASES if c.alone]
    assert {F.plan(c.B * (c.n + c.m), mode=c.mode)[0] for c in alone} == {F.CLUSTER, F.TAIL32} and any(c.mode == 32 for c in alone)


def test_a_form_that_loses_its_cases_is_noticed():
    """Take away all rows of a form: the check above must name that form.  (Forms 0 and 6 are every row's reference run.)"""
    for form in (F.TAIL16, F.TAIL32, F.CLUSTER, F.ENC16, F.ENC32):
        rest = [c for c in F.CASES if form not in F.case_forms(c)]
        assert len(rest) < len(F.CASES) and form in _uncovered(rest), F.NAMES[form]
        assert form not in _uncovered(rest + [next(c for c in F.CASES if form in F.case_forms(c))]), F.NAMES[form]
    assert _uncovered([c for c in F.CASES if c.tail_form is None]) == {F.TAIL16, F.TAIL32, F.CLUSTER, F.TAIL_GEMMS}
    assert _uncovered([]) == set(range(7))
