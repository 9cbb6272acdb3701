"""The fp32 Sinkhorn launchers' choices (csrc/sinkhorn.hip: sinkhorn_plan, exported as mdgat_sinkhorn_plan) as a pure function: no device.
Pins a table worked by hand - every threshold on M and N, the XCD placement on and off, the groups in flight against B, the cooperative
launch, the workspace test, the refusals, the shapes tests/test_gpu_sinkhorn_forms.py runs - and the whole rule, stated again in Python,
over a sweep."""
import pytest

import sinkhorn_forms as S
from sinkhorn_forms import CLUSTER, NONE, STREAMING

S4, S16, S2D = S.SCALING


# ---- the streaming kernel's instantiation: thresholds on M (and N <= 4096 beyond 512 columns) ----
@pytest.mark.parametrize('N,M,want', [
    (3, 64, 'stream<1,16>'), (3, 65, 'stream<2,16>'), (3, 128, 'stream<2,16>'), (3, 129, 'stream<4,16>'), (3, 256, 'stream<4,16>'),
    (3, 257, 'stream<8,16>'), (3, 512, 'stream<8,16>'), (3, 513, 'stream<16,8>'), (3, 1024, 'stream<16,8>'), (3, 1025, 'stream<32,8>'),
    (3, 2048, 'stream<32,8>'), (3, 2049, None),
    (4096, 513, 'stream<16,8>'), (4097, 513, None), (4096, 2048, 'stream<32,8>'), (4097, 1025, None), (4097, 512, 'stream<8,16>'),
    (100000, 64, 'stream<1,16>'),
])
def test_streaming_thresholds(N, M, want):
    for B in (1, 70):
        p = S.plan(B, N, M, workspace=False)
        if want is None:
            assert p == S.Plan(NONE, 'none', 'none', 0, 0, 0, False, 0, False), (B, p)
        else:
            assert p == S.Plan(STREAMING, 'none', want, 0, 0, 0, False, B, False), (B, p)


# ---- the cluster kernel: (B, N, M, cus) -> (scaling, gated, GR, GC, ngroups, xcd_map, grid), worked by hand ----
# P = GR GC workgroups per pair; ngroups = min(cus // P, min(64, 256 // P), B); ng8 = ngroups rounded up to 8;
# xcd_map = P (ng8 / 8) <= cus // 8; grid = (ng8 if xcd_map else ngroups) P
CLUSTER_TABLE = [
    # N at 128 | 129, 512 | 513, 2048 (2049: below)
    ((3, 128, 64, 256), (S4, 'stream<1,16>', 1, 1, 3, True, 8)),
    ((3, 129, 64, 256), (S4, 'stream<1,16>', 2, 1, 3, True, 16)),
    ((3, 512, 64, 256), (S4, 'stream<1,16>', 4, 1, 3, True, 32)),
    ((3, 513, 64, 256), (S16, 'stream<1,16>', 5, 1, 3, True, 40)),
    ((3, 2048, 64, 256), (S16, 'stream<1,16>', 16, 1, 3, True, 128)),
    # M at 64 | 65, 128 | 129, 256 | 257 (the gated kernel's instantiation), 512 | 513, 1024 | 1025, 2048
    ((3, 64, 65, 256), (S4, 'stream<2,16>', 1, 1, 3, True, 8)),
    ((3, 64, 128, 256), (S4, 'stream<2,16>', 1, 1, 3, True, 8)),
    ((3, 64, 129, 256), (S4, 'stream<4,16>', 1, 1, 3, True, 8)),
    ((3, 64, 256, 256), (S4, 'stream<4,16>', 1, 1, 3, True, 8)),
    ((3, 64, 257, 256), (S4, 'stream<8,16>', 1, 1, 3, True, 8)),
    ((3, 64, 512, 256), (S4, 'stream<8,16>', 1, 1, 3, True, 8)),
    ((3, 64, 513, 256), (S2D, 'stream<16,8>', 1, 2, 3, True, 16)),
    ((3, 64, 1024, 256), (S2D, 'stream<16,8>', 1, 2, 3, True, 16)),
    ((3, 64, 1025, 256), (S2D, 'stream<32,8>', 1, 3, 3, True, 24)),
    ((3, 64, 2048, 256), (S2D, 'stream<32,8>', 1, 4, 3, True, 32)),
    ((3, 600, 600, 256), (S2D, 'stream<16,8>', 5, 2, 3, True, 80)),         # 5 row slabs and 2 column slabs: the two-dimensional form
    # the XCD placement: P = 4 with B = 64 is on (4 x 8 = 32 CUs of an XCD) ...
    ((64, 512, 512, 256), (S4, 'stream<8,16>', 4, 1, 64, True, 256)),
    # ... P = 5: 51 groups fit (ng8 = 56: 5 x 7 = 35 > 32: off) from B = 52 on (and from 49: ng8 = 56 as well); 48 groups are placed
    ((52, 513, 40, 256), (S16, 'stream<1,16>', 5, 1, 51, False, 255)),
    ((70, 513, 40, 256), (S16, 'stream<1,16>', 5, 1, 51, False, 255)),
    ((49, 513, 40, 256), (S16, 'stream<1,16>', 5, 1, 49, False, 245)),
    ((48, 513, 40, 256), (S16, 'stream<1,16>', 5, 1, 48, True, 240)),
    # ... 2048 x 2048: 64 workgroups per pair never fit an XCD
    ((1, 2048, 2048, 256), (S2D, 'stream<32,8>', 16, 4, 1, False, 64)),
    ((2, 2048, 2048, 256), (S2D, 'stream<32,8>', 16, 4, 2, False, 128)),
    ((9, 2048, 2048, 256), (S2D, 'stream<32,8>', 16, 4, 4, False, 256)),
    # ngroups against B and sk_max_groups (64 at most, 256 // P)
    ((1, 64, 64, 256), (S4, 'stream<1,16>', 1, 1, 1, True, 8)),
    ((9, 64, 64, 256), (S4, 'stream<1,16>', 1, 1, 9, True, 16)),
    ((64, 64, 64, 256), (S4, 'stream<1,16>', 1, 1, 64, True, 64)),
    ((66, 64, 64, 256), (S4, 'stream<1,16>', 1, 1, 64, True, 64)),         # two pairs for groups 0 and 1
    ((34, 130, 65, 256), (S4, 'stream<2,16>', 2, 1, 34, True, 80)),        # (every pair its own group)
    ((66, 130, 65, 256), (S4, 'stream<2,16>', 2, 1, 64, True, 128)),       # two pairs for groups 0 and 1
    ((130, 129, 64, 256), (S4, 'stream<1,16>', 2, 1, 64, True, 128)),
    ((70, 300, 512, 256), (S4, 'stream<8,16>', 3, 1, 64, True, 192)),      # 256 // 3 = 85 -> 64 groups, 8 per XCD: 3 x 8 = 24 <= 32
    ((5, 2048, 300, 256), (S16, 'stream<8,16>', 16, 1, 5, True, 128)),
    ((20, 2048, 300, 256), (S16, 'stream<8,16>', 16, 1, 16, True, 256)),
    # a smaller part: the groups follow the CU count
    ((64, 512, 512, 128), (S4, 'stream<8,16>', 4, 1, 32, True, 128)),
    ((64, 512, 512, 64), (S4, 'stream<8,16>', 4, 1, 16, True, 64)),
    ((3, 2048, 2048, 64), (S2D, 'stream<32,8>', 16, 4, 1, False, 64)),
]


@pytest.mark.parametrize('case,want', CLUSTER_TABLE, ids=[f'{c[0]}x{c[1]}x{c[2]}-cu{c[3]}' for c, _ in CLUSTER_TABLE])
def test_pinned_cluster_cases(case, want):
    B, N, M, cus = case
    p = S.plan(B, N, M, cus=cus)
    assert p.path == CLUSTER and not p.cooperative, p
    assert (p.scaling, p.stream, p.GR, p.GC, p.ngroups, p.xcd_map, p.grid) == want


def test_2049_rows_or_columns_leave_the_cluster_kernel():
    # no workspace size exists for them (mdgat_sinkhorn_workspace_bytes = 0): the streaming kernel, or a refusal
    assert S.workspace_bytes(3, 2049, 64) == 0 and S.workspace_bytes(3, 64, 2049) == 0
    assert S.plan(3, 2049, 64, ws_addr=4096, ws_bytes=1 << 30) == S.Plan(STREAMING, 'none', 'stream<1,16>', 0, 0, 0, False, 3, False)
    assert S.plan(3, 2049, 513, ws_addr=4096, ws_bytes=1 << 30).stream == 'stream<16,8>'
    assert S.plan(3, 64, 2049, ws_addr=4096, ws_bytes=1 << 30).path == NONE


def test_no_fallback_buffer_means_a_cooperative_launch_and_nothing_behind_it():
    for B, N, M in ((3, 64, 64), (64, 512, 512), (5, 513, 40), (2, 2048, 2048)):
        with_fb, without = S.plan(B, N, M), S.plan(B, N, M, fallback=False)
        assert not with_fb.cooperative and with_fb.stream != 'none'
        assert without.cooperative and without.stream == 'none'
        assert without._replace(cooperative=False, stream=with_fb.stream) == with_fb          # nothing else changes
        assert S.expected(without) == {without.scaling: 1} and S.expected(with_fb) == {with_fb.scaling: 1, S.GATED: 1}


def test_workspace_too_small_or_misaligned_selects_the_streaming_kernel():
    B, N, M = 5, 300, 200
    need = S.workspace_bytes(B, N, M)
    assert need > 0
    streaming = S.Plan(STREAMING, 'none', 'stream<4,16>', 0, 0, 0, False, B, False)
    assert S.plan(B, N, M, ws_addr=4096, ws_bytes=need).path == CLUSTER
    assert S.plan(B, N, M, ws_addr=4096 + 256, ws_bytes=need + 7).path == CLUSTER
    assert S.plan(B, N, M, ws_addr=4096, ws_bytes=need - 1) == streaming
    assert S.plan(B, N, M, ws_addr=4096, ws_bytes=0) == streaming
    for off in (1, 16, 128, 255):
        assert S.plan(B, N, M, ws_addr=4096 + off, ws_bytes=need + 256) == streaming, off
    assert S.plan(B, N, M, workspace=False) == streaming
    # the size grows with the batch: what suffices for 5 pairs does not for 6
    assert S.plan(B + 1, N, M, ws_addr=4096, ws_bytes=need).path == STREAMING


def test_more_workgroups_per_pair_than_compute_units_is_refused():
    for B, N, M, cus, ok in ((1, 2048, 2048, 64, True), (1, 2048, 2048, 63, False), (3, 513, 40, 5, True), (3, 513, 40, 4, False),
                             (3, 64, 64, 1, True), (3, 64, 64, 0, False)):
        p = S.plan(B, N, M, cus=cus)
        assert (p.path == CLUSTER) == ok, (B, N, M, cus, p)
        if not ok:
            assert p.path == NONE and p.ngroups == 0 and p.grid == 0


def test_nothing_to_launch():
    for B, N, M in ((0, 64, 64), (-1, 64, 64), (3, 0, 64), (3, 64, 0)):
        for kw in ({}, {'workspace': False}, {'ragged': True}):
            assert S.plan(B, N, M, ws_addr=4096, ws_bytes=1 << 20, **kw).path == NONE


def test_ragged_batches():
    for M, want in ((1, 'stream<1,16>,RAGGED'), (64, 'stream<1,16>,RAGGED'), (65, 'stream<2,16>,RAGGED'), (128, 'stream<2,16>,RAGGED'),
                    (129, 'stream<4,16>,RAGGED'), (256, 'stream<4,16>,RAGGED'), (257, 'stream<8,16>,RAGGED'), (512, 'stream<8,16>,RAGGED')):
        for N in (1, 300, 512):
            # whatever workspace is offered: the ragged launcher takes none
            for kw in ({'workspace': False}, {}):
                assert S.plan(7, N, M, ragged=True, **kw) == S.Plan(STREAMING, 'none', want, 0, 0, 0, False, 7, False), (N, M)
    # the limit of 512 keypoints per frame, either frame
    assert S.plan(7, 513, 64, ragged=True).path == NONE and S.plan(7, 64, 513, ragged=True).path == NONE
    assert S.plan(7, 512, 512, ragged=True).path == STREAMING


def test_names_and_indices():
    assert len(S.NAMES) == 15 and len(set(S.NAMES)) == 15 and len(S.INSTANTIATIONS) == 13
    assert S.NAMES.index('scaling<true,16>') == 2 and S.NAMES.index('stream<1,16>') == 3 and S.NAMES.index('stream<32,8>') == 8
    assert S.NAMES.index('stream<1,16>,RAGGED') == 9 and S.NAMES.index('stream<8,16>,RAGGED') == 12
    assert S.NAMES.index(S.GATED) == 13 and S.NAMES.index(S.EXTRACT) == 14
    assert S.counts().shape == (15,)        # (readable without a device)


def test_the_gpu_cases_reach_their_forms():
    """The shapes of tests/test_gpu_sinkhorn_forms.py: every scaling instantiation at every (GR, GC) named there, every streaming
    instantiation on its own and gated, and together all of the 13."""
    seen = set()
    for (N, M), (nm, GR, GC) in S.CLUSTER_CASES.items():
        p = S.plan(S.FORMS_BATCH, N, M)
        assert (p.path, p.scaling, p.GR, p.GC, p.ngroups, p.cooperative) == (CLUSTER, nm, GR, GC, S.FORMS_BATCH, False), (N, M, p)
        assert p.stream == S.plan(S.FORMS_BATCH, N, M, workspace=False).stream
        seen.add(p.scaling)
    for (N, M), nm in S.STREAM_CASES.items():
        p = S.plan(S.FORMS_BATCH, N, M, workspace=False)
        assert (p.path, p.stream, p.grid) == (STREAMING, nm, S.FORMS_BATCH), (N, M, p)
        seen.add(p.stream)
    assert len(S.STREAM_CASES) == 21
    for M in (64, 128, 256, 512):
        seen.add(S.plan(3, 100, M, ragged=True).stream)
    assert seen == set(S.INSTANTIATIONS)
    # the gated launches behind the cluster cases: four of the six streaming instantiations (the plan names them; one counter for all)
    assert {S.plan(3, N, M).stream for N, M in S.CLUSTER_CASES} == {'stream<1,16>', 'stream<2,16>', 'stream<16,8>', 'stream<32,8>'}


# ---- the whole rule, stated again ----
def _stream_rule(N, M):
    for lim, nm in zip((64, 128, 256, 512), S.STREAM[:4]):
        if M <= lim:
            return nm
    if N > 4096 or M > 2048:
        return None
    return S.STREAM[4] if M <= 1024 else S.STREAM[5]


def _rule(B, N, M, cus, workspace, fallback, ragged):
    none = S.Plan(NONE, 'none', 'none', 0, 0, 0, False, 0, False)
    if min(B, N, M) <= 0:
        return none
    st = _stream_rule(N, M)
    if ragged:
        return none if max(N, M) > 512 else S.Plan(STREAMING, 'none', st + ',RAGGED', 0, 0, 0, False, B, False)
    if not workspace or max(N, M) > 2048:
        return none if st is None else S.Plan(STREAMING, 'none', st, 0, 0, 0, False, B, False)
    GR, GC = -(-N // 128), -(-M // 512)
    P = GR * GC
    ngroups = min(cus // P, max(1, min(64, 256 // P)), B)
    if ngroups < 1:
        return none._replace(GR=GR, GC=GC)
    slots = -(-ngroups // 8)                                     # groups per XCD
    xcd = P * slots <= cus // 8
    form = S2D if GC > 1 else S16 if GR > 4 else S4
    return S.Plan(CLUSTER, form, st if fallback else 'none', GR, GC, ngroups, xcd, (8 * slots if xcd else ngroups) * P,
                  (not fallback) or ngroups * P > cus)


def test_the_rule_over_a_sweep():
    seen = set()
    Ns = (1, 64, 127, 128, 129, 300, 512, 513, 1024, 2048, 2049, 4096, 4097)
    Ms = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1536, 1537, 2048, 2049)
    for N in Ns:
        for M in Ms:
            for B in (1, 2, 7, 8, 9, 33, 52, 64, 65, 130):
                for cus in (256, 304, 64, 8):
                    for workspace, fallback, ragged in ((True, True, False), (True, False, False), (False, True, False), (False, True, True)):
                        got = S.plan(B, N, M, cus=cus, workspace=workspace, fallback=fallback, ragged=ragged)
                        want = _rule(B, N, M, cus, workspace and S.workspace_bytes(B, N, M) > 0, fallback, ragged)
                        assert got == want, (B, N, M, cus, workspace, fallback, ragged)
                        seen.update((got.scaling, got.stream))
                        if got.path == CLUSTER:
                            # every group's workgroups have a CU each, and no launch is cooperative while a fallback buffer exists
                            assert got.ngroups * got.GR * got.GC <= cus and got.cooperative == (not fallback)
                            assert got.grid >= got.ngroups * got.GR * got.GC
    assert seen == set(S.INSTANTIATIONS) | {'none'}
