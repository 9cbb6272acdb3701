"""Every form of the fp64 layer-tail and encoder kernels (csrc/layer_f64.hip: layer_tail_f64_kernel<1 | 2>, layer_tail_f64_cluster_kernel,
encoder_f64_kernel<1 | 2>) at the smallest launch that reaches it and each edge of it, with the launch counters as witnesses of what ran.

A case (tests/layer_f64_forms.py: the table and what each row is there for) is one tapped forward of an exact-mode network - tapped, so
the batch is not sliced and every launch has R = B (n + m) rows - under the mdgat_set_f64_layer_fusion mode the case names.  Before the
run the plan (mdgat_layer_f64_plan at the device's CU count) must name the case's forms; after it the counters must show exactly those,
the planned number of times, and no other.  The shapes are written for 256 compute units: on another device the cases skip
(tests/test_layer_f64_plan.py sweeps other counts through the plan).  Per case:

(a) the same network under mode 0 - one gemm_f64_kernel launch per product, which its own counters confirm - gives the same bits:
    matches, match scores, Z and the fp32 taps of the encoder output and of every layer's x (torch.equal: the kernels walk every
    accumulator through k in the product kernel's order, csrc/layer_f64.hip).  Cases of at most 1100 rows are also held to the fp64
    oracle on the CPU, at the bars of tests/test_gpu_f64.py::test_f64_stages_vs_reference (x_enc 2e-6, fp64 layers 5e-6, Z 2e-5) and,
    for the layers the fp32-class kernels run behind a hand-over, of tests/test_gpu_layer_forms.py (5e-5), so that the mode-0 run is
    itself anchored outside the library;
(b) cluster_ragged, tail32_auto, tail32_half: pair 0's rows of x_enc and of every layer are those of pair 0 run alone, bit for bit (alone
    the pair of the first two is 12 or 16 blocks and clustered; that of the third, R % 32 = 9, keeps the forced 32 rows). Full attention is held to its split-key form for both runs, which is the
    one whose sums do not depend on the batch (mdgat_set_f64_attention_form); Z is not compared here - the product kernel behind the last
    layer chooses its tiling by the launch's rows;
(c) the same call again gives the same bits; the clustered cases run three times in a row on one handle - the epoch advances, the flags
    of the call before are still set - and each run equals the first.

The clustered kernel's cross-XCD branch (publish through agent-scope stores when the four workgroups of a block do not share an XCD) is
reached by no test: where the hardware places workgroups cannot be chosen from outside.

Measured when the file was written (MI355X, 256 CUs; every case prints its own line) - largest error against the oracle over the cases:
    x_enc 2.4e-07, fp64 layers 2.4e-07, fp32-class layers behind a hand-over 8.9e-07, Z 9.5e-07 behind the fp64 tail (one fp32 rounding of
    the output) and 8.0e-06 behind the fp32-class one"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import layer_f64_forms as LF  # noqa: E402
from mdgat_matcher_amd import MDGAT, _lib, synth  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402
from test_gpu_f64 import X_ENC_STAGE_TOL, X_LAYER_STAGE_TOL, Z_STAGE_TOL  # noqa: E402
from test_gpu_layer_forms import X_LAYER_F64_TOL, X_LAYER_TOL  # noqa: E402

DEV = 'cuda:0'
SEED, FIRST_PAIR, ITERS = 21, 40, 10
OUTS = ('matches0', 'matches1', 'mscores0', 'mscores1', 'Z', 'x_enc', 'x_layers')
CLUSTER_CASES = [c for c in LF.CASES if c.tail_form == LF.CLUSTER]
assert X_LAYER_F64_TOL == X_LAYER_STAGE_TOL      # (one bar, stated in both files)


def _need_the_device_of_the_table():
    cus = LF.cu_count()
    if cus != LF.CASE_CUS:
        pytest.skip(f'the case table is written for {LF.CASE_CUS} compute units, this device reports {cus}')


def _cfg(case):
    over = {'sinkhorn_arithmetic': 'fp32'} if case.tail == 'fp32' else {}
    return synth.default_config(L=case.L, k=list(case.k), sinkhorn_iterations=ITERS, **over)


@functools.lru_cache(maxsize=None)
def _net(L, k, tail):
    case = LF.Case('net', 0, 0, 0, 1, L, list(k), tail, None, None, False)
    net = MDGAT(_cfg(case)).double()
    net.load_state_dict(synth.make_state_dict(L=L, seed=SEED))
    net = net.eval().to(DEV)
    assert net.exact()
    return net


@functools.lru_cache(maxsize=None)
def _data(B, n, m):
    """B pairs of n x m keypoints, every pair its own draw (CPU, fp64).  Shared and read-only."""
    return synth.make_batch(B, n, m, first_pair=FIRST_PAIR)


def _forward(case, mode, B=None, attention_form=None):
    """One tapped forward of the first B pairs of a case (default: all) under `mode`: outputs and taps (CPU) and what the counters saw."""
    B = case.B if B is None else B
    net, P = _net(case.L, tuple(case.k), case.tail), case.n + case.m
    d = {k: v[:B].to(DEV) for k, v in _data(case.B, case.n, case.m).items()}
    taps = {'x_enc': torch.zeros(B, P, 128, device=DEV), 'x_layers': torch.zeros(2 * case.L, B, P, 128, device=DEV)}
    lib = _lib.load()
    prev_form = lib.mdgat_set_f64_attention_form(attention_form) if attention_form is not None else None
    try:
        with LF.fusion(mode), LF.watch() as w:
            m0, m1, s0, s1, Z = net._run(d['keypoints0'], d['scores0'], d['descriptors0'], d['keypoints1'], d['scores1'], d['descriptors1'],
                                         want_Z=True, taps=taps)
            torch.cuda.synchronize()
    finally:
        if attention_form is not None:
            lib.mdgat_set_f64_attention_form(prev_form)
    net.check(DEV)                      # raises when a kernel raised the range guard (a cluster partner that never answered included)
    out = dict(zip(OUTS, (t.cpu() for t in (m0, m1, s0, s1, Z, taps['x_enc'], taps['x_layers']))))
    return out, w.launched()


@functools.lru_cache(maxsize=None)
def _fused(case_id):
    case = next(c for c in LF.CASES if c.id == case_id)
    return _forward(case, case.mode)


@functools.lru_cache(maxsize=None)
def _oracle(case_id):
    """x_enc, x_layers and Z of the fp64 oracle in the library's [B, P, 128] row layout, once per case."""
    case = next(c for c in LF.CASES if c.id == case_id)
    cap = {}
    O.mdgat_forward(synth.make_state_dict(L=case.L, seed=SEED), _cfg(case), _data(case.B, case.n, case.m), cap)
    rows = lambda a, b: torch.cat([cap[a], cap[b]], dim=2).transpose(1, 2).contiguous()
    return {'x_enc': rows('enc0', 'enc1'), 'x_layers': torch.stack([rows(f'layer{i}_desc0', f'layer{i}_desc1') for i in range(2 * case.L)]),
            'Z': cap['Z']}


@pytest.fixture(scope='module', autouse=True)
def _release_the_shared_runs():
    yield
    for f in (_fused, _oracle, _data, _net):
        f.cache_clear()
    torch.cuda.empty_cache()


def _assert_same_bits(a, b, what, keys=OUTS, rows=slice(None)):
    for k in keys:
        x, y = (t[k][:, rows] if k == 'x_layers' else t[k][rows] for t in (a, b))
        assert torch.equal(x, y), (what, k, float((x.double() - y.double()).abs().max()))


@pytest.mark.parametrize('case', LF.CASES, ids=lambda c: c.id)
def test_form_equals_three_launches(case):
    _need_the_device_of_the_table()
    cus, R, first = LF.cu_count(), case.B * (case.n + case.m), LF.f64_layers(case)
    # before the launch: the plan names the forms the case is written for
    want = LF.case_forms(case, cus)
    assert want == {case.encoder_form: 1, **({case.tail_form: first} if first else {})}, LF.named(want)
    out, ran = _fused(case.id)
    assert ran == want, f'{case.id}: planned {LF.named(want)}, launched {LF.named(ran)}'
    ref, ran_ref = _forward(case, 0)
    assert ran_ref == LF.case_forms(case, cus, mode=0) and set(ran_ref) <= {LF.TAIL_GEMMS, LF.ENC_GEMMS}, LF.named(ran_ref)
    line = (f'[layer-f64-forms] {case.id} mode {case.mode} R={R}: ' +
            ', '.join(f'{LF.NAMES[f]} x{t} ({LF.plan(R, f >= LF.ENC16, mode=case.mode, cus=cus)[1]} workgroups)' for f, t in sorted(ran.items())))
    err = None
    if R <= LF.ORACLE_MAX_ROWS:
        o = _oracle(case.id)
        err = {'x_enc': float((out['x_enc'].double() - o['x_enc']).abs().max()), 'Z': float((out['Z'].double() - o['Z']).abs().max()),
               'x_layers': [float((out['x_layers'][i].double() - o['x_layers'][i]).abs().max()) for i in range(2 * case.L)]}
        line += f'; vs oracle x_enc {err["x_enc"]:.2e} x_layers ' + ' '.join(f'{e:.2e}' for e in err['x_layers']) + f' Z {err["Z"]:.2e}'
    print(line)
    assert all(torch.isfinite(out[k]).all() for k in ('x_enc', 'x_layers', 'Z'))
    _assert_same_bits(ref, out, case.id)
    if err is not None:
        assert err['x_enc'] < X_ENC_STAGE_TOL, err
        for i, e in enumerate(err['x_layers']):
            assert e < (X_LAYER_STAGE_TOL if i < first else X_LAYER_TOL), (i, first, err)
        assert err['Z'] < Z_STAGE_TOL, err


@pytest.mark.parametrize('case', [c for c in LF.CASES if c.alone], ids=lambda c: c.id)
def test_pair_zero_does_not_depend_on_the_batch(case):
    _need_the_device_of_the_table()
    batch, ran = _forward(case, case.mode, attention_form=0)
    alone, ran_alone = _forward(case, case.mode, B=1, attention_form=0)
    assert ran == LF.case_forms(case, LF.cu_count()), LF.named(ran)
    one = case._replace(B=1)
    assert ran_alone == LF.case_forms(one, LF.cu_count()), LF.named(ran_alone)
    print(f'[layer-f64-forms] {case.id}: in the batch {LF.named(ran)}, pair 0 alone {LF.named(ran_alone)}')
    _assert_same_bits(alone, batch, case.id, keys=('x_enc', 'x_layers'), rows=slice(0, 1))


@pytest.mark.parametrize('case', LF.CASES, ids=lambda c: c.id)
def test_the_same_call_again_gives_the_same_bits(case):
    _need_the_device_of_the_table()
    first, ran = _fused(case.id)
    for again in range(2 if case in CLUSTER_CASES else 1):
        out, ran_again = _forward(case, case.mode)
        assert ran_again == ran, (again, LF.named(ran_again))
        _assert_same_bits(first, out, (case.id, again))


def test_every_form_is_run_by_this_file():
    """All seven counters move across the cases above (their runs are shared; the mode-0 form by one small run of its own)."""
    _need_the_device_of_the_table()
    seen = set()
    for c in LF.CASES:
        seen |= set(_fused(c.id)[1])
    seen |= set(_forward(next(c for c in LF.CASES if c.id == 'cluster_one'), 0)[1])
    assert seen == set(range(len(LF.NAMES))), [LF.NAMES[i] for i in sorted(set(range(len(LF.NAMES))) - seen)]
