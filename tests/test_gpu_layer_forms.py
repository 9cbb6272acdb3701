"""Every form of the fp32-class layer kernel (csrc/layer.hip, csrc/layer_split.hip: 14 instantiations in three families) at the smallest
launch that reaches it, stage by stage against the fp64 oracle and bit for bit against the split kernel.

launch_layer picks the family by the launch size - layer_split_kernel up to mdgat_set_layer_split_tiles tiles of 128 keypoints,
layer_kernel with 64-keypoint workgroups (NW = 4) up to 128 tiles, with 128-keypoint workgroups (NW = 8) beyond - and the V^T store path by
N | M (tests/test_layer_plan.py pins the rule and holds the cases of tests/layer_forms.py to it).  A case here is one tapped forward with
L = 1 and full attention: it runs unsliced, one launch of all R = B (n + m) rows, and issues exactly one <0,1,...>, one <1,1,...> and
one <1,2,...> launch, which the launch counters confirm; the self layer reads the q / k / V^T of the first, the cross layer those of the
second, so a wrong V^T column, bias or store of either shows in x_layers.  Per case:

(a) x_enc, x_layers, mdesc, scores against the oracle (CPU, fp64) over every row of every pair, at the stage bars of
    tests/test_gpu_forward.py::test_forward_stages_golden (1e-5, 5e-5, 5e-5, 1e-4), Z at the 1e-4 north star, and no f16 range violation;
(b) the same shape on the split kernel: x_layers, mdesc, scores, Z and the matches bit for bit.

The projection-only final_proj launch <0,2,...> is issued only by the exact mode with every layer in fp64 (arithmetic='fp64',
f64_layers = 2 L): its three forms run at (131 | 3 | 3) x 61 x 66, the only layer-kernel launch of those forwards, with x_layers under
the 5e-6 of tests/test_gpu_f64.py::test_f64_stages_vs_reference, mdesc and scores at the bars above, and each layer_kernel form bit for
bit against split<0,2> on its own batch.

Measured when the file was written (MI355X; every case prints its own line) - largest error against the oracle over all cases:
    fp32 class:  x_enc 1.3e-6, x_layers 1.4e-6, mdesc 1.8e-6, scores 9.9e-6, Z 1.8e-5
    exact mode:  x_layers 1.3e-7, mdesc 1.0e-6, scores 6.4e-6, Z 9.6e-6"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import layer_forms as LF  # noqa: E402
from mdgat_matcher_amd import MDGAT, synth  # noqa: E402
from oracle import mdgat_oracle as O  # noqa: E402

DEV = 'cuda:0'
L = 1
X_ENC_TOL, X_LAYER_TOL, MDESC_TOL, SCORES_TOL, Z_TOL = 1e-5, 5e-5, 5e-5, 1e-4, 1e-4     # test_forward_stages_golden
X_LAYER_F64_TOL = 5e-6                                                                  # test_f64_stages_vs_reference
CFG = synth.default_config(L=L, k=[], sinkhorn_iterations=1)
SEED, FIRST_PAIR = 6, 17
STAGES = ('x_layers', 'mdesc', 'scores', 'Z', 'matches0', 'matches1', 'mscores0', 'mscores1')


@functools.lru_cache(maxsize=None)
def _sd():
    return synth.make_state_dict(L=L, seed=SEED)


@functools.lru_cache(maxsize=None)
def _net(exact):
    """The fp32-class module, or the exact mode's with every layer in fp64 and the fp32-class tail (final_proj, scores, Sinkhorn)."""
    cfg = {**CFG, 'arithmetic': 'fp64', 'f64_layers': 2 * L} if exact else {**CFG, 'arithmetic': 'fp32'}
    net = MDGAT(cfg).double()
    net.load_state_dict(_sd())
    net = net.double().eval().to(DEV)
    assert net.exact() == exact
    return net


@functools.lru_cache(maxsize=None)
def _data(B, n, m):
    """B pairs of n x m keypoints, every pair its own draw (CPU, fp64).  Shared and read-only."""
    return synth.make_batch(B, n, m, first_pair=FIRST_PAIR)


@functools.lru_cache(maxsize=None)
def _oracle(B, n, m):
    """The stage tensors of the fp64 oracle in the library's [B, P, 128] row layout, once per shape."""
    cap = {}
    O.mdgat_forward(_sd(), CFG, _data(B, n, m), cap)
    rows = lambda a, b: torch.cat([cap[a], cap[b]], dim=2).transpose(1, 2).contiguous()      # [B, 128, n] | [B, 128, m] -> [B, n + m, 128]
    return {'x_enc': rows('enc0', 'enc1'), 'x_layers': torch.stack([rows(f'layer{i}_desc0', f'layer{i}_desc1') for i in range(2 * L)]),
            'mdesc': rows('mdesc0', 'mdesc1'), 'scores': cap['scores'], 'Z': cap['Z']}


@functools.lru_cache(maxsize=None)
def _forward(B, n, m, how, exact=False):
    """One tapped forward under mdgat_set_layer_split_tiles forced as `how`: the taps and outputs (on the CPU) and the layer launches it
    made, once per (shape, family)."""
    net, data = _net(exact), {k: v.to(DEV) for k, v in _data(B, n, m).items()}
    P = n + m
    taps = {'x_enc': torch.empty(B, P, 128, device=DEV), 'x_layers': torch.empty(2 * L, B, P, 128, device=DEV),
            'mdesc': torch.empty(B, P, 128, device=DEV), 'scores': torch.empty(B, n, m, device=DEV)}
    with LF.forced(how), LF.watch() as w:
        m0, m1, s0, s1, Z = net._run(data['keypoints0'], data['scores0'], data['descriptors0'], data['keypoints1'], data['scores1'],
                                     data['descriptors1'], want_Z=True, taps=taps)
        torch.cuda.synchronize()
    net.check(DEV)                          # raises on an f16 range violation
    out = {k: v.cpu() for k, v in taps.items()}
    out.update(Z=Z.cpu(), matches0=m0.cpu(), matches1=m1.cpu(), mscores0=s0.cpu(), mscores1=s1.cpu())
    return out, w.launched()


@pytest.fixture(scope='module', autouse=True)
def _release_the_shared_runs():
    yield
    for f in (_forward, _oracle, _data, _net):
        f.cache_clear()
    torch.cuda.empty_cache()


def _errors(out, ref):
    e = {k: float((out[k].double() - ref[k]).abs().max()) for k in ('x_enc', 'mdesc', 'scores', 'Z')}
    e['x_layers'] = [float((out['x_layers'][i].double() - ref['x_layers'][i]).abs().max()) for i in range(2 * L)]
    return e


@pytest.mark.parametrize('case', LF.CASES, ids=LF.case_id)
def test_form_vs_oracle(case):
    fam, how, B, n, m, v_store = case
    out, launched = _forward(B, n, m, how)
    assert launched == LF.case_forms(case, L), f'{LF.case_id(case)}: wanted {LF.case_forms(case, L)}, launched {launched}'
    e = _errors(out, _oracle(B, n, m))
    print(f'[layer-forms] {LF.case_id(case)} R={B * (n + m)} v_store={v_store} {sorted(launched)}: x_enc {e["x_enc"]:.2e} x_layers '
          f'{max(e["x_layers"]):.2e} mdesc {e["mdesc"]:.2e} scores {e["scores"]:.2e} Z {e["Z"]:.2e}')
    assert all(torch.isfinite(out[k]).all() for k in ('x_enc', 'x_layers', 'mdesc', 'scores', 'Z'))
    assert e['x_enc'] < X_ENC_TOL, e
    assert max(e['x_layers']) < X_LAYER_TOL, e
    assert e['mdesc'] < MDESC_TOL, e
    assert e['scores'] < SCORES_TOL, e
    assert e['Z'] < Z_TOL, e


@pytest.mark.parametrize('case', [c for c in LF.CASES if c[0] != 'split'], ids=LF.case_id)
def test_form_equals_split_kernel(case):
    """The project's "same arithmetic to the bit" claim for every layer_kernel form: NW = 8 included, all four V^T paths."""
    fam, how, B, n, m, v_store = case
    out, launched = _forward(B, n, m, how)
    split, launched_split = _forward(B, n, m, 'split')
    assert launched == LF.case_forms(case, L)
    assert launched_split == LF.case_forms(('split',) + case[1:], L), launched_split
    for k in STAGES:
        assert torch.equal(out[k], split[k]), (k, float((out[k].double() - split[k].double()).abs().max()))


@pytest.mark.parametrize('case', LF.CASES_F64, ids=LF.case_id)
def test_final_proj_only_form_vs_oracle(case):
    fam, how, B, n, m = case
    out, launched = _forward(B, n, m, how, exact=True)
    assert launched == {LF.form_name(fam, 0, 2): 1}, launched       # the only layer-kernel launch of the forward
    e = _errors(out, _oracle(B, n, m))
    print(f'[layer-forms] exact {LF.case_id(case)} {sorted(launched)}: x_enc {e["x_enc"]:.2e} x_layers {max(e["x_layers"]):.2e} '
          f'mdesc {e["mdesc"]:.2e} scores {e["scores"]:.2e} Z {e["Z"]:.2e}')
    assert max(e['x_layers']) < X_LAYER_F64_TOL, e
    assert e['mdesc'] < MDESC_TOL, e
    assert e['scores'] < SCORES_TOL, e
    assert e['Z'] < Z_TOL, e


def test_final_proj_only_forms_agree_bit_for_bit():
    """mdesc (and what follows from it) of the three <0,2,...> forms, each layer_kernel form against split<0,2> on its own batch: the fp64
    layers in front choose their own kernels by the batch size, so only forwards of the same batch hand the same x over."""
    for fam, how, B, n, m in LF.CASES_F64:
        if fam == 'split':
            continue
        out, launched = _forward(B, n, m, how, exact=True)
        split, launched_split = _forward(B, n, m, 'split', exact=True)
        assert launched == {LF.form_name(fam, 0, 2): 1} and launched_split == {'split<0,2>': 1}, (launched, launched_split)
        for k in STAGES:
            assert torch.equal(out[k], split[k]), (fam, k, float((out[k].double() - split[k].double()).abs().max()))


def test_every_form_is_launched_by_this_file():
    """All 14 counters move across the cases above (runs shared with them where they have been made)."""
    seen = {}
    for c in LF.CASES:
        for nm, k in _forward(*c[2:5], c[1])[1].items():
            seen[nm] = seen.get(nm, 0) + k
    for c in LF.CASES_F64:
        for nm, k in _forward(*c[2:], c[1], exact=True)[1].items():
            seen[nm] = seen.get(nm, 0) + k
    assert set(seen) == set(LF.NAMES), sorted(set(LF.NAMES) - set(seen))
