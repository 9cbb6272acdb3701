"""config['ragged_arithmetic'] = 'module': every ragged entry - forward_ragged / evaluate_ragged and the bank's match_frames_ragged /
evaluate_frames_ragged - runs the arithmetic the module's forward runs, for all three FPFH descriptors.  What is accepted and what is
refused before anything looks for a device (CPU tensors throughout), and the shared float32 normalisation of csrc/fpfh_norm.hpp on the
host: a stand-alone program against the reference loader's own descriptors (tests/golden/aux_loader.npz)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from mdgat_matcher_amd import MDGAT, ops, synth

K = [8, None, 8, None]
PAIRS = [(16, 16), (20, 12)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(dtype=torch.float32, **over):
    cfg = synth.default_config(L=2, k=K, sinkhorn_iterations=20, **{'ragged_arithmetic': 'module', **over})
    net = MDGAT(cfg)
    net.load_state_dict(synth.make_state_dict(L=2, seed=1, descriptor=cfg['descriptor']))
    return net.to(dtype).eval()


def _pairs(counts):
    return [synth.make_batch(1, n, m, first_pair=b) for b, (n, m) in enumerate(counts)]


def _bank(counts=(16, 20)):
    rs = np.random.RandomState(5)
    return ops.pack_frames([rs.standard_normal((n, 37)).astype(np.float32) for n in counts], device='cpu')


def test_module_is_accepted_and_garbage_is_not():
    assert _net().ragged_arithmetic == 'module'
    for value in ('fp32', 'modul', 'Module'):
        with pytest.raises(ValueError, match='ragged_arithmetic'):
            _net(ragged_arithmetic=value)


def test_the_environment_stands_in_for_modules_without_the_key(monkeypatch):
    monkeypatch.setenv('MDGAT_RAGGED_ARITHMETIC', 'module')
    cfg = synth.default_config(L=2, k=K, sinkhorn_iterations=20)
    net = MDGAT(cfg).float().eval()
    assert net.ragged_arithmetic == 'module' and net._ragged_fp32() and net._ragged_module()
    assert not MDGAT({**cfg, 'ragged_arithmetic': 'exact'}).float()._ragged_fp32()
    assert not MDGAT({**cfg, 'ragged_arithmetic': 'auto'}).float()._ragged_module()


def test_ragged_fp32_is_true_for_auto_and_module_on_a_module_that_is_not_exact():
    for value, want in (('exact', False), ('auto', True), ('module', True)):
        assert _net(ragged_arithmetic=value)._ragged_fp32() is want
        assert _net(torch.float64, arithmetic='fp32', ragged_arithmetic=value)._ragged_fp32() is want
        assert _net(torch.float64, ragged_arithmetic=value)._ragged_fp32() is False            # an exact module


def test_an_exact_module_with_the_key_stays_exact():
    net = _net(torch.float64)
    assert net.exact() and not net._ragged_fp32() and not net._ragged_module()
    with pytest.raises(ValueError, match='pair 0 has 576 x 16 keypoints: ragged batches hold at most 575'):
        net.forward_ragged(_pairs([(576, 16), (16, 16)]))


@pytest.mark.parametrize('descriptor', ['FPFH', 'FPFH_only', 'FPFH_gloabal'])
def test_every_descriptor_gets_as_far_as_the_device(descriptor):
    """a float32 module of any of the three descriptors passes every refusal; on CPU tensors the next thing it wants is a device"""
    for net in (_net(descriptor=descriptor), _net(torch.float64, arithmetic='fp32', descriptor=descriptor)):
        assert net._ragged_fp32() and net._handle_f64() == (descriptor == 'FPFH_gloabal')
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            net.forward_ragged(_pairs(PAIRS))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            net.evaluate_ragged([dict(p, gt_matches0=torch.full((1, n), -1), gt_matches1=torch.full((1, m), -1))
                                 for p, (n, m) in zip(_pairs(PAIRS), PAIRS)])
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            net.match_frames_ragged(_bank(), [0], [1])
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            net.evaluate_frames_ragged(_bank(), [0], [1], None, None)


def test_train_mode_the_evaluation_loss_and_single_f16_attention_are_refused():
    for net in (_net().train(), _net(eval_loss=True)):
        with pytest.raises(NotImplementedError, match='eval\\(\\) mode, without the evaluation loss'):
            net.forward_ragged(_pairs(PAIRS))
        with pytest.raises(NotImplementedError, match='eval\\(\\) mode, without the evaluation loss'):
            net.match_frames_ragged(_bank(), [0], [1])
    net = _net(attention_dtype='f16')
    with pytest.raises(NotImplementedError, match="attention_dtype='fp32'"):
        net.forward_ragged(_pairs(PAIRS))
    with pytest.raises(NotImplementedError, match="attention_dtype='fp32'"):
        net.match_frames_ragged(_bank(), [0], [1])


def test_more_than_512_keypoints_and_a_count_below_a_layers_k():
    net = _net()
    with pytest.raises(ValueError, match='pair 1 has 16 x 513 keypoints: ragged batches hold at most 512 per frame'):
        net.forward_ragged(_pairs([(16, 16), (16, 513)]))
    with pytest.raises(ValueError, match='pair 1 has 20 x 7 keypoints: fewer than a dynamic layer keeps'):
        net.forward_ragged(_pairs([(16, 16), (20, 7), (9, 9)]))
    bank = _bank((513, 16, 7, 20))
    with pytest.raises(ValueError, match='pair 1 has 513 x 16 keypoints: ragged batches hold at most 512 per frame'):
        net.match_frames_ragged(bank, [1, 0], [3, 1])
    with pytest.raises(ValueError, match='pair 0 has 20 x 7 keypoints: fewer than a dynamic layer keeps'):
        net.evaluate_frames_ragged(bank, [3], [2], None, None)


def test_an_empty_frame_gets_the_early_out_without_a_device():
    net = _net()
    got = net.match_frames_ragged(_bank((0, 16)), [0], [1])
    assert got[0]['skip_train'] is True and (got[0]['matches1'] == -1).all() and got[0]['matches1'].numel() == 16


# ---------------------------------------------------------------------------------------------- csrc/fpfh_norm.hpp on the host
HOST_MAIN = r'''
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#define __device__
#define __forceinline__ inline
#include "fpfh_norm.hpp"
// argv[1]: n rows of 33 float32 (the records' FPFH part), argv[2]: n rows of 33 float32 (the loader's normalised descriptors)
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::vector<float> in, want;
    for (int i = 0; i < 2; ++i) {
        FILE* f = std::fopen(argv[1 + i], "rb");
        if (!f) return 2;
        std::vector<float>& v = i ? want : in;
        float buf[33];
        while (std::fread(buf, sizeof(float), 33, f) == 33) v.insert(v.end(), buf, buf + 33);
        std::fclose(f);
    }
    if (in.size() != want.size() || in.empty()) return 2;
    long bad = 0;
    for (size_t r = 0; r < in.size() / 33; ++r) {
        const float inv = fpfh_inv_norm(&in[r * 33]);
        for (int c = 0; c < 33; ++c) {
            volatile float p = in[r * 33 + c] * inv;
            const float q = p;
            bad += std::memcmp(&q, &want[r * 33 + c], sizeof(float)) != 0;
        }
    }
    const float zeros[33] = {};
    if (!std::isinf(fpfh_inv_norm(zeros))) return 3;          // (an all-zero row: what the guard tests)
    std::printf("%zu rows, %ld words differ\n", in.size() / 33, bad);
    return bad ? 1 : 0;
}
'''


def test_the_shared_normalisation_gives_the_reference_loaders_bits_on_the_host(tmp_path, golden_dir):
    """The inverse-norm body that f64.hip's assemble kernels and the encoder's bank form share, compiled for the host with the address
    and undefined-behaviour sanitizers where the compiler has them, against every FPFH row of the loader fixture.  (The loader's
    descriptors are float32 values widened to float64: narrowing them is exact.)"""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    g = np.load(os.path.join(golden_dir, 'aux_loader.npz'))
    rows_in, rows_want = [], []
    for j in range(int(g['n_items'])):
        for f in (0, 1):
            rows_in.append(g[f'item{j}_rec{f}'][:, 4:])
            want = g[f'item{j}_descriptors{f}']
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
            rows_want.append(want.astype(np.float32))
    np.concatenate(rows_in).astype(np.float32).tofile(tmp_path / 'in.bin')
    np.concatenate(rows_want).tofile(tmp_path / 'want.bin')
    (tmp_path / 'main.cpp').write_text(HOST_MAIN)
    base = [cxx, '-O2', '-std=c++17', '-ffp-contract=off', '-I', os.path.join(ROOT, 'mdgat_matcher_amd', 'csrc'), str(tmp_path / 'main.cpp')]
    exe = str(tmp_path / 'fpfh_norm_host')
    if subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe], capture_output=True).returncode != 0:
        subprocess.run(base + ['-o', exe], check=True, capture_output=True)          # (a compiler without the sanitizer runtimes)
    run = subprocess.run([exe, str(tmp_path / 'in.bin'), str(tmp_path / 'want.bin')], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
