"""The chunks the split form of the fp32 Sinkhorn is tested on (test_gpu_ragged_sinkhorn_split.py), their oracle, and which of their
pairs the oracle decides (ragged_decided.py; checked on the CPU by test_ragged_sinkhorn_split.py).  L = 1 without a dynamic layer: the
only discontinuity behind the Sinkhorn is the extraction's arg-max, so a pair is decided by its smallest margin on Z alone.

    A   slot 130 x 70, G = 2: the second slab holds 2, 0, 1 and 0 rows of its pairs
    B   slot 512 x 500, G = 4: every slab full, a slab cut at row 385 (one row in the last), slabs 1 .. 3 empty

The seeds (SEED: the first pair index synth.make_batch starts from) were chosen, by the oracle alone, so that at least half of each chunk
is decided at every iteration count."""
import functools

from mdgat_matcher_amd import synth

import ragged_decided as RD

CHUNKS = {'A': ((130, 70), (128, 64), (129, 33), (16, 70)), 'B': ((512, 500), (385, 257), (100, 64))}
ITERS = {'A': (1, 2, 3, 20), 'B': (100,)}
SEED = {'A': 0, 'B': 0}
L = 1
# (chunk, iterations) -> the pairs the oracle decides
# (margins: A 4.4e-4, 2.2e-4, 3.1e-7, 5.9e-3 after one iteration; 1.3e-3, 6.4e-4, 7.8e-6, 5.4e-3 after two; 8.0e-4, 1.5e-3, 7.3e-5, 5.3e-2
# after three; 8.5e-4, 3.1e-3, 8.8e-3, 1.2e-2 after twenty.  B 4.5e-4, 2.2e-3, 1.6e-3)
DECIDED = {('A', 1): (0, 1, 3), ('A', 2): (0, 1, 3), ('A', 3): (0, 1, 3), ('A', 20): (0, 1, 2, 3), ('B', 100): (0, 1, 2)}


def cfg(iters, **over):
    return synth.default_config(L=L, k=[], sinkhorn_iterations=iters, **over)


def state_dict():
    return synth.make_state_dict(L=L, seed=1)


@functools.lru_cache(maxsize=None)
def pairs(name, device='cpu'):
    """the per-pair dicts of a chunk as a batch_size=1 loader yields them"""
    return tuple({k: v.to(device) for k, v in synth.make_batch(1, n, m, first_pair=SEED[name] + b).items()} for b, (n, m) in enumerate(CHUNKS[name]))


@functools.lru_cache(maxsize=None)
def oracle(name, iters):
    """the fp64 oracle on every pair of the chunk alone, once: (outputs, Z, smallest top-k gap - inf: no dynamic layer -, smallest arg-max
    margin) per pair"""
    out = []
    for p in pairs(name):
        ref, cap, gap, margin = RD.oracle_pair(state_dict(), cfg(iters), p)
        out.append((ref, cap['Z'], gap, margin))
    return tuple(out)
