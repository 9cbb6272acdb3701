"""The ten instantiations of gemm_f64_kernel (csrc/f64.hip) as the tests name them, and the two symbols that make the launcher's choice
observable: mdgat_gemm_f64_plan (the choice as a pure function; no device) and mdgat_gemm_f64_launches (launches so far by index).

Index = 5 * bnt + form; form: 0 <2,slow>, 1 <2,fast,32>, 2 <2,fast,64>, 3 <4,slow>, 4 <4,fast> (<WN, FAST, KC>: 64 x 32 WN tiles, whole-tile
16-byte copies or guarded 8-byte ones, chunks of KC); bnt: the A operand is bn_relu of what is loaded."""
import ctypes as C

import numpy as np

FORMS = ('<2,slow>', '<2,fast,32>', '<2,fast,64>', '<4,slow>', '<4,fast>')
NAMES = FORMS + tuple(f[:-1] + ',BNT>' for f in FORMS)


def index(form, bnt=False):
    return 5 * int(bnt) + FORMS.index(form)


def _lib():
    from mdgat_matcher_amd import _lib
    return _lib.load()


def plan(M, N, K, K0=None, batch=1, aligned=True, bnt=False, cus=256):
    """The index launch_gemm_f64 chooses (-1: no launch).  K0: columns of the first source (default: a single source)."""
    return _lib().mdgat_gemm_f64_plan(M, N, K, K if K0 is None else K0, batch, int(aligned), int(bnt), cus)


def counts():
    buf = (C.c_uint64 * 10)()
    _lib().mdgat_gemm_f64_launches(buf)
    return np.array(list(buf), dtype=np.int64)


class watch:
    """``with watch() as w: ...`` - afterwards w.delta[i] = launches of instantiation i in between (as numpy int64 [10])."""

    def __enter__(self):
        self.before = counts()
        self.delta = None
        return self

    def __exit__(self, *exc):
        self.delta = counts() - self.before

    def launched(self):
        return {NAMES[i]: int(n) for i, n in enumerate(self.delta) if n}


def cu_count(device=0):
    import torch
    return torch.cuda.get_device_properties(device).multi_processor_count


def pick(candidates, want, cus, shape):
    """The first of ``candidates`` for which the plan names instantiation ``want`` on a device of ``cus`` compute units;
    ``shape(candidate)`` = the keyword arguments of ``plan``.  No candidate: the case fails, with the CU count in the message."""
    for c in candidates:
        if plan(cus=cus, **shape(c)) == want:
            return c
    raise AssertionError(f'no candidate of {list(candidates)} reaches {NAMES[want]} on a device of {cus} CUs: '
                         f'{[NAMES[plan(cus=cus, **shape(c))] for c in candidates]}')


def assert_launched(w, want, cus, what, times=1):
    """The watched region launched instantiation ``want`` exactly ``times`` times."""
    assert w.delta[want] == times, f'{what}: wanted {times} x {NAMES[want]}, launched {w.launched()} on a device of {cus} CUs'


# ---- the shapes that reach each instantiation (tests/test_gpu_gemm_f64.py, tests/test_gpu_mlp_grad.py, tests/test_gpu_head_grad.py) ----
# The first candidate of every list is the shape worked by hand for 256 CUs (tests/test_gemm_f64_plan.py pins it); the others serve devices of
# other CU counts (partitions of 32, 64 and 128 CUs; 304).  The <4,.> forms need a launch whose narrow tiles take two rounds of resident
# workgroups (4 per CU) while its wide tiles take one (3 per CU): at 256 CUs 33 row tiles x 2048 columns make tn = 1056 > 1024, tw = 528 <= 768.

# (a) plain products through mdgat_pointwise_f64: form -> candidates (M, N, K)
PLAIN = {'<2,slow>': [(65, 48, 33)],
         '<2,fast,64>': [(64, 64, 64)],
         '<2,fast,32>': [(64, 64, 96)],
         '<4,fast>': [(2112, 2048, 32), (2560, 2048, 32), (4160, 2048, 32)],
         '<4,slow>': [(2100, 2048, 36), (2548, 2048, 36), (4148, 2048, 36)]}
# ... and the wide general form ragged in every dimension: N no multiple of its 128-column tile, K no multiple of the 4-deep matrix step
# (the table's 2100 x 2048 x 36 is ragged in M and in the chunk only)
WIDE_RAGGED = [(2100, 2000, 35), (2548, 2000, 35), (4148, 2000, 35)]

# (d) a bare convolution of two sources, 64 outputs: (K0, K1, rows) -> the forward product's form
TWO_SOURCE = {(32, 32, 64): '<2,fast,32>', (64, 64, 64): '<2,fast,64>', (40, 24, 64): '<2,slow>', (40, 24, 70): '<2,slow>',
              (8, 56, 64): '<2,slow>', (8, 56, 70): '<2,slow>'}

# (d) the product behind a BatchNorm, as the second convolution of a two-convolution stack: name -> (channels, candidate rows, form)
BNT = {'fast32': ((16, 96, 64), [64], '<2,fast,32>'),
       'fast64': ((16, 64, 64), [64], '<2,fast,64>'),
       'slow': ((16, 96, 64), [65], '<2,slow>'),
       'wide_fast': ((16, 32, 512), [8256, 10304, 16448], '<4,fast>'),
       'wide_slow': ((16, 32, 512), [8250, 10300, 16440], '<4,slow>')}

# (e) the score matrix of ops.match_head, `batch` products of N x M x 128: the parametrized (B, N, M) -> (form, candidate B)
BATCHED = {(5, 512, 512): ('<2,fast,32>', [5, 2]),
           (17, 512, 512): ('<4,fast>', [17, 9, 21]),
           (17, 512, 500): ('<4,slow>', [17, 9, 21])}
