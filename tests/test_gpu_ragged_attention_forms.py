"""Every RAGGED instantiation the fp32-class attention launcher can reach (ops.attention with counts=), each at the smallest slots that reach
it: the launch counters move as mdgat_attention_ragged_plan says - the plan and the launch are one decision (csrc/attention.hip:
attention_plan, launch_attention).  Thirteen launches: the eight forms of attention_kernel within 512 x 512, and with wide=True the windowed
one and the four wide ones, which alone move the ragged-wide counters.  B = 2, one pair filling its slots and one short.  The values are the
subject of tests/test_gpu_ragged_attention_fp32.py and tests/test_gpu_ragged_attention_fp32_wide.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_forms as AF  # noqa: E402
from mdgat_matcher_amd import ops  # noqa: E402

DEV = 'cuda:0'
K = 8       # at most the shortest count below
# (slots, the short pair, wide) -> the forms reached: full, dynamic (then also with the tap)
SLOTS = [
    ((33, 31), (9, 12), False, 'full<4>', 'dyn<4>'),                    # 2 key blocks (the smallest slots past one)
    ((130, 129), (40, 9), False, 'full<8>', 'dyn<8>'),                  # 5
    ((257, 258), (9, 100), False, None, 'dyn<16>'),                     # 9 (full: full<8> again)
    ((513, 40), (100, 9), True, 'full<8,windowed>', 'wide<4>'),         # 17
    ((1025, 40), (300, 9), True, None, 'wide<8>'),                      # 33 (full: the windowed kernel again)
]
CASES = [(slots, short, wide, form, k, tap) for slots, short, wide, full, dyn in SLOTS
         for form, k, tap in ((full, 0, False), (dyn, K, False), (dyn, K, True)) if form]
# the ragged-wide counter (ops.RAGGED_WIDE_LAUNCHES) of the forms only a wide slot reaches
WIDE_COUNTER = {'full<8,windowed>': 'full<8>,windowed,RAGGED', 'wide<4>': 'wide<4>,RAGGED', 'wide<4>,TAP': 'wide<4>,TAP,RAGGED',
                'wide<8>': 'wide<8>,RAGGED', 'wide<8>,TAP': 'wide<8>,TAP,RAGGED'}


def test_the_cases_are_the_thirteen_ragged_forms():
    names = [AF.NAMES[AF.index(form, tap)] for _, _, _, form, _, tap in CASES]
    assert len(names) == 13 and len(set(names)) == 13
    assert {n.replace(',TAP', '') for n in names} == set(AF.RAGGED)
    assert [n for n in names if n in WIDE_COUNTER] == names[-5:] and set(names[-5:]) == set(WIDE_COUNTER)


@pytest.mark.parametrize('slots,short,wide,form,k,tap', CASES, ids=[f'{AF.NAMES[AF.index(c[3], c[5])]}-{c[0][0]}x{c[0][1]}' for c in CASES])
def test_the_launch_counters_move_as_the_plan_says(slots, short, wide, form, k, tap):
    (Np, Mp), B = slots, 2
    planned, split, tiles = AF.ragged_plan(B, Np, Mp, k, tap, wide)
    assert AF.name(planned) == AF.NAMES[AF.index(form, tap)] and split >= 1 and tiles >= 1
    qkv = torch.randn(B, Np + Mp, 3, 4, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(Np + k)).to(DEV)
    before = ops.ragged_wide_launches()
    with AF.watch() as w:
        ops.attention(qkv, Np, Mp, True, topk=k, return_selection=tap, counts=([Np, short[0]], [Mp, short[1]]), wide=wide)
    torch.cuda.synchronize()
    AF.assert_launched(w, planned, f'ragged {Np} x {Mp} k={k} tap={tap} wide={wide}')
    after = ops.ragged_wide_launches()
    moved = {n: after[n] - before[n] for n in after if after[n] != before[n]}
    assert moved == ({WIDE_COUNTER[AF.name(planned)]: 1} if AF.name(planned) in WIDE_COUNTER else {}), moved
