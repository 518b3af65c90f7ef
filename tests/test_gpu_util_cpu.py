"""CPU tests of the helpers in tests/gpu_util.py that GPU assertions rest on.  count_other is what the relocated operator tests (pages above 2^31 elements of 4.3 GB
pools) use to say "every other element of the pool still holds the fill": here it runs on small CPU tensors, where every element can be changed in turn."""
import pytest
import torch

from gpu_util import count_other

FILL = 0x7FA5


@pytest.mark.parametrize("numel,lo,hi,chunk", [(50, 17, 31, 7), (50, 0, 31, 7), (50, 17, 50, 7), (50, 0, 0, 7), (50, 50, 50, 7), (50, 0, 50, 7), (64, 16, 32, 16), (50, 17, 31, 1 << 29),
                                               (50, 21, 22, 1), (3, 1, 2, 1)])
def test_count_other_counts_every_element_outside_the_window_and_none_inside(numel, lo, hi, chunk):
    pool = torch.full((numel,), FILL, dtype=torch.int16)
    assert count_other(pool, FILL, lo, hi, chunk) == 0
    for i in range(numel):                                 # ONE changed element, anywhere: 0, lo - 1, lo, hi - 1, hi, numel - 1 and every chunk boundary among them
        for v in (FILL ^ 1, 0, -1, -32768):
            pool[i] = v
            assert count_other(pool, FILL, lo, hi, chunk) == (0 if lo <= i < hi else 1), (i, v)
        pool[i] = FILL
    pool[:] = 0                                            # everything changed: exactly the window is skipped
    assert count_other(pool, FILL, lo, hi, chunk) == numel - (hi - lo)
    assert count_other(pool, 0, lo, hi, chunk) == 0


def test_count_other_takes_a_negative_pattern_and_refuses_a_window_outside_the_pool():
    sent = int(torch.tensor(-1.75, dtype=torch.bfloat16).view(torch.int16))          # decode_proj_ref.SENTINEL: bit 15 set
    assert sent < 0
    pool = torch.full((40,), -1.75, dtype=torch.bfloat16).view(torch.int16)
    assert count_other(pool, sent, 10, 20, 8) == 0
    pool[39] = sent + 1
    pool[15] = 0
    assert count_other(pool, sent, 10, 20, 8) == 1
    for lo, hi in ((-1, 5), (5, 41), (20, 10)):
        with pytest.raises(AssertionError):
            count_other(pool, sent, lo, hi)
