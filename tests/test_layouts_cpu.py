"""tests/layouts.py on CPU tensors: the views have the stated stride, alignment and poison, and the checker sees a
touched sentinel, a touched input and a touched element in front of an `offset` base."""
import math

import pytest
import torch

import layouts

_DTYPES = (torch.float32, torch.float64, torch.bfloat16)
_SHAPES = ((5, 256), (7, 100), (3, 513), (1, 48), (4, 1))


@pytest.mark.parametrize("dtype", _DTYPES, ids=str)
@pytest.mark.parametrize("layout", layouts.LAYOUTS)
def test_views_have_the_stated_stride_alignment_and_poison(layout, dtype):
    vec = 8 if dtype == torch.bfloat16 else 4
    for rows, cols in _SHAPES:
        t = torch.arange(rows * cols, dtype=torch.float32).view(rows, cols).to(dtype)
        p = layouts.place(t, layout, float("nan"))
        v, ld = p.view, p.ld
        assert tuple(v.shape) == (rows, cols) and v.stride(1) == 1 and (rows == 1 or v.stride(0) == ld) and ld >= cols
        assert torch.equal(v, t)
        if layout == "natural":
            assert ld == cols and v.data_ptr() % 16 == 0 and v.is_contiguous()
        elif layout == "pitched":
            assert ld % vec == 0 and ld == (cols + vec - 1) // vec * vec + 8 and ld != cols and v.data_ptr() % 16 == 0
        elif layout == "odd":
            assert ld % 4 != 0 and ld - cols in (3, 5) and v.data_ptr() % 16 == 0
        else:
            assert ld % vec == 0 and ld > cols and v.data_ptr() % 16 == t.element_size()
            assert v.data_ptr() - p.buffer.data_ptr() == t.element_size() and math.isnan(float(p.buffer[0]))
        # every element of the buffer that is not the operand is poison
        whole = p.buffer[p.front:].view(rows, ld)
        assert p.buffer.numel() == p.front + rows * ld
        assert bool(torch.isnan(whole[:, cols:].float()).all()) and not bool(torch.isnan(v.float()).any())
        p.check()


@pytest.mark.parametrize("layout", layouts.LAYOUTS)
def test_output_buffers_are_the_sentinel_and_the_checker_sees_a_touched_one(layout):
    rows, cols = 6, 100
    t = torch.zeros(rows, cols)
    p = layouts.place(t, layout, layouts.SENTINEL, fill=layouts.SENTINEL)
    assert bool((p.buffer == layouts.SENTINEL).all())
    p.view.copy_(torch.randn(rows, cols))          # what a correct kernel does
    p.check(written=True)
    with pytest.raises(AssertionError, match="was modified"):
        p.check(written=False)
    if layout == "natural":
        return                                     # no padding to touch
    for r, c in ((0, cols), (rows - 1, p.ld - 1), (2, cols + 1)):
        q = layouts.place(t, layout, layouts.SENTINEL, fill=layouts.SENTINEL)
        q.buffer[q.front:].view(rows, q.ld)[r, c] = 1.0
        with pytest.raises(AssertionError, match="padding elements were written"):
            q.check(written=True)
    if layout == "offset":
        q = layouts.place(t, layout, layouts.SENTINEL, fill=layouts.SENTINEL)
        q.buffer[0] = 0.0
        with pytest.raises(AssertionError, match="padding"):
            q.check(written=True)


def test_the_checker_compares_bits():
    """NaN padding that stays NaN passes; a NaN with another payload, or -0.0 over 0.0, does not"""
    t = torch.zeros(3, 10)
    p = layouts.place(t, "pitched", float("nan"))
    p.check()
    p.buffer.view(torch.int32)[p.front + 10] ^= 1      # still a NaN, another bit pattern
    assert math.isnan(float(p.buffer[p.front + 10]))
    with pytest.raises(AssertionError, match="padding"):
        p.check()
    p = layouts.place(t, "odd", float("nan"))
    p.view[1, 2] = -0.0
    with pytest.raises(AssertionError, match="was modified"):
        p.check()
    p.reset(t)
    p.check()


def test_the_plan_of_a_call():
    got = layouts.plans(("x", "w"))
    assert [tag for tag, _ in got] == ["natural", "x-pitched", "w-pitched", "x-odd", "w-odd", "all-odd", "x-offset",
                                       "w-offset", "all-offset"]
    assert got[0][1] == {"x": "natural", "w": "natural"} and got[2][1] == {"x": "natural", "w": "pitched"}
    assert got[5][1] == {"x": "odd", "w": "odd"} and got[-1][1] == {"x": "offset", "w": "offset"}
