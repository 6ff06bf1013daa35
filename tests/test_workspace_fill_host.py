"""tests/workspace_fill.py on the host: the fill patterns are what their descriptions claim."""
import numpy as np
import pytest
import torch

import workspace_fill as wf


@pytest.mark.parametrize("dtype,count", [(torch.float32, 37), (torch.uint8, 64), (torch.float16, 10), (torch.int64, 5)])
def test_zero_and_ones(dtype, count):
    t = torch.arange(count).to(dtype)
    assert wf.fill(t, wf.ZERO) is t
    assert t.view(torch.uint8).eq(0).all()
    wf.fill(t, wf.ONES)
    b = t.view(torch.uint8)
    assert b.eq(0xFF).all()
    n4 = b.numel() // 4 * 4
    assert torch.isnan(b[:n4].view(torch.float32)).all()                                  # NaN as fp32
    assert torch.isnan(b[:n4].view(torch.float16)).all()                                  # and as each fp16 half
    assert (b[:n4].numpy().view(np.uint32) == 0xFFFFFFFF).all()                           # the largest unsigned value


def test_big():
    t = torch.zeros(41, dtype=torch.float32)
    wf.fill(t, wf.BIG)
    assert (t.numpy().view(np.uint32) == 0x7F000000).all()
    assert torch.isfinite(t).all() and (t == 2.0 ** 127).all()
    assert torch.equal(torch.relu(t), t)                                                  # survives relu
    assert torch.isinf(t[:2].sum())                                                       # overflows in a sum
    assert t.numpy().view(np.uint32)[0] > np.array([1.0e30], np.float32).view(np.uint32)[0]  # wins an unsigned maximum


def test_big_in_a_byte_buffer_with_a_tail():
    b = torch.full((11,), 0x55, dtype=torch.uint8)
    wf.fill(b, wf.BIG)
    assert b.tolist() == [0, 0, 0, 0x7F, 0, 0, 0, 0x7F, 0, 0, 0]
    assert (b[:8].view(torch.float32) == 2.0 ** 127).all()


def test_fill_writes_a_slice_and_nothing_beside_it():
    t = torch.arange(12, dtype=torch.float32)
    wf.fill(t[4:8], wf.BIG)
    assert t[:4].tolist() == [0, 1, 2, 3] and t[8:].tolist() == [8, 9, 10, 11] and (t[4:8] == 2.0 ** 127).all()
    with pytest.raises(ValueError, match="contiguous"):
        wf.fill(t[::2], wf.ONES)


def test_stale_is_not_a_fill():
    with pytest.raises(ValueError, match="STALE"):
        wf.fill(torch.zeros(4), wf.STALE)
    with pytest.raises(ValueError, match="unknown"):
        wf.fill(torch.zeros(4), "ONE")
    assert wf.PATTERNS == (wf.ZERO, wf.ONES, wf.BIG, wf.STALE) and wf.FILLS == wf.PATTERNS[:3]


def test_fill_all_only_one_buffer():
    bufs = dict(a=torch.ones(4), b=torch.ones(4))
    wf.fill_all(bufs, wf.ONES, only="b")
    assert (bufs["a"] == 0).all() and torch.isnan(bufs["b"]).all()


def test_same_bits_and_first_difference():
    nan = torch.tensor([float("nan"), 1.0, -0.0])
    assert wf.same_bits(nan, nan.clone())
    assert not wf.same_bits(nan, torch.tensor([float("nan"), 1.0, 0.0]))                  # -0 is not +0
    assert not wf.same_bits(nan, nan[:2])
    assert wf.first_difference(dict(x=nan), dict(x=nan.clone())) is None
    msg = wf.first_difference(dict(x=nan, y=torch.tensor([1.0, 2.0])), dict(x=nan.clone(), y=torch.tensor([1.0, 3.0])))
    assert msg.startswith("y: 1 of 2 words differ, first at 1")


def test_other_family():
    assert wf.other_family({}) == dict(split_f16=0)
    assert wf.other_family(dict(split_f16=0)) == {} and wf.other_family(dict(split_bf16=0, complex_3m=0)) == {}
