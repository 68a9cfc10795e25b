"""The guard-band detector of tests/layout_frames.py tested on the CPU: every region of a frame is poked once and must be reported with its position;
a NaN over a NaN sentinel of another payload, one unwritten element and one changed input element must each be seen."""
import pytest
import torch

from layout_frames import ALT_NAN, SENTINEL, Frame, FrameError, dense_guarded, frame_for_tile, out_ld

BF = torch.bfloat16
DTYPES = [torch.bfloat16, torch.float32, torch.uint8]


def _frame(dtype):
    # batch 3, 5 x 7 logical, 16-element rows, three rows between slices, 64 in front, 4 rows behind
    return Frame((3, 5, 7), dtype, ld=16, batch_stride=8 * 16, front=64, tail_rows=4)


def _other(f):
    return 0x11 if f.dtype == torch.uint8 else 0        # raw bits that differ from every sentinel


@pytest.mark.parametrize("dtype", DTYPES)
def test_geometry_and_sentinel(dtype):
    f = _frame(dtype)
    assert f.view.shape == (3, 5, 7) and f.view.stride() == (128, 16, 1) and f.view.storage_offset() == 64
    assert f.numel == 64 + 2 * 128 + 5 * 16 + 4 * 16
    assert int(f.inside.sum()) == 3 * 5 * 7
    want = SENTINEL[dtype]
    assert int(f.bits[0]) & ((1 << (8 * f.bits.element_size())) - 1) == want
    if dtype.is_floating_point:
        assert torch.isnan(f.buf).all()                 # the sentinel is a NaN: a kernel that read it would poison its result
    f.assert_untouched()
    with pytest.raises(FrameError):
        f.assert_all_written()
    f.view.fill_(1)
    f.assert_all_written()
    f.assert_untouched()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("region,offset,pos", [
    ("front guard, first element", 0, (-1, 0, -64)),
    ("front guard, directly in front of the view", 63, (-1, 0, -1)),
    ("row padding", 64 + 1 * 128 + 2 * 16 + 7, (1, 2, 7)),
    ("row padding, last column", 64 + 0 * 128 + 4 * 16 + 15, (0, 4, 15)),
    ("inter-batch gap", 64 + 0 * 128 + 5 * 16 + 0, (0, 5, 0)),
    ("inter-batch gap, last row", 64 + 1 * 128 + 7 * 16 + 3, (1, 7, 3)),
    ("last row's padding", 64 + 2 * 128 + 4 * 16 + 7, (2, 4, 7)),
    ("tail guard, first row", 64 + 2 * 128 + 5 * 16, (2, 5, 0)),
    ("tail guard, last element", 64 + 2 * 128 + 9 * 16 - 1, (2, 8, 15)),
])
def test_a_poke_into_every_region_is_found_and_named(dtype, region, offset, pos):
    f = _frame(dtype)
    f.view.fill_(1)
    assert offset < f.numel and not bool(f.inside[offset])
    f.bits[offset] = _other(f)
    with pytest.raises(FrameError) as e:
        f.assert_untouched()
    assert e.value.count == 1 and e.value.positions == [pos], (region, e.value.positions)
    assert str(pos) in str(e.value)
    assert f.touched_positions() == [pos]
    f.assert_all_written()                               # the view itself is complete


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float16])
def test_a_nan_with_another_payload_over_the_nan_sentinel_is_detected(dtype):
    f = Frame((4, 6), dtype, ld=8, front=8, tail_rows=2)
    f.view.fill_(0.5)
    f.assert_untouched()
    f.bits[8 + 1 * 8 + 6] = ALT_NAN[dtype]               # still a NaN as a float: only the integer comparison sees it
    assert torch.isnan(f.buf[8 + 1 * 8 + 6])
    with pytest.raises(FrameError) as e:
        f.assert_untouched()
    assert e.value.positions == [(0, 1, 6)]


def test_the_view_is_not_part_of_the_guard():
    f = _frame(BF)
    f.view.copy_(torch.randn(3, 5, 7).to(BF))
    f.view[1, 2, 3] = float("nan")                       # a NaN result inside the view is the comparison's business, not the guard's
    f.assert_untouched()
    f.assert_all_written()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_unwritten_element_is_detected(dtype):
    f = _frame(dtype)
    f.view.fill_(1)
    f._view_bits[2, 4, 6] = f.bits[0]                    # put the sentinel back into the very last element
    with pytest.raises(FrameError) as e:
        f.assert_all_written()
    assert e.value.count == 1 and e.value.positions == [(2, 4, 6)]


@pytest.mark.parametrize("where", ["view", "poison"])
def test_a_changed_input_element_is_detected(where):
    data = torch.randn(2, 5, 7).to(BF)
    f = Frame.of(data, ld=16, batch_stride=8 * 16, front=64, tail_rows=2)
    assert torch.equal(f.view, data) and torch.isnan(f.padded[:, :, 7:]).all() and torch.isnan(f.rows_behind(2)).all()
    with pytest.raises(AssertionError):
        f.assert_unchanged()                             # not sealed yet
    f.seal()
    f.assert_unchanged()
    if where == "view":
        f.view[1, 3, 2] += 1
        want = (1, 3, 2)
    else:
        f.bits[64 + 5 * 16 + 1] = 0
        want = (0, 5, 1)
    with pytest.raises(FrameError) as e:
        f.assert_unchanged()
    assert e.value.positions == [want]


def test_input_poison_may_be_a_finite_value():
    data = torch.ones(4, 33, dtype=BF)
    f = Frame.of(data, ld=48, poison=0.0)
    assert (f.padded[0, :, 33:] == 0).all() and (f.buf[:64] == 0).all()
    f.padded[0, :, 33:] = torch.tensor([3e38, -3e38, 3e38] * 5, dtype=BF)
    f.seal().assert_unchanged()
    assert torch.isfinite(f.buf).all()


def test_sizing_rule_holds_a_whole_unmasked_tile():
    """a 77 x 200 output of a 256 x 320 tile: every element of the tile stored from the view's origin lies inside the allocation"""
    assert out_ld(200, 128) == 264 and out_ld(200, 160) == 328 and out_ld(200, 320) == 328 and out_ld(100, 0 + 1) == 112
    f = frame_for_tile((3, 77, 200), BF, tile_rows=256, tile_cols=320)
    assert f.ld == 328 and f.ld % 8 == 0 and f.batch_stride == 80 * 328 and f.front == 64
    last = f.front + 2 * f.batch_stride + (256 - 1) * f.ld + 319                   # last element of the last slice's unmasked tile
    assert last < f.numel
    assert (f.front * f.buf.element_size()) % 16 == 0 and (f.batch_stride * f.buf.element_size()) % 16 == 0      # the view keeps the allocation's 16-byte alignment
    g = dense_guarded((2, 5, 6, 64), BF, rows=256)
    assert g.view.is_contiguous() and g.view.shape == (2, 5, 6, 64) and g.view.storage_offset() == 64
    g.view.fill_(1)
    g.assert_untouched()
    g.assert_all_written()


def test_two_frames_in_one_allocation():
    """an ABI that addresses one array relative to another (bytes + scales of an e4m3 copy) gets two frames inside one buffer: each watches its own part only"""
    a = Frame((6, 10), torch.uint8, ld=16, front=16, tail_rows=2)
    b = Frame((3, 6), torch.uint8, ld=16, front=16, tail_rows=1)
    both = torch.empty(a.numel + b.numel, dtype=torch.uint8)
    a = Frame((6, 10), torch.uint8, ld=16, front=16, tail_rows=2, storage=both[:a.numel])
    b = Frame((3, 6), torch.uint8, ld=16, front=16, tail_rows=1, storage=both[a.numel:])
    assert b.view.data_ptr() - a.view.data_ptr() == a.numel and a.view.data_ptr() - both.data_ptr() == 16
    a.view.fill_(1)
    b.view.fill_(2)
    for f in (a, b):
        f.assert_untouched()
        f.assert_all_written()
    assert int((both == 1).sum()) == 60 and int((both == 2).sum()) == 18
    both[a.numel + 16 + 6] = 9                            # row padding of b
    a.assert_untouched()
    with pytest.raises(FrameError) as e:
        b.assert_untouched()
    assert e.value.positions == [(0, 0, 6)]
