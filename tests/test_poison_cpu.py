"""tests/poison.py's own logic on CPU tensors (no GPU): what check() reports and accepts, how
guarded_frames lays the frames out, and that poisoned_empty leaves CPU tensors alone and
restores torch.empty."""
import numpy as np
import pytest
import torch

import poison

DTYPES = [torch.float64, torch.float32]


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sentinel_is_a_quiet_nan_with_a_payload(dtype):
    view, check = poison.guarded(10, dtype, "cpu", guard=8)
    assert view.dtype == dtype and view.numel() == 10 and check.buffer.numel() == 26
    assert torch.isnan(check.buffer).all()
    canonical = _bits(torch.full((1,), float("nan"), dtype=dtype))[0]
    assert (_bits(check.buffer) != canonical).all() and (_bits(check.buffer) != _bits(-torch.full(
        (1,), float("nan"), dtype=dtype))[0]).all()
    want = poison.SENTINEL_BITS["float64" if dtype == torch.float64 else "float32"]
    assert int(_bits(view)[0]) == want


@pytest.mark.parametrize("dtype", DTYPES)
def test_fully_written_buffer_is_accepted(dtype):
    view, check = poison.guarded(100, dtype, "cpu", guard=16)
    view.copy_(torch.arange(100, dtype=dtype))
    check()
    view.zero_()
    check("zeros")


@pytest.mark.parametrize("dtype", DTYPES)
def test_canonical_nan_is_a_value(dtype):
    view, check = poison.guarded(50, dtype, "cpu", guard=16)
    view.fill_(float("nan"))
    check()
    view.copy_(-view)  # the sign bit set: still not the sentinel
    check()
    view[7] = float("inf")
    check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("left", [[0], [99], [3, 40, 41]])
def test_untouched_elements_are_reported(dtype, left):
    view, check = poison.guarded(100, dtype, "cpu", guard=16)
    keep = view.clone()
    view.fill_(1.5)
    for i in left:
        _bits(view)[i] = _bits(keep)[i]
    msg = rf"vx: {len(left)} of 100 output elements never written.*first at {left[0]}$"
    with pytest.raises(AssertionError, match=msg):
        check("vx")


def test_nothing_written_reports_everything():
    view, check = poison.guarded(33, torch.float32, "cpu", guard=4)
    with pytest.raises(AssertionError, match=r"33 of 33 output elements never written.*first at 0$"):
        check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where,index,msg", [(15, -1, "below"), (0, -16, "below"), (116, 100, "above"),
                                             (131, 115, "above")])
def test_guard_overwrites_are_reported_on_either_side(dtype, where, index, msg):
    view, check = poison.guarded(100, dtype, "cpu", guard=16)
    view.fill_(2.0)
    check()
    check.buffer[where] = 2.0
    with pytest.raises(AssertionError, match=rf"1 guard elements {msg} the output overwritten, the first at {index} "):
        check()


def test_guard_overwritten_with_a_canonical_nan_is_reported():
    view, check = poison.guarded(10, torch.float64, "cpu", guard=4)
    view.fill_(0.0)
    check.buffer[3] = float("nan")
    check.buffer[2] = float("nan")
    with pytest.raises(AssertionError, match=r"2 guard elements below the output overwritten, the first at -2 "):
        check()


def test_guarded_refuses_other_types():
    with pytest.raises(TypeError):
        poison.guarded(4, torch.int32, "cpu")
    view, _ = poison.guarded(4, np.float32, "cpu", guard=2)  # numpy dtypes name the same types
    assert view.dtype == torch.float32


@pytest.mark.parametrize("dtype,loud", [(np.uint16, -1), (np.uint8, 255), (np.float32, 1e30), (np.float64, 1e30),
                                        (np.int16, -1)])
@pytest.mark.parametrize("misaligned", [False, True])
def test_guarded_frames_layout(dtype, loud, misaligned):
    rng = np.random.default_rng(3)
    stack = rng.integers(0, 200, size=(5, 3, 7, 5)).astype(dtype)  # 105 elements per frame: no 16-byte multiple
    frames = poison.guarded_frames(stack, device="cpu", guard_planes=2, misaligned=misaligned)
    assert len(frames) == 5
    es = np.dtype(dtype).itemsize
    base = frames[0]._base if frames[0]._base is not None else frames[0]
    whole = base.numpy()
    start = [(f.data_ptr() - base.data_ptr()) // es for f in frames]
    covered = np.zeros(whole.size, bool)
    for i, f in enumerate(frames):
        assert (f.data_ptr() % 16 == 0) == (not misaligned)
        assert np.array_equal(f.numpy().view(dtype), stack[i].reshape(-1))
        covered[start[i]:start[i] + 105] = True
        # two planes (70 elements) of the loud value on either side of every frame
        assert not covered[start[i] - 70:start[i]].any() and start[i] >= 70 and start[i] + 105 + 70 <= whole.size
    for i in range(4):
        assert start[i + 1] - (start[i] + 105) >= 70
    assert (whole[~covered] == np.asarray(loud).astype(whole.dtype)).all() and (~covered).sum() >= 6 * 70


def test_guarded_frames_takes_2d_windows():
    stack = np.arange(3 * 4 * 8, dtype=np.uint16).reshape(3, 4, 8)
    frames = poison.guarded_frames(stack, device="cpu")
    assert [f.numel() for f in frames] == [32, 32, 32]
    assert np.array_equal(frames[2].numpy().view(np.uint16), stack[2].reshape(-1))


def test_poisoned_empty_leaves_cpu_tensors_alone_and_restores(monkeypatch):
    real = torch.empty
    with poison.poisoned_empty(monkeypatch) as counter:
        assert torch.empty is not real
        t = torch.empty(16, dtype=torch.float64)
        u = torch.empty((2, 3), dtype=torch.int32, device="cpu")
        assert t.shape == (16,) and u.shape == (2, 3) and u.dtype == torch.int32
        assert counter.device_allocations == 0 and counter.bytes == 0
    assert torch.empty is real


def test_poisoned_empty_fills_device_tensors(monkeypatch):
    """The wrapper's fill and its counter without a GPU: the device branch is driven by tensors
    that report a device type other than "cpu" (zero-size tensors are not counted)."""
    real = torch.empty

    class FakeDevice:
        type = "cuda"

    class Reporting(torch.Tensor):
        @property
        def device(self):
            return FakeDevice()

    def fake_real(*a, **k):
        return real(*a, **k).as_subclass(Reporting)

    monkeypatch.setattr(torch, "empty", fake_real)
    with poison.poisoned_empty(monkeypatch) as counter:
        t = torch.empty(8, dtype=torch.float32)
        z = torch.empty(0, dtype=torch.float32)
        i = torch.empty((2, 2), dtype=torch.int64)
    assert counter.device_allocations == 2 and counter.bytes == 32 + 32 and z.numel() == 0
    assert torch.isnan(t.as_subclass(torch.Tensor)).all() and (i.as_subclass(torch.Tensor) == -1).all()
    assert torch.empty is fake_real
    monkeypatch.undo()
    assert torch.empty is real


def test_poisoned_empty_restores_after_a_failure(monkeypatch):
    real = torch.empty
    with pytest.raises(RuntimeError):
        with poison.poisoned_empty(monkeypatch):
            raise RuntimeError("inside")
    assert torch.empty is real
