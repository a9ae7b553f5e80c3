"""FlowStream.windows(load, first, count): the push-ahead protocol of a series in one place.
Every window it yields equals calc_flow3D / calc_flow2D of its frames bit for bit, whatever the
lookahead (K0 batching 5 and 2, frame pipelining, none; a 2-D stream), each frame is loaded
once, in order, and `lookahead` frames early except at the series' end."""
import numpy as np
import pytest

from conftest import bits_equal
from opticalflow3d_dev_amd import calc_flow2D, calc_flow3D
from opticalflow3d_dev_amd.stream import FlowStream

pytestmark = pytest.mark.gpu

SIG = (2, 2, 5)
NWIN = 13
NT = NWIN + 5  # 6 windows: with 4 frames of lookahead the last four go short of it


@pytest.fixture(autouse=True)
def _k12(monkeypatch):
    # batching rides on the fused gradient kernel's workspace layout; force it at test sizes
    monkeypatch.setenv("OF3D_K12", "1")


@pytest.fixture(scope="module")
def series():
    """ndim -> (frames, the host entry's result per window), computed once."""
    out = {}
    for ndim, shape, flow in ((3, (24, 40, 48), calc_flow3D), (2, (40, 48), calc_flow2D)):
        stack = np.random.default_rng(21 + ndim).integers(0, 3000, size=(NT,) + shape).astype(np.uint16)
        out[ndim] = (stack, [flow(stack[k:k + NWIN], *SIG) for k in range(NT - NWIN + 1)])
    return out


def _run(fs, stack, want, first, count):
    """Drive windows() with fs.depth windows in flight; checks every window and the loads."""
    loads, got, pend = [], [], []

    def load(i):
        loads.append(i)
        return stack[i]

    def take(k, p):
        for a, b in zip(p.result(), want[k]):
            assert a.dtype == b.dtype and bits_equal(a, b), k
        p.release()
        got.append(k)

    end = first + count + fs.nwin - 1
    for k, p in fs.windows(load, first, count):
        # resident when window k was submitted: its frames and the lookahead, up to the last frame
        assert loads == list(range(first, min(k + fs.nwin + fs.lookahead, end))), (k, loads)
        pend.append((k, p))
        if len(pend) == fs.depth:
            take(*pend.pop(0))
    for k, p in pend:
        take(k, p)
    assert got == list(range(first, first + count))
    assert loads == list(range(first, end))  # once per frame, in increasing order


@pytest.mark.parametrize("ndim,kw,batch,L", [(3, {}, 5, 4), (3, {"k0_batch": 2}, 2, 1), (3, {"lookahead": True}, 0, 1),
                                             (3, {"lookahead": False, "k0_batch": 0}, 0, 0), (2, {}, 0, 0)])
def test_windows_equal_host_entry(series, ndim, kw, batch, L):
    stack, want = series[ndim]
    with FlowStream(ndim, stack.shape[1:], np.uint16, *SIG, depth=2, **kw) as fs:
        assert (fs.nwin, fs.depth, fs.batch, fs.lookahead) == (NWIN, 2, batch, L)
        _run(fs, stack, want, 0, NT - NWIN + 1)
        assert ("k_tderiv_multi" in fs.plan.kernels()) == bool(batch), fs.plan.kernels()
        with pytest.raises(RuntimeError, match="ring already holds frames"):
            next(fs.windows(lambda i: stack[i], 0, 1))
    assert fs.plan.handle is None  # __exit__ closed the stream


@pytest.mark.parametrize("first,count", [(2, 3), (4, 1)])
def test_windows_sub_range(series, first, count):
    stack, want = series[3]
    with FlowStream(3, stack.shape[1:], np.uint16, *SIG, depth=2) as fs:
        _run(fs, stack, want, first, count)
