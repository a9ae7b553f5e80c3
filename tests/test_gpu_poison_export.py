"""The field export into hostile memory: of3d_field_export writes every byte of its result —
header, blocks and pads — and nothing outside it.  The result is allocated inside
poison.guarded (float64 words, all the sentinel NaN): after the call no word of it still holds
the sentinel and both guards are intact; and the same call under poison.poisoned_empty()
(every fresh device allocation 0xFF) gives the bytes it gives into a zeroed buffer."""
import numpy as np
import pytest

import export_ref as er
import poison
import quiver_ref as qr
from opticalflow3d_dev_amd import FieldSpec, export_fields
from opticalflow3d_dev_amd import analysis as an

pytestmark = pytest.mark.gpu

KW = dict(rel_percentile=60, xyscale=0.3, zscale=1.2, tscale=0.5)
SHAPE, ROIS = (5, 9, 13), [(0, 3, 1, 6, 0, 7), (2, 3, 4, 5, 6, 7)]  # 105 voxels and 1: odd counts, so pads


def _export_into(result, f, spec, v_f32=False):
    """One of3d_field_export call into `result` (a device tensor of the call's size) with the
    threshold at the 60th percentile; returns the _ExportCall."""
    import torch

    boxes = an.SummarySpec(rois=ROIS).resolve(SHAPE)[0]
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in f]
    call = an._ExportCall(boxes, SHAPE, t[3].dtype == torch.float64, v_f32, spec, 3,
                          (KW["xyscale"], KW["zscale"], KW["tscale"]))
    assert call.result_bytes == result.numel() * result.element_size()
    thresh = an.percentile_threshold_device(t[3], KW["rel_percentile"])
    call.enqueue((t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), v_f32), thresh.data_ptr(), None,
                 result.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return call


@pytest.mark.parametrize("v_dtype,spec", [
    (np.float64, FieldSpec(rois=(1, 2), dtype="float32")),                 # fp32 blocks of odd counts: 12-byte pads
    (np.float64, FieldSpec(rois=(1, 2))),                                  # fp64 blocks, the fp32 rel block
    (np.float32, FieldSpec(rois=(2, 0), mask="summary")),                  # ROI 1 listed and skipped
    (np.float64, FieldSpec(rois=(1,), fields=("vx", "rel"), mask=None)),   # fields left out
    (np.float64, FieldSpec(rois=(1, 2), fields=("vz",), mask="zero", physical=False)),
])
def test_every_byte_of_the_result_is_written_and_nothing_else(v_dtype, spec):
    f = qr.planted_fields(SHAPE, 41, v_dtype=v_dtype)
    boxes = an.SummarySpec(rois=ROIS).resolve(SHAPE)[0]
    size = an._ExportCall(boxes, SHAPE, False, v_dtype == np.float32, spec, 3, (1.0, 1.0, 1.0)).result_bytes
    view, check = poison.guarded(size // 8, np.float64, "cuda")
    assert view.data_ptr() % 16 == 0
    call = _export_into(view, f, spec, v_f32=v_dtype == np.float32)
    check("export result")
    words = view.cpu().numpy().view(np.int64)
    got = call.decode(words)
    exported, names, *_ = spec.resolve(3, 3)
    ref = er.export_ref(*f, **KW, rois=ROIS, export_rois=exported, fields=names, mask=spec.mask,
                        physical=spec.physical, dtype=spec.dtype)
    er.assert_blocks({"rois": ref["rois"], "threshold": ref["threshold"], "blocks": got}, ref,
                     bytes_exact=spec.mask is None and not spec.physical)
    # the pads are zeros: a block's words past its elements
    for blk in got:
        for name in names:
            a = blk[name]
            tail = (-a.nbytes) % 16
            start = (a.__array_interface__["data"][0] - words.__array_interface__["data"][0]) + a.nbytes
            assert start % 16 == a.nbytes % 16  # the block starts on a 16-byte boundary of the result
            assert not words.view(np.uint8)[start:start + tail].any(), (blk["roi"], name)
    assert any((-blk[n].nbytes) % 16 for blk in got for n in names)  # at least one pad was there to check


@pytest.mark.parametrize("spec", [FieldSpec(rois=(1, 2), dtype="float32"), FieldSpec(rois=(0, 2), mask="zero")])
def test_poisoned_allocations_give_the_same_bytes(spec, monkeypatch):
    import torch

    f = qr.planted_fields(SHAPE, 42)
    boxes = an.SummarySpec(rois=ROIS).resolve(SHAPE)[0]
    size = an._ExportCall(boxes, SHAPE, False, False, spec, 3, (1.0, 1.0, 1.0)).result_bytes
    zeroed = torch.zeros(size // 8, dtype=torch.int64, device="cuda")
    _export_into(zeroed, f, spec)
    kw = dict(KW, rois=ROIS, spec=spec)
    plain = export_fields(*f, **kw)
    with poison.poisoned_empty(monkeypatch) as counter:
        hostile = torch.empty(size // 8, dtype=torch.int64, device="cuda")
        assert int(hostile[0]) == -1
        _export_into(hostile, f, spec)
        poisoned = export_fields(*f, **kw)
    assert counter.device_allocations >= 2
    assert hostile.cpu().numpy().tobytes() == zeroed.cpu().numpy().tobytes()
    for a, b in zip(plain["blocks"], poisoned["blocks"]):
        for name in ("vx", "vy", "vz", "rel"):
            assert a[name].tobytes() == b[name].tobytes(), (a["roi"], name)
