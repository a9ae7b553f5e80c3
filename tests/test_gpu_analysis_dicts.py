"""The Python host of the device-side analysis gives the same dictionaries, bit for bit, and the
same errors, word for word, as the version that made tests/golden/summary/analysis_dicts.npz.

tests/test_gpu_summary_words.py holds the device words; this holds what analysis.py and
stream.py decode from them: tools/analysis_dicts.py runs every public entry and
a FlowStream with every add-on on small seeded fields and flattens the returned dicts to path ->
array; the paths, and every array's dtype, shape and bytes, must equal the committed file's.
The error table below — one entry, one bad input — is recorded in the same file as
"Type: message" strings; every case raises on the host, before any kernel is launched.
"""

import importlib.util
import os

import numpy as np
import pytest
from conftest import GOLDEN, REPO, bits_equal

pytestmark = pytest.mark.gpu

SHAPE3, SHAPE2 = (3, 5, 7), (5, 7)


def _tool():
    spec = importlib.util.spec_from_file_location("analysis_dicts", os.path.join(REPO, "tools", "analysis_dicts.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "summary", "analysis_dicts.npz")) as f:
        return _tool().unpack(f), {k: str(f[k]) for k in f.files if k.startswith("meta_")}


def test_analysis_dicts_are_bit_equal_to_the_golden_file(golden):
    want = {k: a for k, a in golden[0].items() if not k.startswith("error/")}
    got = _tool().generate()
    assert sorted(got) == sorted(want)
    wrong_type = [k for k in sorted(want) if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape]
    assert not wrong_type, f"dtype or shape differs from the file made by {golden[1]}: {wrong_type[:8]}"
    differing = [k for k in sorted(want) if not bits_equal(got[k], want[k])]
    assert not differing, f"{len(differing)} of {len(want)} arrays differ from {golden[1]}'s: {differing[:8]}"


def error_cases():
    """name -> call: every call hands one entry one bad input (everything else about it is good)."""
    import torch

    from opticalflow3d_dev_amd import analysis as an

    f3 = lambda dt=np.float64: np.ones(SHAPE3, dtype=dt)
    f2 = lambda dt=np.float64: np.ones(SHAPE2, dtype=dt)
    r3, r2, r1 = f3(np.float32), f2(np.float32), np.ones(7, dtype=np.float32)
    i3 = f3(np.int32)
    t3 = lambda: torch.ones(SHAPE3, dtype=torch.float32, device="cuda")
    ch = lambda rel=r3: (f3(), f3(), f3(), rel)
    four = {"flow_summary": an.flow_summary, "quiver_sample": an.quiver_sample, "export_fields": an.export_fields,
            "contractility": an.contractility}
    rel_only = {"reliability_mask": an.reliability_mask, "largest_component_mask": an.largest_component_mask,
                "principal_axes": an.principal_axes, "reliability_profile": an.reliability_profile}
    cases = {}
    for name, fn in four.items():
        cases[f"{name}/velocity_dtype"] = lambda fn=fn: fn(i3, i3, i3, r3)
        cases[f"{name}/rel_dtype"] = lambda fn=fn: fn(f3(), f3(), f3(), i3)
        cases[f"{name}/3d_without_vz"] = lambda fn=fn: fn(f3(), f3(), None, r3)
        cases[f"{name}/vz_with_2d"] = lambda fn=fn: fn(f2(), f2(), f2(), r2)
    for name, fn in rel_only.items():
        cases[f"{name}/rel_dtype"] = lambda fn=fn: fn(i3)
        cases[f"{name}/ndim"] = lambda fn=fn: fn(r1)
    cases["reliability_thresholds/rel_dtype"] = lambda: an.reliability_thresholds(t3().to(torch.int32), [50])
    cases["reliability_thresholds/numpy"] = lambda: an.reliability_thresholds(r3, [50])
    cases["reliability_thresholds/ndim"] = lambda: an.reliability_thresholds(t3().reshape(-1), [50])
    cases["reliability_mask/min_size"] = lambda: an.reliability_mask(r3, min_size=0)
    cases["joint_reliability_mask/mixed"] = lambda: an.joint_reliability_mask(r3, t3())
    cases["joint_reliability_mask/rel_dtype"] = lambda: an.joint_reliability_mask(r3, f3())
    cases["joint_reliability_mask/ndim"] = lambda: an.joint_reliability_mask(r1, r1)
    cases["joint_reliability_mask/shapes"] = lambda: an.joint_reliability_mask(r3, r2)
    cases["joint_reliability_mask/min_size"] = lambda: an.joint_reliability_mask(r3, r3, min_size=0)
    cases["joint_reliability_mask/two_thresholds"] = lambda: an.joint_reliability_mask(r3, r3, thresholds=[0.5])
    cases["channel_compare/mixed_rel"] = lambda: an.channel_compare(ch(), ch(t3()))
    cases["channel_compare/mixed_fields"] = lambda: an.channel_compare(ch(), (f3(), t3().double(), f3(), r3))
    cases["channel_compare/rel_dtype"] = lambda: an.channel_compare(ch(), ch(f3()))
    cases["channel_compare/velocity_dtype"] = lambda: an.channel_compare(ch(), (f3(), f3(np.float32), f3(), r3))
    cases["channel_compare/one_vz"] = lambda: an.channel_compare(ch(), (f3(), f3(), None, r3))
    cases["channel_compare/3d_without_vz"] = lambda: an.channel_compare((f3(), f3(), None, r3), (f3(), f3(), None, r3))
    cases["channel_compare/vz_with_2d"] = lambda: an.channel_compare((f2(), f2(), f2(), r2), (f2(), f2(), f2(), r2))
    cases["channel_compare/three_fields"] = lambda: an.channel_compare(ch()[:3], ch())
    cases["channel_compare/field_shape"] = lambda: an.channel_compare(ch(), (f3(), np.ones((3, 5, 8)), f3(), r3))
    return cases


def raised(call):
    """"Type: message" of the exception `call` raises."""
    with pytest.raises((TypeError, ValueError)) as e:
        call()
    return f"{type(e.value).__name__}: {e.value}"


def test_every_error_case_raises_the_recorded_error(golden):
    want = {k[len("error/"):]: str(a) for k, a in golden[0].items() if k.startswith("error/")}
    got = {name: raised(call) for name, call in error_cases().items()}
    assert sorted(got) == sorted(want)
    differing = {k: (got[k], want[k]) for k in sorted(want) if got[k] != want[k]}
    assert not differing, differing
