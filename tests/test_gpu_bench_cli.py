"""bench.py as a program: a plain run (no --full) of the small 2D config times exactly the steps it
is given, prints the headline line without the --full measurements, and --dump-outputs writes the
last timed step's outputs — bit-identical to the oracle (oracle/cpu_ref.py calc_flow2D), as every
2D output is."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, bits_equal

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_outputs(tmp_path):
    import bench
    from oracle import cpu_ref

    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "c1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "Mvoxels/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    nt, _, ny, nx, s, t, w, _ = bench.CONFIGS["c1"]
    vox = line["config"]["frames_per_step"] * ny * nx
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(vox / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    # what --full adds is absent from a plain line
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["parity_sample"] is None
    assert "single_frame" not in line
    assert line["dump_outputs"]["files"] == ["vx.npy", "vy.npy", "rel.npy"] and line["dump_outputs"]["sample"] is None
    got = [np.load(out / f) for f in line["dump_outputs"]["files"]]
    nwin = line["config"]["nt_window"]
    assert all(a.dtype == np.float64 and a.shape == (nt - nwin + 1, ny, nx) for a in got)
    import torch

    series = bench.synthetic_slab(nt, 1, ny, nx, 0, 1, 20260206 + 1, torch.device("cuda", 0)).view(nt, ny, nx)
    host = series.cpu().numpy().view(np.uint16)
    for j in (0, nt - nwin):  # the first and the last output frame of the series
        want = cpu_ref.calc_flow2D(host[j:j + nwin], s, t, w, backend="scipy")
        for a, b in zip(got, want):
            assert bits_equal(a[j], np.ascontiguousarray(b, np.float64))
