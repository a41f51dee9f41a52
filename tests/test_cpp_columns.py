"""The column maps through the C++ class surface (libtsdf_host.so: TSDFVolume::column_map, TSDFVolume::ColumnMap): build/test_columns
(tests/cpp/test_columns.cpp) projects the random 13 x 7 x 5 state field this test writes along every axis, an inner band reversed and
classified, and one map with an ESDF, checks the class against the C ABI and the refusals as exceptions; what it prints and dumps must
be the CPU reference's (tests/columns_ref.py), byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import columns_ref, explore_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_columns")
F32 = np.float32
VS, OFFSET = np.array([10.0, 12.5, 9.0], F32), (100.0, -50.0, 25.0)


@pytest.mark.gpu
def test_cpp_columns_match_the_reference(tmp_path):
    if not os.path.exists(BIN):
        pytest.fail("build/test_columns missing: run `make cpptest` (build() does)")
    size = (13, 7, 5)
    D, Wt = explore_ref.random_state_field(size, 1357, 0.8, fp32_oddities=True)
    D.tofile(str(tmp_path / "dist.f32"))
    Wt.tofile(str(tmp_path / "weight.f32"))
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "columns ok" in r.stdout

    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    printed = [int(v) for v in re.findall(r"\d+", r.stdout.split("columns ok:")[1])]
    want_printed = []
    for axis in (0, 1, 2):
        rows, totals = columns_ref.project(D, Wt, size, axis)
        assert load("rows%d.bin" % axis, columns_ref.COLUMN_DTYPE).tobytes() == rows.tobytes(), axis
        want_printed += [totals["n_unknown"], totals["n_free"], totals["n_occupied"], totals["n_ground"]]
    band, _ = columns_ref.project(D, Wt, size, 2, (1, 4), True)
    assert (band["top"] >= 0).sum() > 20
    assert load("band.bin", columns_ref.COLUMN_DTYPE).tobytes() == band.tobytes()
    cells, counts = columns_ref.classify(band, 1, 1)
    assert np.array_equal(load("cells.u8", np.uint8).reshape(cells.shape), cells)
    assert printed == want_printed + [counts["n_no_ground"], counts["n_traversable"], counts["n_blocked"]], r.stdout
    assert load("world.f32", F32).tobytes() == columns_ref.height_world(band, size, 2, (1, 4), True, VS, OFFSET).tobytes()
    E = load("esdf.f32", F32)
    assert len(E) == 13 * 7 * 5 and np.isfinite(E).any()
    with_esdf, _ = columns_ref.project(D, Wt, size, 1, None, False, esdf=E)
    assert load("with_esdf.bin", columns_ref.COLUMN_DTYPE).tobytes() == with_esdf.tobytes()
