"""The rolling volume through the C++ class surface (libtsdf_host.so: TSDFVolume::Snapshot::select, TSDFVolume::restore with a shift,
TSDFVolume::shift): build/test_rolling (tests/cpp/test_rolling.cpp) fills a 40 x 32 x 24 volume from a random field, selects a box,
shifts there and back and restores with a shift, and checks the refusals as exceptions; its dumps must be the CPU reference's
(tests/rolling_ref.py), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import rolling_ref as RR
from tests import snapshot_cases as K
from tests import snapshot_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_rolling")
F32, U32 = np.float32, np.uint32


@pytest.mark.gpu
def test_cpp_rolling_matches_the_reference(tmp_path):
    if not os.path.exists(BIN):
        pytest.fail("build/test_rolling missing: run `make cpptest` (build() does)")
    size = (40, 32, 24)
    D, Wt, _ = K.random_case(size, 8, False)
    D.tofile(str(tmp_path / "distances.f32"))
    Wt.tofile(str(tmp_path / "weights.f32"))
    r = subprocess.run([BIN, str(tmp_path / "distances.f32"), str(tmp_path / "weights.f32")] + [str(s) for s in size] + [str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "rolling ok" in r.stdout
    for word in ("dst is src", "never been filled", "flags", "leaving is work", "multiple of 8"):
        assert word in r.stdout, (word, r.stdout)

    def dumped(name, dtype):
        return np.fromfile(str(tmp_path / name), dtype)

    def assert_list(stem, want):
        assert dumped(stem + "_ids.u32", U32).tobytes() == want[0].tobytes(), stem
        assert dumped(stem + "_distances.f32", F32).tobytes() == want[1].tobytes(), stem
        assert dumped(stem + "_weights.u8", np.uint8).tobytes() == want[2].tobytes(), stem

    snap = R.take(D, Wt, size, K.FILL, 8)
    inside, outside = RR.select(*snap, size, (1, 0, 1), (3, 2, 2)), RR.select(*snap, size, (1, 0, 1), (3, 2, 2), outside=True)
    assert 0 < len(inside[0]) < len(snap[0])
    assert_list("inside", inside)
    assert_list("outside", outside)
    after, leaving = RR.shift(D, Wt, None, size, (1, 0, -1), K.FILL, 8)
    assert len(leaving[0]) > 0
    assert dumped("shifted_distances.f32", F32).tobytes() == after[0].tobytes()
    assert dumped("shifted_weights.f32", F32).tobytes() == after[1].tobytes()
    assert_list("leaving", leaving)
    assert dumped("shifted_offset.f32", F32).tobytes() == RR.shifted_offset(K.OFFSET, (1, 0, -1), K.VS).tobytes()
    restored = RR.restore_shifted(*snap, size, size, (-1, 1, 0), K.FILL)
    assert dumped("restored_distances.f32", F32).tobytes() == restored[0].tobytes()
    assert dumped("restored_weights.f32", F32).tobytes() == restored[1].tobytes()
    assert "%d bricks, %d in the box, %d left" % (len(snap[0]), len(inside[0]), len(leaving[0])) in r.stdout
