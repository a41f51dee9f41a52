"""The frame differences through the C++ class surface (libtsdf_host.so: FrameDiff): build/test_frame_diff
(tests/cpp/test_frame_diff.cpp) compares, clusters and masks a 70 x 37 pair of images, checks the class against the C ABI and the
refusals as exceptions; what it prints and dumps must be the CPU reference's (tests/frame_diff_ref.py), byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import frame_diff_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_frame_diff")


@pytest.mark.gpu
def test_cpp_frame_differences_match_the_reference(tmp_path):
    if not os.path.exists(BIN):
        pytest.fail("build/test_frame_diff missing: run `make cpptest` (build() does)")
    w, h = 70, 37
    rng = np.random.default_rng(70)
    model = rng.integers(1500, 2500, (h, w)).astype(np.uint16)
    model[rng.random((h, w)) < 0.1] = 0
    frame = model.copy()
    frame[rng.random((h, w)) < 0.05] = 0
    frame[3:12, 60:70] = 700          # a blob that ends at the right border
    frame[20:30, 0:8] = 900           # one that starts at the left border
    frame[15:17, 30:33] = 650         # one below min_pixels
    frame[32:36, 40:50] = 3300        # farther
    p = dict(tolerance_mm=40, quadratic=1 << 14, connectivity=4, depth_step=60, min_pixels=10, dilate_px=3)
    frame.tofile(str(tmp_path / "frame.u16"))
    model.tofile(str(tmp_path / "model.u16"))
    r = subprocess.run([BIN, str(tmp_path / "frame.u16"), str(tmp_path / "model.u16"), str(w), str(h), str(p["tolerance_mm"]), str(p["quadratic"]),
                        str(p["connectivity"]), str(p["depth_step"]), str(p["min_pixels"]), str(p["dilate_px"]), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "frame differences ok" in r.stdout
    want = R.run(frame, model, **p)
    assert len(want["blobs"]) >= 2 and len(want["rows"]) > len(want["blobs"]) and want["counts"].min() > 0
    printed = [int(v) for v in re.findall(r"\d+", r.stdout.split("frame differences ok:")[1])]
    assert printed == want["counts"].tolist() + [len(want["rows"]), len(want["blobs"])], r.stdout
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    assert load("states.u8", np.uint8).tobytes() == want["states"].tobytes()
    assert np.array_equal(load("pixels.u32", np.uint32), want["pixels"])
    assert np.array_equal(load("labels.u32", np.uint32), want["labels"])
    assert load("blobs.bin", R.BLOB_DTYPE).tobytes() == want["blobs"].tobytes()
    assert load("mask.u8", np.uint8).tobytes() == want["mask"].tobytes()
    assert load("blob_index.u32", np.uint32).tobytes() == want["blob_index"].tobytes()
    assert load("frame_out.u16", np.uint16).tobytes() == want["frame_out"].tobytes()
