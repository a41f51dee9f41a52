"""Sparse snapshots through the C++ class surface (libtsdf_host.so: TSDFVolume::snapshot / restore / save_sparse / load_sparse):
build/test_snapshot (tests/cpp/test_snapshot.cpp) fuses three frames on a 64^3 volume, snapshots, saves, clears, loads and restores,
and checks the refusals as the class surface's errors; its dumps must be the CPU reference's (tests/snapshot_ref.py) on the oracle's
own fusion, bit for bit, and its file's bytes the Python writer's."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_amd
from tests import snapshot_ref as R
from tests.helpers import H, W
from tsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_snapshot")
F32 = np.float32


@pytest.mark.gpu
def test_cpp_snapshot_matches_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_snapshot missing: run `make cpptest` (build() does)")
    n, frames = 64, 3
    fr = [synth.depth_frame(i * 9, 40, seed=0x5EEDE5D0) for i in range(frames)]
    np.concatenate([d.reshape(-1) for d, _ in fr]).astype(np.uint16).tofile(str(tmp_path / "frames.u16"))
    np.concatenate([cam.pose().astype(F32).reshape(-1) for _, cam in fr]).tofile(str(tmp_path / "poses.f32"))
    r = subprocess.run([BIN, str(tmp_path / "frames.u16"), str(tmp_path / "poses.f32"), str(frames), str(n), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "snapshot ok" in r.stdout
    # the refused files say why
    for word in ("grid", "open", "bytes", "magic", "deformation"):
        assert word in r.stdout, (word, r.stdout)

    offset = (10.0, -20.0, 30.0)
    ov = oracle.Volume((n,) * 3, (3000.0,) * 3)
    gv = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    for d, cam in fr:
        ov.integrate(d, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
        gv.integrate(d, W, H, cam)
    gv.offset(*offset)                   # (after the fusion, as the program does: it goes into the file's header)
    D, Wt = ov.dist, ov.weight
    ids, d, w, _ = R.take(D, Wt, (n,) * 3, F32(gv.truncation_distance()), 8)
    assert len(ids) == 288 and "%d bricks" % len(ids) in r.stdout
    assert np.fromfile(str(tmp_path / "ids.u32"), np.uint32).tobytes() == ids.tobytes()
    assert np.fromfile(str(tmp_path / "distances.f32"), F32).tobytes() == d.tobytes()
    assert np.fromfile(str(tmp_path / "weights.u8"), np.uint8).tobytes() == w.tobytes()
    # the file's bytes are the Python writer's
    gv.save_sparse(str(tmp_path / "python.tsdfs"))
    assert open(str(tmp_path / "python.tsdfs"), "rb").read() == open(str(tmp_path / "volume.tsdfs"), "rb").read()
    back = tsdf_amd.TSDFVolume.load_sparse(str(tmp_path / "volume.tsdfs"))
    assert back.get_distance_data().tobytes() == D.tobytes() and back.get_weight_data().tobytes() == Wt.tobytes()
    assert tuple(back.offset()) == offset
    for o in (gv, back):
        o.close()
