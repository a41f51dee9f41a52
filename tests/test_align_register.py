"""Volume-to-volume registration (TSDFVolume.register: the source's mesh vertices aligned to the destination's field): two 48^3 volumes
of the same scene, the second's frames integrated under a known 20 mm / 2 degree offset.  register() from the identity must follow the
float64 reference chain (tests/align_ref.py) within the tolerance rule of tests/test_align.py -- 8 x the distance between that chain
summed in float64 and in fp32 in ascending point order -- and fuse() with the inverse then updates voxels."""
import numpy as np
import pytest

import tsdf_amd
from tests import align_ref as R
from tests import field_ref
from tests.helpers import Cam, assert_same_floats
from tsdf_amd import synth

pytestmark = pytest.mark.gpu
F = np.float32
N, PHYS, SEED, FRAMES, PERIOD = 48, 3000.0, 0x5EED2E61, (0, 5, 10), 40
ITERATIONS = 10


def test_register_recovers_a_known_offset_and_fuse_takes_it(oracle):
    fr = [synth.depth_frame(i, PERIOD, seed=SEED) for i in FRAMES]
    M = R.perturbation(20.0, 2.0, (PHYS / 2,) * 3, 0x2E61)          # the second session's world is M x the first's
    moved = []
    for d, cam in fr:
        pose = (M @ cam.pose().astype(np.float64).reshape(4, 4).T).astype(F)
        inv = np.linalg.inv(pose.astype(np.float64)).astype(F)
        moved.append((d, Cam(pose.T.reshape(-1), inv.T.reshape(-1), cam.k(), cam.kinv())))
    dst, src = tsdf_amd.TSDFVolume((N,) * 3, (PHYS,) * 3), tsdf_amd.TSDFVolume((N,) * 3, (PHYS,) * 3)
    od, osrc = oracle.Volume((N,) * 3, (PHYS,) * 3), oracle.Volume((N,) * 3, (PHYS,) * 3)
    for (d, cam), (_, cam2) in zip(fr, moved):
        dst.integrate(d, R.W, R.H, cam)
        src.integrate(d, R.W, R.H, cam2)
        od.integrate(d, R.W, R.H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
        osrc.integrate(d, R.W, R.H, cam2.inverse_pose(), cam2.k(), cam2.kinv(), nthreads=oracle.max_threads())
    assert_same_floats(dst.get_distance_data(), od.dist, "destination distances")
    assert_same_floats(dst.get_weight_data(), od.weight, "destination weights")
    assert_same_floats(src.get_distance_data(), osrc.dist, "source distances")
    mesh = src.extract_surface()
    assert len(mesh) >= 3000

    s = R.Scene()
    s.geom, s.dist, s.weight, s.gate = field_ref.geometry(od), od.dist, od.weight, float(od.truncation_distance())
    stages = [(mesh, ITERATIONS)]
    ref, norms, counts = R.chain(oracle, s, stages, np.eye(4), s.gate, order="f64")
    asc = R.chain(oracle, s, stages, np.eye(4), s.gate, order="ascending")[0]
    tol = 8 * R.pose_distance(ref, asc)
    truth = np.linalg.inv(M)
    # the reference alone: it sees enough of the surface and moves towards the known offset
    assert min(counts) * 4 >= len(mesh)
    assert R.pose_distance(ref, truth) < R.pose_distance(np.eye(4), truth) / 4

    T, res, inl = dst.register(src, iterations=ITERATIONS)
    print("register: |GPU - float64 reference| = %.3e, tolerance 8 x %.3e; to the known offset %.3f (start %.3f); inliers %g of %d"
          % (R.pose_distance(T, ref), tol / 8, R.pose_distance(T, truth), R.pose_distance(np.eye(4), truth), inl, len(mesh)))
    assert tol > 0 and R.pose_distance(T, ref) <= tol
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-12

    before = dst.get_weight_data()
    fused = dst.fuse(src, np.linalg.inv(T).T.reshape(-1))           # column-major dst_to_src
    assert fused > 0
    assert (dst.get_weight_data() != before).sum() == fused
    src.close()
    dst.close()
