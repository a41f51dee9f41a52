"""Ray integration through the C++ class surface (libtsdf_host.so: TSDFVolume::integrate_rays, release_ray_scratch):
build/test_integrate_rays (tests/cpp/test_integrate_rays.cpp) fuses the rays it is given twice -- from one origin, then band only with a
range gate from one origin per ray -- and checks that the refusals throw; its dumps must be the CPU reference's
(tests/rays_integrate_ref.py) bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import rays_integrate_cases as RC
from tests import rays_integrate_ref as ref
from tests.helpers import assert_same_floats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "test_integrate_rays")
F32 = np.float32
MIN_RANGE, MAX_RANGE = 900.0, 2400.0


@pytest.mark.gpu
def test_cpp_integrate_rays_matches_the_reference(tmp_path, oracle):
    if not os.path.exists(BIN):
        pytest.fail("build/test_integrate_rays missing: run `make cpptest` (build() does)")
    o, p = RC.permutation_sets()[0]
    o.astype(F32).tofile(str(tmp_path / "origins.f32"))
    p.astype(F32).tofile(str(tmp_path / "points.f32"))
    r = subprocess.run([BIN, str(tmp_path / "origins.f32"), str(tmp_path / "points.f32"), str(len(p)), repr(MIN_RANGE), repr(MAX_RANGE),
                        str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    counts = [int(g) for g in re.search(r"integrate_rays surface ok: (\d+) then (\d+) voxels updated", r.stdout).groups()]

    ov, geom = RC.make_geometry(oracle, RC.GRID)
    d1, w1, upd1, _ = ref.integrate(geom, ov.dist, ov.weight, o[:1], p)
    d2, w2, upd2, _ = ref.integrate(geom, d1, w1, o, p, MIN_RANGE, MAX_RANGE, ref.BAND_ONLY)
    assert upd1.sum() >= 5000 and 500 <= upd2.sum() < upd1.sum() and w2.max() == 2
    assert counts == [int(upd1.sum()), int(upd2.sum())]
    load = lambda name: np.fromfile(str(tmp_path / name), F32)
    assert_same_floats(load("distances.f32"), d2, "C++ ray-integrated distances")
    assert_same_floats(load("weights.f32"), w2, "C++ ray-integrated weights")
