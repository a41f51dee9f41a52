"""The condition tests/test_frame_diff_tracking.py puts on its scene, checked on the CPU (no GPU): the sequence's frames through the
oracle's bilateral filter, the model's depth image from the oracle's ray cast of an oracle volume that fuses the reference-masked frames,
and tests/frame_diff_ref.py with the test's parameters.  On the frames without a disc the reference masks at most 1 % of the pixels with
f > 0 (observed: 0 of 3072 on each of them), and on the frames with one every disc pixel over a known model is masked."""
import numpy as np

from tests import frame_diff_ref as R
from tests import test_frame_diff_tracking as T


def model_depth(ov, cam, oracle):
    """GPURaycaster::render_to_depth_image on the oracle's vertex map: the rounded camera z of every hit, 0 for a miss."""
    V = ov.raycast(T.W, T.H, cam.pose(), cam.kinv(), nthreads=oracle.max_threads())
    V = np.asarray(V[0] if isinstance(V, tuple) else V, np.float32).reshape(-1, 3)
    ip = cam.inverse_pose()
    z = np.rint(ip[2] * V[:, 0] + ip[6] * V[:, 1] + ip[10] * V[:, 2] + ip[14])
    ok = np.isfinite(z) & (z >= 1) & (z <= 65535)
    return np.where(ok, z, 0).astype(np.uint16).reshape(T.H, T.W)


def test_the_reference_masks_nothing_where_nothing_moves(oracle):
    ov = oracle.Volume(T.SIZE, T.PHYS)
    shares = []
    for i, (d, cam, disc) in enumerate(T.frames()):
        f = oracle.bilateral_u16(d, T.W, T.H, 30.0, 4.5)
        m = model_depth(ov, cam, oracle)
        want = R.run(f, m, **T.REF)
        seen = f > 0
        if i < T.FIRST_DISC:
            shares.append(int(want["mask"][seen].sum()) / int(seen.sum()))
            assert want["mask"][seen].sum() <= 0.01 * seen.sum(), (i, shares)
        else:
            on_model = disc.reshape(T.H, T.W) & (m > 0) & seen
            assert on_model.sum() > 50 and want["mask"][on_model].all(), i
        ov.integrate(want["frame_out"], T.W, T.H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=oracle.max_threads())
    print("masked share on the disc-free frames:", shares)
    assert len(shares) == T.FIRST_DISC
