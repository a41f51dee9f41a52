"""The two users of the voxel-set chain (tsdf_amd/csrc/voxel_set.hpp) against each other: the frontier voxels of a state field, and
the same voxels carrying one class, must give the same list, labels and rows -- the explorer through the policy "any listed neighbour",
the objects handle through "same class".  Integers and bytes only."""
import numpy as np
import pytest

import tsdf_amd
from tests import explore_ref as R

pytestmark = pytest.mark.gpu

# chunks that straddle rows with a partial last chunk; a row one longer than a chunk; more than one wave of the flag kernel
GRIDS = [(13, 7, 5), (65, 4, 3), (67, 9, 11)]
CLASS = 7


@pytest.fixture(scope="module", params=GRIDS, ids=lambda s: "%dx%dx%d" % s)
def pair(request):
    """(size, the frontier ids of the reference, the votes of every voxel, the explorer after find_frontiers, the volume)."""
    size = request.param
    D, Wt = R.random_state_field(size, 5100 + size[0], 0.5)
    ids, _ = R.frontiers(D, Wt, size)
    n = size[0] * size[1] * size[2]
    votes = np.zeros(n, np.uint32)
    votes[ids] = 1 + ids % 3
    words = np.zeros(n, np.uint32)
    words[ids] = (votes[ids] << 16) | CLASS
    gv = tsdf_amd.TSDFVolume(size, (size[0] * 10.0, size[1] * 12.5, size[2] * 9.0))
    gv.set_distance_data(D)
    gv.set_weight_data(Wt)
    gv.enable_classes()
    gv.set_class_data(words)
    return size, ids, votes, gv.find_frontiers(), gv


@pytest.mark.parametrize("min_size", [1, 3])
@pytest.mark.parametrize("connectivity", [6, 26])
def test_frontier_clusters_are_the_objects_of_one_class(pair, connectivity, min_size):
    size, ids, votes, ex, gv = pair
    ex.cluster(connectivity, min_size)
    ob = gv.find_objects(min_votes=1, classes=None, connectivity=connectivity, min_size=min_size)
    voxels, labels, rows = ob.voxels, ob.labels, ob.objects
    assert len(voxels) >= 100 and len(rows) >= 1
    if connectivity == 6 and min_size == 3:
        assert len(rows) >= 10
    assert np.array_equal(voxels, ex.voxels) and np.array_equal(voxels, ids)
    assert np.array_equal(labels, ex.labels)
    e, o = ex.info, ob.info
    assert (o.n_labelled, o.n_objects, o.n_listed_objects) == (e.n_frontiers, e.n_clusters, e.n_listed_clusters)
    assert (o.n_labelled, o.n_listed_objects) == (len(voxels), len(rows))
    clusters = ex.clusters
    assert len(clusters) == len(rows)
    for field in ("label", "size", "lo", "hi", "sum"):
        assert np.array_equal(rows[field], clusters[field]), field
    assert np.all(rows["class_id"] == CLASS) and np.all(rows["reserved"] == 0)
    per_label = np.bincount(labels, weights=votes[voxels], minlength=len(voxels)).astype(np.uint64)
    assert np.array_equal(rows["votes"], per_label[rows["label"]])
