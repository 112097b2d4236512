"""A frame that k_cluster_lds gives up - at most 8192 object points in more cells than its table holds - is clustered again by
the global-memory kernels.  The rank and label kernels of the FIRST launch still run over that frame: k_cluster_lds leaves it as
single points without a rank so that they read nothing that was not written (before, k_label_count took parent[i] - whatever
an earlier, smaller frame or the allocation had left there - as an index).  Here: the labels of such a frame, first in a fresh
context after a smaller clustered frame, equal the oracle's."""
import numpy as np
import pytest

from perception_amd import capi

pytestmark = pytest.mark.gpu


def test_frame_given_up_by_the_lds_kernel(O):
    rng = np.random.RandomState(5)
    prm = capi.default_params()
    prm.cluster_tolerance = 0.01       # cells of 5.77 mm: the 6 mm lattice below puts every point into a cell of its own
    prm.cluster_min_size = 20
    # three slabs of a 6 mm lattice, 20 mm apart: 3 x 45 x 45 = 6075 points (<= 8192) in 6075 cells (> 3072), three clusters
    g = np.arange(45) * 0.006
    slab = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    big = np.concatenate([np.c_[slab, np.full(len(slab), 0.4 + 0.02 * s)] for s in range(3)]).astype(np.float32)
    big = big[rng.permutation(len(big))]
    small = big[:500].copy()           # a smaller frame first: the arrays behind its 500 points are untouched when `big` comes
    cx = capi.Context(max_points=8192, max_frames=1)
    try:
        for pts in (small, big, small):
            lab, sizes, k = cx.cluster(pts, prm)
            lo, so, ko = O.cluster(pts, prm)
            assert k == ko and np.array_equal(sizes, so) and np.array_equal(lab, lo), len(pts)
        assert k >= 0 and O.cluster(big, prm)[2] == 3
    finally:
        cx.close()
