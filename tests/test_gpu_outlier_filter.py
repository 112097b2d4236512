"""cd_outlier_filter on the GPU (k_outlier.hip): the kept indices, the bits of every dist_i and the bits of the three statistics
equal canonical rule C16 restated in numpy (perception_amd/outlier_filter.py) exactly - no tolerance - at both ends of mean_k,
around every edge of the kernel's 64-candidate step and of its LDS tile, with several workgroups per cloud, on ties, coincident
points and non-finite points; the argument checks."""
import struct

import numpy as np
import pytest

from perception_amd import capi, outlier_filter as OF
from test_outlier_filter_cpu import coincident_cloud, lattice_cloud, nan_cloud, random_cloud

pytestmark = pytest.mark.gpu
TILE = capi.CD_OUTLIER_LDS_TILE      # candidates the kernel stages in LDS at a time (include/cuboid_hip.h)
CAP = 4096


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(max_points=CAP, max_frames=1)
    yield c
    c.close()


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _check(ctx, p, mean_k, std_mul=1.0, negative=False):
    want = OF.outlier_filter(p, mean_k, std_mul, negative)
    idx, dist, stats = ctx.outlier_filter(p, mean_k, std_mul, negative)
    bad = np.flatnonzero(dist.view(np.uint32) != want["dist"].view(np.uint32))
    print("n=%d mean_k=%d std_mul=%g negative=%d: m=%d kept=%d (module %d), dist words differing: %d" % (
        len(p), mean_k, std_mul, negative, want["n_finite"], len(idx), len(want["indices"]), len(bad)))
    assert len(bad) == 0, (bad[:8], dist[bad[:8]], want["dist"][bad[:8]])
    assert [_bits(v) for v in stats] == [_bits(want[k]) for k in ("mean", "stddev", "threshold")]
    assert idx.dtype == np.int32 and np.array_equal(idx, want["indices"])
    return want


def test_one_point_mean_k_points_and_the_first_size_that_computes(ctx):
    assert not _check(ctx, random_cloud(1, 1), 1)["computed"]
    assert not _check(ctx, random_cloud(16, 2), 16)["computed"]
    assert _check(ctx, random_cloud(17, 3), 16)["computed"]
    for negative in (False, True):        # step 2 holds for negative too
        idx, dist, stats = ctx.outlier_filter(random_cloud(16, 2), 16, 1.0, negative)
        assert list(idx) == list(range(16)) and not dist.any() and stats == (0.0, 0.0, 0.0)
    idx, dist, stats = ctx.outlier_filter(np.zeros((0, 3), np.float32), 4)
    assert len(idx) == 0 and len(dist) == 0


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
@pytest.mark.parametrize("mean_k", [1, 63])
def test_edges_of_a_64_candidate_step_at_both_ends_of_mean_k(ctx, n, mean_k):
    want = _check(ctx, random_cloud(n, 1000 + n), mean_k)
    assert want["computed"] == (n > mean_k)


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_around_the_lds_tile(ctx, n):
    assert TILE == 1024
    want = _check(ctx, random_cloud(n, 2000 + n), 16)
    assert 0 < len(want["indices"]) < n


def test_2500_points_several_workgroups(ctx):
    want = _check(ctx, random_cloud(2500, 77, spread=0.05), 16)
    assert 0 < len(want["indices"]) < 2500
    _check(ctx, random_cloud(2500, 78, spread=0.05), 50)


def test_lattice_ties_coincident_pairs_and_non_finite_points(ctx):
    for mean_k in (6, 16):
        _check(ctx, lattice_cloud(), mean_k)
    _check(ctx, coincident_cloud(), 4)
    want = _check(ctx, coincident_cloud(), 1)
    assert (want["dist"][1::3] == 0).all()           # mean_k = 1: a twin's 0 is the whole mean
    p = nan_cloud()
    want = _check(ctx, p, 10)
    idx, dist, _ = ctx.outlier_filter(p, 10)
    assert want["n_finite"] == len(p) - 3 and not np.isin([7, 20, 33], idx).any() and not dist[[7, 20, 33]].any()
    _check(ctx, p, 10, negative=True)
    allnan = np.full((40, 3), np.nan, np.float32)
    idx, dist, stats = ctx.outlier_filter(allnan, 3)
    assert len(idx) == 0 and not dist.any() and stats == (0.0, 0.0, 0.0)


def test_std_mul_zero_negative_and_a_descending_cloud(ctx):
    p = random_cloud(500, 5)
    _check(ctx, p, 16, std_mul=0.0)
    _check(ctx, p, 16, std_mul=-0.5)
    a = _check(ctx, p, 16, negative=True)
    b = _check(ctx, p, 16, negative=False)
    assert sorted(list(a["indices"]) + list(b["indices"])) == list(range(500))
    # candidates in descending distance from the first queries: every step lowers the 64th best, so every step merges
    q = np.zeros((700, 3), np.float32)
    q[:, 0] = np.arange(700, 0, -1) * 0.001
    _check(ctx, q, 63)
    _check(ctx, q[::-1].copy(), 30)
    big = random_cloud(300, 6) * np.float32(1e19)    # squared distances overflow to +inf: still candidates, still ordered
    _check(ctx, big, 5)


def test_argument_checks_and_capacity(ctx):
    p = random_cloud(200, 8)
    want = OF.outlier_filter(p, 16, 1.0)
    kept = len(want["indices"])
    assert 0 < kept < 200
    with pytest.raises(capi.CuboidError) as e:
        ctx.outlier_filter(p, 16, 1.0, capacity=kept - 1)
    assert e.value.status == capi.CD_ERR_CAPACITY
    idx, _, _ = ctx.outlier_filter(p, 16, 1.0, capacity=kept)
    assert np.array_equal(idx, want["indices"])
    for mean_k, std_mul in ((64, 1.0), (-1, 1.0), (0, 1.0), (16, float("nan")), (16, float("inf"))):
        with pytest.raises(capi.CuboidError) as e:
            ctx.outlier_filter(p, mean_k, std_mul)
        assert e.value.status == capi.CD_ERR_INVALID_ARG
    with pytest.raises(capi.CuboidError) as e:
        ctx.outlier_filter(random_cloud(CAP + 1, 9), 16)
    assert e.value.status == capi.CD_ERR_CAPACITY
    # the setting of the fused calls: off by default, checked, kept on a refused change, and not touched by the call above
    assert ctx.outlier_filter_setting()[0] == 0
    ctx.set_outlier_filter(16, 1.5, True)
    assert ctx.outlier_filter_setting() == (16, 1.5, True)
    for mean_k, std_mul in ((64, 1.0), (-1, 1.0), (5, float("nan"))):
        with pytest.raises(capi.CuboidError) as e:
            ctx.set_outlier_filter(mean_k, std_mul)
        assert e.value.status == capi.CD_ERR_INVALID_ARG
    assert ctx.outlier_filter_setting() == (16, 1.5, True)
    ctx.set_outlier_filter(0)
    assert ctx.outlier_filter_setting()[0] == 0
    with pytest.raises(capi.CuboidError):
        ctx.outlier_stats(0)                          # no fused call
