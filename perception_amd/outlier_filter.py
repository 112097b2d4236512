"""Canonical rule C16 restated in numpy: statistical outlier removal on a cloud (pcl::StatisticalOutlierRemoval).

This module is the specification (include/cuboid_hip.h states the rule, DESIGN.md lists it): the device
(perception_amd/csrc/k_outlier.hip, cd_outlier_filter and the fused calls after cd_set_outlier_filter) and the host arithmetic
(perception_amd/csrc/outlier_math.hpp) equal it bit for bit - every dist_i, the three statistics and the kept set.  numpy only - no
GPU, no library.  Parity with a real PCL is unpinned, as for every other rule: PCL takes its neighbours from a k-d tree whose
order among equidistant points and whose summation order are its own.

The rule, for a cloud of n float32 xyz points, mean_k in 1..63, std_mul (double) and negative:
  1. points with a non-finite coordinate are dropped first: never anyone's neighbour, not counted, never in the output; m = the
     number of finite points;
  2. m <= mean_k: every finite point is kept (negative or not), nothing is computed, the statistics are reported as 0;
  3. for finite point i the squared distances to ALL finite points, itself included: d2 = (dx*dx + dy*dy) + dz*dz with
     dx = p_j.x - p_i.x ..., every operation one float32 operation; of these the mean_k + 1 smallest as a multiset, less exactly
     one entry, the smallest (the point itself; a coincident twin's 0 stays and counts);
  4. the float32 square root of each of the mean_k values left, added into a double in ascending order of value;
     dist_i = (float)(sum / mean_k);
  5. over the finite points in cloud order, sequentially in double: sum += d, sq += d * d with d = (double)dist_i; then
     mean = sum / m, var = (sq - sum * sum / m) / (m - 1), stddev = sqrt(var), threshold = mean + std_mul * stddev;
  6. a point is kept iff (double)dist_i <= threshold - with negative iff that is false; the output keeps the cloud's order.
Every operation is correctly rounded, so nothing here depends on how the work is divided.
"""
import numpy as np

MAX_MEAN_K = 63
_ROWS = 256      # queries per block of the distance matrix


def _check(mean_k, std_mul):
    if not (isinstance(mean_k, (int, np.integer)) and 1 <= int(mean_k) <= MAX_MEAN_K):
        raise ValueError("mean_k must be in 1 .. %d" % MAX_MEAN_K)
    if not np.isfinite(std_mul):
        raise ValueError("std_mul must be finite")


def finite_mask(xyz):
    """Step 1: the points every coordinate of which is finite."""
    return np.isfinite(np.asarray(xyz, np.float32)[:, :3]).all(axis=1)


def mean_distances(xyz, mean_k):
    """Steps 1 - 4.  Returns (finite, dist): dist is float32 of the cloud's length, 0 for a dropped point and for every point
    when step 2 applies."""
    p = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    fin = finite_mask(p)
    q = p[fin]
    m = len(q)
    dist = np.zeros(len(p), np.float32)
    if m <= mean_k:
        return fin, dist
    out = np.empty(m, np.float32)
    x, y, z = (np.ascontiguousarray(q[:, a]) for a in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        for r0 in range(0, m, _ROWS):
            r1 = min(r0 + _ROWS, m)
            dx = x[None, :] - x[r0:r1, None]
            dy = y[None, :] - y[r0:r1, None]
            dz = z[None, :] - z[r0:r1, None]
            d2 = (dx * dx + dy * dy) + dz * dz                      # float32 arrays: one rounding per operation
            assert d2.dtype == np.float32
            best = np.sort(np.partition(d2, mean_k, axis=1)[:, :mean_k + 1], axis=1)[:, 1:]    # ascending, the smallest dropped
            root = np.sqrt(best)                                    # float32, correctly rounded
            s = np.zeros(r1 - r0, np.float64)
            for k in range(mean_k):                                 # ascending order of value
                s = s + root[:, k].astype(np.float64)
            out[r0:r1] = (s / np.float64(mean_k)).astype(np.float32)
    dist[fin] = out
    return fin, dist


def statistics(dist, std_mul):
    """Step 5 over the dist_i of the finite points in cloud order: (mean, stddev, threshold) as Python floats."""
    d = np.asarray(dist, np.float32).astype(np.float64)
    m = len(d)
    with np.errstate(over="ignore", invalid="ignore"):
        total = np.add.accumulate(d)[-1]                            # sequential
        sq = np.add.accumulate(d * d)[-1]
        mean = total / np.float64(m)
        var = (sq - total * total / np.float64(m)) / np.float64(m - 1)
        stddev = np.sqrt(var)
        threshold = mean + np.float64(std_mul) * stddev
    return float(mean), float(stddev), float(threshold)


def outlier_filter(xyz, mean_k, std_mul, negative=False):
    """The rule.  Returns dict(indices int32 ascending, dist float32 (n), n_finite, computed, mean, stddev, threshold)."""
    _check(mean_k, std_mul)
    mean_k = int(mean_k)
    fin, dist = mean_distances(xyz, mean_k)
    m = int(fin.sum())
    if m <= mean_k:
        return dict(indices=np.flatnonzero(fin).astype(np.int32), dist=dist, n_finite=m, computed=False, mean=0.0, stddev=0.0, threshold=0.0)
    mean, stddev, threshold = statistics(dist[fin], std_mul)
    with np.errstate(invalid="ignore"):
        inlier = dist.astype(np.float64) <= np.float64(threshold)
    keep = fin & (~inlier if negative else inlier)
    return dict(indices=np.flatnonzero(keep).astype(np.int32), dist=dist, n_finite=m, computed=True, mean=mean, stddev=stddev, threshold=threshold)


def filter_cloud(records, mean_k, std_mul, negative=False):
    """The kept rows of an (n, k >= 3) float32 record array (x y z first), whole rows in their order, and the rule's dict."""
    r = np.asarray(records)
    o = outlier_filter(r[:, :3].view(np.float32) if r.dtype != np.float32 else r[:, :3], mean_k, std_mul, negative)
    return r[o["indices"]], o
