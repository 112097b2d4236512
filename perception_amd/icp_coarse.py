"""Canonical rule C18: coarse-to-fine ICP, a resolution pyramid of two levels, in plain Python and numpy.  No
GPU and no library.  The ICP of either level is not restated here: it is the oracle's (oracle.oracle_py.icp) or, under rule
C17, perception_amd.icp_plane.icp - the caller hands it in.  This module holds what the rule adds: the subsample, the
eligibility test, the hand-over and fall-back decision, and the stats record.  perception_amd/csrc/icp_coarse_plan.hpp
restates the host part, k_icp_coarse.hip the hand-over on the GPU, and both are compared with this module.

The setting is (stride s, min_points m); s = 0 is off.  A (cluster, template) pair whose cluster has n >= m points is eligible:

    1. coarse set   the points p[j s], j = 0 .. ceil(n / s) - 1, of the cluster in extraction order
    2. coarse ICP   the ICP of the coarse set as a cluster of its own - same template, parameters, bound, plane weight and guess
                    mode (a per-cluster guess is computed on the coarse set) -> T_c
    3. fine ICP     the ICP of the whole cluster started from T_c, as a single guess T_c would start it; the iteration limit
                    applies to each level on its own; every record of the cluster is the fine level's
    4. fall-back    a coarse ICP that stopped (fewer than three correspondences, a singular plane-weighted step) or whose T_c has
                    a non-finite entry is dropped: the fine level starts from the call's own guess, as with the mode off
"""
import collections

import numpy as np

STRIDE_MIN, STRIDE_MAX = 2, 64
NOT_ELIGIBLE, USED, FELL_BACK = 0, 1, 2
CD_OK, CD_ERR_FEW_CORRESPONDENCES = 0, -5
MAX_DOUBLE = float(np.finfo(np.float64).max)

# cd_icp_coarse_stats
CoarseStats = collections.namedtuple("CoarseStats", "n_coarse coarse_iterations coarse_converged coarse_status coarse_fitness used")
NO_STATS = CoarseStats(0, 0, 0, CD_OK, 0.0, NOT_ELIGIBLE)


def setting_ok(stride, min_points):
    """What cd_set_icp_coarse takes: stride 0 (off), or 2 .. 64 with min_points >= 3 * stride (no coarse set under three points)."""
    if stride == 0:
        return True
    return STRIDE_MIN <= stride <= STRIDE_MAX and min_points >= 3 * stride


def eligible(n, stride, min_points):
    return stride >= STRIDE_MIN and n >= min_points


def indices(n, stride):
    """Step 1's index rule alone: j s for j = 0 .. ceil(n / s) - 1 (int32, ascending)."""
    return np.array([j * stride for j in range(-(-n // stride))], np.int32)


def subsample(n, stride, min_points):
    """Step 1: the indices of the coarse set of a set of n points (int32, ascending); empty when the set is not eligible or the
    setting is not one setting_ok takes."""
    if n < 0 or not setting_ok(stride, min_points) or not eligible(n, stride, min_points):
        return np.zeros(0, np.int32)
    return indices(n, stride)


def fall_back(stopped, T):
    """Step 4 on the end of a coarse ICP: stopped (truthy: too few correspondences, a singular step) or a non-finite entry of T_c."""
    return bool(stopped) or not bool(np.all(np.isfinite(np.asarray(T, np.float32))))


def two_level(points, stride, min_points, run, guess_of):
    """One (cluster, template) pair under the rule.
    points: (n, 3) float32 in extraction order.  run(points, guess) -> a dict with at least T (4, 4) float32, iterations,
    converged, fitness and stopped: the ICP of the mode on that set from that guess (None: none).  guess_of(points) -> the call's
    own guess for a set (a constant for every mode but the per-cluster one).
    Returns (the pair's record - the fine level's dict - and its CoarseStats)."""
    pts = np.ascontiguousarray(points, np.float32)
    idx = subsample(len(pts), stride, min_points)
    if len(idx) == 0:
        return run(pts, guess_of(pts)), NO_STATS
    coarse = np.ascontiguousarray(pts[idx])
    c = run(coarse, guess_of(coarse))
    back = fall_back(c["stopped"], c["T"])
    stats = CoarseStats(len(coarse), int(c["iterations"]), int(c["converged"]), CD_ERR_FEW_CORRESPONDENCES if c["stopped"] else CD_OK,
                        float(c["fitness"]), FELL_BACK if back else USED)
    fine = run(pts, guess_of(pts) if back else np.asarray(c["T"], np.float32).reshape(4, 4))
    return fine, stats
