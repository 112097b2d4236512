"""The expected result of a fused call (or of a cd_icp) with coarse-to-fine ICP on (rule C18), composed on the CPU: tests/fused_reference.py
with its own pair function run twice per eligible pair - coarse pair -> hand-over -> fine pair - by perception_amd/icp_coarse.py.
CPU only.  Everything fused_reference.expected returns stays; every pair that was run (and so every Cluster) gains coarse_stats, an
icp_coarse.CoarseStats; clusters that were never run (fewer than three points) have none (coarse_stats_of gives NO_STATS)."""
import numpy as np

import fused_reference as FR
from perception_amd import cluster_frame as cf, icp_coarse as IC

SINGLE_PAIR = FR._pair      # fused_reference's pair function: one ICP by the specification of the mode


def pair(tpl, axes, src, prm, opt, guess, coarse):
    """One (cluster, template) pair under rule C18 with the setting coarse = (stride, min_points); (0, anything): the mode is off.
    guess: the call's own guess for the whole cluster, as fused_reference hands it to its pair function."""
    stride, min_points = coarse
    if opt["guess"] == "cluster":
        trec = cf.shape_frame(tpl)
        guess_of = lambda pts: cf.guess(cf.shape_frame(pts), trec)[0]      # (rule C13 on the set that is registered)
    else:
        guess_of = lambda pts: guess
    fine, stats = IC.two_level(src, stride, min_points, lambda pts, g: SINGLE_PAIR(tpl, axes, pts, prm, opt, g), guess_of)
    fine = dict(fine)
    fine["coarse_stats"] = stats
    return fine


def expected(frames_or_depth, prm, templates_by_slot, opt, coarse):
    """fused_reference.expected with every pair run by `pair` above.  The selection among slots (the lower fitness, ties to the
    lower slot) is fused_reference's own, on the records `pair` returns: the fine level's."""
    FR._pair = lambda tpl, axes, src, q, o, guess: pair(tpl, axes, src, q, o, guess, coarse)
    try:
        return FR.expected(frames_or_depth, prm, templates_by_slot, opt)
    finally:
        FR._pair = SINGLE_PAIR


def coarse_stats_of(c):
    """The CoarseStats of a Cluster or of one of its pairs (a dict)."""
    s = c.get("coarse_stats") if isinstance(c, dict) else getattr(c, "coarse_stats", None)
    return IC.NO_STATS if s is None else s


def stats_tuple(s):
    """(n_coarse, coarse_iterations, coarse_converged, coarse_status, the bits of coarse_fitness, used) of a CoarseStats or a
    capi.CdIcpCoarseStats"""
    return (s.n_coarse, s.coarse_iterations, s.coarse_converged, s.coarse_status, int(np.float64(s.coarse_fitness).view(np.uint64)), s.used)
