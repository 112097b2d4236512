"""The expected result of a cd_icp or of a fused call with median-distance correspondence rejection on (rule C19), composed on the
CPU.  TEST INFRASTRUCTURE ONLY: the oracle, numpy and the specification modules.

pair() is one (cluster, template) pair under the rule, written as the loop of perception_amd.icp_plane.icp: the correspondences are
the oracle's (O.nn, mode 1), the kept set is perception_amd.icp_reject.keep_mask's, the iteration's transformation is the T of the
oracle's own ICP run for ONE iteration, without a guess, on the kept points (O.icp searches again and finds the same neighbours,
so its estimate is the step over exactly the kept correspondences); the integer-sum MSE, the convergence tail, mat4_mul and xform
are icp_plane's.  With nothing ever rejected it equals O.icp bit for bit (tests/test_icp_reject_cpu.py asserts it).

expected() is tests/fused_reference.py's composition with every pair run by pair() - the way tests/coarse_reference.py puts rule
C18 around fused_reference's pair function; with coarse = (stride, min_points) rule C18 goes around rule C19's pair."""
import collections

import numpy as np

import fused_reference as FR
from oracle import oracle_py as O
from perception_amd import capi, cluster_frame as cf, icp_coarse as IC, icp_plane as IP, icp_reject as IR

f32, f64 = np.float32, np.float64

# cd_icp_reject_stats (last_median as the bits of the float32)
RejectStats = collections.namedtuple("RejectStats", "first_kept last_kept min_kept stopped_few last_median_bits")
NO_STATS = RejectStats(0, 0, 0, 0, 0)


def _bits(v):
    return int(np.array([v], f32).view(np.uint32)[0])


def pair(tpl, src, prm, factor, guess=None, d2_max=None):
    """Rule C19 for one (cluster, template) pair of at least three points.  prm: the call's cd_params; guess: (4, 4) float32 or
    None; d2_max: rule C8's float32 threshold on d2 (None: unbounded).  Returns a dict with the fields of fused_reference's pair
    function plus reject_stats (a RejectStats) and kept (the kept count of every iteration that looked for correspondences)."""
    tpl = np.ascontiguousarray(np.asarray(tpl, f32).reshape(-1, 3))
    src = np.ascontiguousarray(np.asarray(src, f32).reshape(-1, 3))
    n_src = len(src)
    assert n_src >= IR.MIN_CORR and IR.valid_factor(factor)
    one = FR.copy_params(prm)
    one.icp_max_iterations = 1
    one.icp_use_guess = capi.CD_GUESS_NONE
    max_iter = int(prm.icp_max_iterations)
    trans_eps = f64(prm.icp_transformation_epsilon)
    rel_mse = f64(prm.icp_euclidean_fitness_epsilon)
    rot_thr = f64(1.0) - trans_eps
    abs_mse = f64(1e-12)
    Tfinal = np.eye(4, dtype=f32) if guess is None else np.asarray(guess, f32).reshape(4, 4).copy()
    X = src.copy() if guess is None else IP.xform(Tfinal, src)
    prev_mse = np.finfo(f64).max
    iters = converged = stopped_few = 0
    kept, last_m = [], f32(0.0)
    while True:
        _, d2 = O.nn(tpl, X, mode=1)
        keep, m, _, _ = IR.keep_mask(d2, factor, d2_max)
        n = int(keep.sum())
        kept.append(n)
        if m is not None:
            last_m = m
        if n < IR.MIN_CORR:
            stopped_few = 1
            break
        st, r, _ = O.icp(tpl, np.ascontiguousarray(X[keep]), one, nn_mode=1)
        assert st == 0 and r.iterations == 1
        T = np.array(list(r.T), f32).reshape(4, 4)
        with np.errstate(over="ignore"):
            mse = IP.unfix(IP.fix(d2[keep], IP.FIX_SHIFT_D2).sum(dtype=np.int64), IP.FIX_SHIFT_D2) / f64(n)
        Tfinal = IP.mat4_mul(T, Tfinal)
        iters += 1
        done = 0
        if iters >= max_iter:
            done = 1
        else:
            with np.errstate(all="ignore"):
                cos_angle = f64(0.5) * f64(((T[0, 0] + T[1, 1]) + T[2, 2]) - f32(1.0))
                translation_sqr = f64((T[0, 3] * T[0, 3] + T[1, 3] * T[1, 3]) + T[2, 3] * T[2, 3])
                if cos_angle >= rot_thr and translation_sqr <= trans_eps:
                    done = 1
                else:
                    if abs(mse - prev_mse) < abs_mse:
                        done = 1
                    elif abs(mse - prev_mse) / prev_mse < rel_mse:
                        done = 1
                    prev_mse = mse
        X = IP.xform(T, X)
        if done:
            converged = 1
            break
    _, d2f = O.nn(tpl, IP.xform(Tfinal, src), mode=1)
    with np.errstate(over="ignore"):
        sf = IP.fix(d2f, IP.FIX_SHIFT_D2).sum(dtype=np.int64)
    fitness = float(IP.unfix(sf, IP.FIX_SHIFT_D2) / f64(n_src))
    accepted = 1 if (converged and fitness < float(prm.icp_accept_fitness)) else 0
    stats = RejectStats(kept[0], kept[-1], min(kept), stopped_few, _bits(last_m))
    return dict(T=Tfinal, iterations=iters, converged=converged, accepted=accepted, fitness=fitness, plane_stats=None, aligned=X,
                stopped=stopped_few, stopped_few=stopped_few, stopped_singular=0, first_kept=kept[0], reject_stats=stats, kept=kept)


def coarse_pair(tpl, src, prm, factor, coarse, guess=None, d2_max=None, guess_mode="none"):
    """pair() inside rule C18 with the setting coarse = (stride, min_points): (the fine level's dict, its icp_coarse.CoarseStats).
    guess_mode "cluster": rule C13's guess of the set that is registered; otherwise `guess` for both levels."""
    if guess_mode == "cluster":
        trec = cf.shape_frame(np.asarray(tpl, f32).reshape(-1, 3))
        guess_of = lambda pts: cf.guess(cf.shape_frame(pts), trec)[0]
    else:
        guess_of = lambda pts: guess
    return IC.two_level(src, coarse[0], coarse[1], lambda pts, g: pair(tpl, pts, prm, factor, guess=g, d2_max=d2_max), guess_of)


def expected(frames, prm, templates_by_slot, opt, factor):
    """fused_reference.expected with every pair run by pair() above (opt: fused_reference.options(...) with plane=None; a bound is
    allowed here, the rule's own reference has one).  Every pair dict, and so every Cluster, gains reject_stats; a cluster that was
    never run (fewer than three points) has none (stats_of gives NO_STATS).  The selection among slots is fused_reference's."""
    assert opt["plane"] is None
    d2_max = None if opt["bound"] is None else FR.correspondence_threshold(opt["bound"])
    saved = FR._pair
    FR._pair = lambda tpl, axes, src, q, o, guess: pair(tpl, src, q, factor, guess=guess, d2_max=d2_max)
    try:
        return FR.expected(frames, prm, templates_by_slot, opt)
    finally:
        FR._pair = saved


def stats_of(c):
    """The RejectStats of a Cluster or of one of its pairs (a dict)."""
    s = c.get("reject_stats") if isinstance(c, dict) else getattr(c, "reject_stats", None)
    return NO_STATS if s is None else s


def stats_tuple(s):
    """(first_kept, last_kept, min_kept, stopped_few, the bits of last_median) of a RejectStats or a capi.CdIcpRejectStats"""
    if isinstance(s, RejectStats):
        return tuple(s)
    return (s.first_kept, s.last_kept, s.min_kept, s.stopped_few, _bits(s.last_median))


def contamination_scene(tpl, seed, n_object=1500, n_blob=300, max_angle_deg=4.0, max_shift=0.008, noise=0.0007, gap=0.004, blob_radius=0.015):
    """A source cloud with points the template has no counterpart for: n_object template points (all of them when it has fewer)
    moved by a rotation of up to max_angle_deg about a random axis through their centroid and a shift of up to max_shift, with
    Gaussian noise, plus a ball of n_blob points whose surface lies `gap` beside the object's box along +x.  Deterministic in
    the seed.  Returns (source (n, 3) float32, truth (4, 4) float64: the motion that was applied to the template points)."""
    rng = np.random.default_rng(seed)
    t = np.asarray(tpl, f64).reshape(-1, 3)
    pick = np.sort(rng.choice(len(t), min(n_object, len(t)), replace=False))
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = np.deg2rad(max_angle_deg) * rng.uniform(0.5, 1.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    shift = rng.normal(size=3)
    shift *= max_shift * rng.uniform(0.5, 1.0) / np.linalg.norm(shift)
    c = t[pick].mean(axis=0)
    truth = np.eye(4)
    truth[:3, :3] = R
    truth[:3, 3] = c - R @ c + shift
    obj = t[pick] @ R.T + truth[:3, 3] + rng.normal(scale=noise, size=(len(pick), 3))
    lo, hi = obj.min(axis=0), obj.max(axis=0)
    centre = np.array([hi[0] + gap + blob_radius, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])])
    d = rng.normal(size=(n_blob, 3))
    d *= (blob_radius * rng.uniform(size=n_blob) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    return np.ascontiguousarray(np.vstack([obj, centre + d]), f32), truth


def translation_error(T, truth):
    """|| t(T) - t(truth^-1) ||: how far the registration's translation is from the one that undoes the scene's motion."""
    return float(np.linalg.norm(np.asarray(T, f64).reshape(4, 4)[:3, 3] - np.linalg.inv(truth)[:3, 3]))
