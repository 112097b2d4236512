"""The expected result of a cd_icp or of a fused call with reciprocal correspondences on (rule C22), composed on the CPU.  TEST
INFRASTRUCTURE ONLY: the oracle, numpy and the specification modules.

pair() is one (cluster, template) pair under the rule, written as tests/reject_reference.py's: the correspondences are the oracle's
(O.nn, mode 1), the kept set is perception_amd.icp_reciprocal.keep_mask's, the iteration's transformation is the T of the oracle's
own ICP run for ONE iteration, without a guess, on the kept points; the integer-sum MSE, the convergence tail, mat4_mul and xform are
icp_plane's.  With nothing ever rejected it equals O.icp bit for bit, and the kept set equals the oracle's nn composed in both
directions (tests/test_icp_recip_cpu.py asserts both).

expected() is tests/fused_reference.py's composition with every pair run by pair()."""
import collections

import numpy as np

import fused_reference as FR
from oracle import oracle_py as O
from perception_amd import capi, cluster_frame as cf, icp_coarse as IC, icp_plane as IP, icp_reciprocal as IQ

f32, f64 = np.float32, np.float64

# cd_icp_recip_stats
RecipStats = collections.namedtuple("RecipStats", "first_kept last_kept min_kept stopped_few last_n0")
NO_STATS = RecipStats(0, 0, 0, 0, 0)


def keep_by_oracle(tpl, X, nn, d2, d2_max=None):
    """Steps 1 - 3 with the oracle's nn in the reverse direction too: the nearest source point of every template neighbour."""
    k0 = d2 <= (f32(d2_max) if d2_max is not None else f32(np.inf))
    if int(k0.sum()) < IQ.MIN_CORR:
        return k0
    back, _ = O.nn(X, np.ascontiguousarray(tpl[nn]), mode=1)
    return k0 & (back == np.arange(len(X)))


def pair(tpl, src, prm, guess=None, d2_max=None, on=True):
    """Rule C22 for one (cluster, template) pair of at least three points.  prm: the call's cd_params; guess: (4, 4) float32 or
    None; d2_max: rule C8's float32 threshold on d2 (None: unbounded); on = False: nothing but rule C8 rejects (the composition
    with the rule off).  Returns a dict with the fields of fused_reference's pair function plus recip_stats (a RecipStats) and kept
    (the kept count of every iteration that looked for correspondences)."""
    tpl = np.ascontiguousarray(np.asarray(tpl, f32).reshape(-1, 3))
    src = np.ascontiguousarray(np.asarray(src, f32).reshape(-1, 3))
    n_src = len(src)
    assert n_src >= IQ.MIN_CORR
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
    kept, n0s = [], []
    while True:
        nn, d2 = O.nn(tpl, X, mode=1)
        if on:
            keep, n0 = IQ.keep_mask(X, tpl, nn, d2, d2_max)
        else:
            keep = d2 <= (f32(d2_max) if d2_max is not None else f32(np.inf))
            n0 = int(keep.sum())
        n = int(keep.sum())
        kept.append(n)
        n0s.append(n0)
        if n < IQ.MIN_CORR:
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
    stats = RecipStats(kept[0], kept[-1], min(kept), stopped_few, n0s[-1])
    return dict(T=Tfinal, iterations=iters, converged=converged, accepted=accepted, fitness=fitness, plane_stats=None, aligned=X,
                stopped=stopped_few, stopped_few=stopped_few, stopped_singular=0, first_kept=kept[0], recip_stats=stats, kept=kept)


def coarse_pair(tpl, src, prm, coarse, guess=None, d2_max=None, guess_mode="none"):
    """pair() inside rule C18 with the setting coarse = (stride, min_points): (the fine level's dict, its icp_coarse.CoarseStats).
    guess_mode "cluster": rule C13's guess of the set that is registered; otherwise `guess` for both levels."""
    if guess_mode == "cluster":
        trec = cf.shape_frame(np.asarray(tpl, f32).reshape(-1, 3))
        guess_of = lambda pts: cf.guess(cf.shape_frame(pts), trec)[0]
    else:
        guess_of = lambda pts: guess
    return IC.two_level(src, coarse[0], coarse[1], lambda pts, g: pair(tpl, pts, prm, guess=g, d2_max=d2_max), guess_of)


def expected(frames, prm, templates_by_slot, opt):
    """fused_reference.expected with every pair run by pair() above (opt: fused_reference.options(...) with plane=None).  Every
    pair dict, and so every Cluster, gains recip_stats; a cluster that was never run (fewer than three points) has none (stats_of
    gives NO_STATS).  The selection among slots is fused_reference's."""
    assert opt["plane"] is None
    d2_max = None if opt["bound"] is None else FR.correspondence_threshold(opt["bound"])
    saved = FR._pair
    FR._pair = lambda tpl, axes, src, q, o, guess: pair(tpl, src, q, guess=guess, d2_max=d2_max)
    try:
        return FR.expected(frames, prm, templates_by_slot, opt)
    finally:
        FR._pair = saved


def stats_of(c):
    """The RecipStats of a Cluster or of one of its pairs (a dict)."""
    s = c.get("recip_stats") if isinstance(c, dict) else getattr(c, "recip_stats", None)
    return NO_STATS if s is None else s


def stats_tuple(s):
    """(first_kept, last_kept, min_kept, stopped_few, last_n0) of a RecipStats or a capi.CdIcpRecipStats"""
    if isinstance(s, RecipStats):
        return tuple(s)
    return (s.first_kept, s.last_kept, s.min_kept, s.stopped_few, s.last_n0)
