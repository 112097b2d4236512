"""The truth of one ICP step, from the inputs the device gets (16 uint64 fixed-point moment sums of rule C4, n, the incoming
ICP_STATE, the criteria) - written from the definition, not from icp_solve.hpp: numpy only.

* moments(): mp, mq and sigma = E[q p^T] - mq mp^T in float64 from the integers (shift 32; 36 for the d2 sum); nothing is rounded
  to float32.
* truth(): U, S, Vt = numpy.linalg.svd(sigma), d = sign(det U det Vt), R* = U diag(1, 1, d) Vt - the proper rotation that
  maximises tr(R^T sigma) - and gapmin = min(S0 + S1, S0 + d S2, S1 + d S2), the conditioning of that maximiser.
* figures(): what section "asserted for every record" of the tests reads off a solver's outgoing T, in float64.
* tail(): pcl::registration::DefaultConvergenceCriteria::hasConverged (PCL 1.7.2 / 1.8, no rejected-similar-transform counting:
  max_iterations_similar_transforms_ = 0) and IterativeClosestPoint's final_transformation_ = transformation_ * final_..., given
  the T a solver produced.  Everything float32 there is numpy.float32 in PCL's association, so these fields are bit-exact.

The three calibrated tolerances are NOT taken from the code under test: they are 4 x the worst value of the CPU oracle's float32
solve (oracle_py.umeyama_from_moments) over icp_solve_cases.case_set(), measured by test_icp_solve_truth_cpu.py, which also fails
when the oracle's worst value moves above what is written here.  The device runs the same float32 algorithm; the factor covers
only that nothing in these tests demands equal bits."""
import numpy as np

from perception_amd import icp_plane

# Worst values of the oracle over the case set (records with a finite T; the rotation figure over classes A-F where
# gapmin / S0 >= 1e-3), and the tolerances = 4 x them.  profiles/EXPERIMENTS.md records the measurement.
ORACLE_WORST_ORTH = 1.57e-6    # max |R^T R - I|
ORACLE_WORST_GAP = 1.113e-6    # |S0 + S1 + d S2 - tr(R^T sigma)| / S0
ORACLE_WORST_C = 11.39         # max |R - R*| / (2^-24 S0 / gapmin)
TOL_ORTH = 4 * ORACLE_WORST_ORTH
TOL_GAP = 4 * ORACLE_WORST_GAP
C_ROT = 4 * ORACLE_WORST_C
GAP_FLOOR = 1e-3               # assertion 4 applies where gapmin / S0 >= this
PROPER_FLOOR = 1e-4            # det R > 0 is asserted where S1 / S0 > this
EPS32 = 2.0 ** -24


def _signed(u):
    """uint64 sums as the signed integers they are (two's complement), exactly."""
    return np.ascontiguousarray(u, np.uint64).view(np.int64)


def moments(sums, n):
    """(mp [K, 3], mq [K, 3], sigma [K, 3, 3], mse [K]) in float64 from uint64 sums [K, 16] and counts n [K]."""
    s = _signed(np.asarray(sums, np.uint64).reshape(-1, 16)).astype(np.float64)
    k = np.asarray(n, np.float64).reshape(-1, 1)
    with np.errstate(all="ignore"):
        m = np.ldexp(s[:, :15], -32) / k
        mp, mq = m[:, 0:3], m[:, 3:6]
        sigma = m[:, 6:15].reshape(-1, 3, 3) - mq[:, :, None] * mp[:, None, :]
        mse = np.ldexp(s[:, 15], -36) / k[:, 0]
    return mp, mq, sigma, mse


def truth(sigma):
    """dict(R [K, 3, 3], S [K, 3], d [K], gapmin [K]) of float64 sigmas [K, 3, 3]."""
    U, S, Vt = np.linalg.svd(sigma)
    d = np.where(np.linalg.det(U) * np.linalg.det(Vt) > 0, 1.0, -1.0)
    D = np.zeros_like(sigma)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    s2 = d * S[:, 2]
    gapmin = np.minimum(np.minimum(S[:, 0] + S[:, 1], S[:, 0] + s2), S[:, 1] + s2)
    return dict(R=U @ D @ Vt, S=S, d=d, gapmin=gapmin)


def figures(T, mp, mq, sigma, tr):
    """Of outgoing float32 T [K, 16] (converted to float64 exactly): dict of [K] arrays
       finite  every entry of T is finite (the other figures mean nothing otherwise)
       orth    max |R^T R - I|
       det     det R
       gap     |S0 + S1 + d S2 - tr(R^T sigma)| / S0           (0 where S0 == 0)
       rot     max |R - R*| / (2^-24 S0 / gapmin)               (to compare with C_ROT where gapmin / S0 >= GAP_FLOOR)
       dR      max |R - R*|
       trans   max_i |t_i - (mq - R mp)_i| / (|mq_i| + sum_j |R_ij| |mp_j|)   (0 where the denominator is 0 and t_i exact)
       and last_row: T's last row is 0 0 0 1."""
    T = np.asarray(T, np.float32).reshape(-1, 4, 4).astype(np.float64)
    R, t = T[:, :3, :3], T[:, :3, 3]
    with np.errstate(all="ignore"):
        finite = np.isfinite(T).all(axis=(1, 2))
        orth = np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max(axis=(1, 2))
        S = tr["S"]
        best = S[:, 0] + S[:, 1] + tr["d"] * S[:, 2]
        got = np.einsum("kij,kij->k", R, sigma)
        gap = np.where(S[:, 0] > 0, np.abs(best - got) / S[:, 0], np.abs(best - got))
        dR = np.abs(R - tr["R"]).max(axis=(1, 2))
        rot = dR / (EPS32 * S[:, 0] / tr["gapmin"])
        want_t = mq - np.einsum("kij,kj->ki", R, mp)
        scale = np.abs(mq) + np.einsum("kij,kj->ki", np.abs(R), np.abs(mp))
        err = np.abs(t - want_t)
        trans = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf)).max(axis=1)
    return dict(finite=finite, orth=orth, det=np.linalg.det(np.where(finite[:, None, None], R, 0.0)), gap=gap, rot=rot, dR=dR,
                trans=trans, last_row=(T[:, 3] == [0, 0, 0, 1]).all(axis=1))


def with_truth(case_set):
    """A case set (icp_solve_cases.case_set()) with its float64 moments and truth: adds mp, mq, sigma, truth."""
    c = dict(case_set)
    c["mp"], c["mq"], c["sigma"], _ = moments(c["sums"], c["n"])
    c["truth"] = truth(c["sigma"])
    return c


def assert_solve(T, cases, who, solved=None):
    """Assertions 1-5 on the outgoing T [K, 16] of the records in `solved` (default: all).  Returns the figures."""
    cls, tr = cases["cls"], cases["truth"]
    fig = figures(T, cases["mp"], cases["mq"], cases["sigma"], tr)
    solved = np.ones(len(cls), bool) if solved is None else solved
    S = tr["S"]
    with np.errstate(all="ignore"):
        af = (cls != "G") & solved
        conditioned = af & (tr["gapmin"] >= GAP_FLOOR * S[:, 0])
    assert fig["finite"][af].all(), (who, np.flatnonzero(af & ~fig["finite"])[:8])     # a finite record of A-F is owed an answer
    ok = solved & fig["finite"]
    improper = np.flatnonzero(ok & (fig["det"] <= 0))
    print("%s: %d records, worst orth %.3g gap %.3g C %.3g trans/2^-24 %.3g; improper (rank <= 1, reported): %d, first %s" % (
        who, ok.sum(), fig["orth"][ok].max(), fig["gap"][ok].max(), fig["rot"][conditioned].max(),
        fig["trans"][ok].max() / EPS32, len(improper), improper[:6].tolist()))

    def worst(name, mask, bound):
        bad = np.flatnonzero(mask & ~(fig[name] <= bound))
        assert not len(bad), (who, name, bound, len(bad), [(int(i), str(cls[i]), float(fig[name][i])) for i in bad[:8]])

    assert fig["last_row"][ok].all()
    worst("orth", ok, TOL_ORTH)                                                     # 1
    assert (fig["det"][af] > 0).all(), (who, "det", np.flatnonzero(af & ~(fig["det"] > 0))[:8])   # 2
    assert (S[af, 1] > PROPER_FLOOR * S[af, 0]).all()                               #    (A-F are the records of that rule)
    assert (S[improper, 1] <= PROPER_FLOOR * S[improper, 0]).all()
    worst("gap", ok, TOL_GAP)                                                       # 3
    worst("rot", conditioned, C_ROT)                                                # 4
    worst("trans", ok, 6 * EPS32)                                                   # 5
    return fig, conditioned


def criteria(max_iter=50, trans_eps=1e-8, rel_mse=1e-6, rot_thr=None, abs_mse=1e-12):
    """The criteria of one launch with capi.icp_solve_batch's defaults: rot_thr = 1 - trans_eps unless given."""
    return dict(max_iter=int(max_iter), trans_eps=float(trans_eps), rel_mse=float(rel_mse),
                rot_thr=float(1.0 - trans_eps if rot_thr is None else rot_thr), abs_mse=float(abs_mse))


EXITS = ("stop", "limit", "eps", "abs", "rel", "open")


def tail(T, state, sum_d2, n, crit, bounded):
    """One record: the expected outgoing (T float32 [16], Tfinal float32 [16], iters, prev_mse, converged, done, exit name) given
    the T the solver under test produced.  Rule C8's stop (bounded and n < 3): T = identity, converged = 0, done, nothing else
    moves."""
    f32 = np.float32
    if bounded and n < 3:
        return np.eye(4, dtype=f32).ravel(), state["Tfinal"].copy(), int(state["iters"]), float(state["prev_mse"]), 0, 1, "stop"
    T = np.asarray(T, f32).reshape(16)
    Tfinal = icp_plane.mat4_mul(T, state["Tfinal"]).ravel()
    iters = int(state["iters"]) + 1
    prev = float(state["prev_mse"])
    done, how = 0, "open"
    with np.errstate(all="ignore"):
        if iters >= crit["max_iter"]:
            done, how = 1, "limit"
        else:
            cos_angle = 0.5 * float(((T[0] + T[5]) + T[10]) - f32(1.0))
            translation_sqr = float((T[3] * T[3] + T[7] * T[7]) + T[11] * T[11])
            if cos_angle >= crit["rot_thr"] and translation_sqr <= crit["trans_eps"]:
                done, how = 1, "eps"
            else:
                d2 = int(sum_d2)
                mse = np.float64(float(d2 - (1 << 64) if d2 >= 1 << 63 else d2) * 2.0 ** -36) / np.float64(n)
                if abs(mse - prev) < crit["abs_mse"]:
                    done, how = 1, "abs"
                elif np.float64(abs(mse - prev)) / np.float64(prev) < crit["rel_mse"]:
                    done, how = 1, "rel"
                prev = float(mse)
    return T, Tfinal, iters, prev, done, done, how


def tail_mismatches(out, done, states, sums, n, crit, bounded):
    """Indices of the records of a launch (out ICP_STATE [K], done [K]) whose tail fields are not bit-equal to tail() of their own
    outgoing T, and the count of each exit.  status and the caller's done word must come back untouched."""
    bad, exits = [], dict.fromkeys(EXITS, 0)
    for i in range(len(n)):
        T, Tfinal, iters, prev, conv, dn, how = tail(out["T"][i], states[i], sums[i, 15], int(n[i]), crit, bounded)
        exits[how] += 1
        ok = (out["T"][i].tobytes() == T.tobytes() and out["Tfinal"][i].tobytes() == Tfinal.tobytes() and out["iters"][i] == iters
              and np.float64(out["prev_mse"][i]).tobytes() == np.float64(prev).tobytes() and out["converged"][i] == conv
              and done[i] == dn and out["status"][i] == states["status"][i] and out["done"][i] == states["done"][i])
        if not ok:
            bad.append(i)
    return bad, exits


# ---- single-face clusters end to end ----
POSE_TOL = 1e-4   # BASELINE.json north_star: ICP pose Frobenius error < 1e-4


def assert_planar_input(tpl, scene):
    """By float64 brute force: every moved point's nearest template point is the point it came from (so the first iteration's
    correspondences are known), and the pairs' covariance is rank 2 with S1 / S0 >= 1e-3.  Returns the float64 Umeyama of
    (moved, original): dict(T 4 x 4, R, mp, mq, S, gapmin, bound_R, bound_t [3])."""
    src, q = scene["src"].astype(np.float64), tpl[scene["origin"]].astype(np.float64)
    t64 = tpl.astype(np.float64)
    for a in range(0, len(src), 256):
        d2 = ((src[a:a + 256, None, :] - t64[None, :, :]) ** 2).sum(axis=2)
        assert (d2.argmin(axis=1) == scene["origin"][a:a + 256]).all()
        near = np.sort(d2, axis=1)[:, :2]
        assert (near[:, 0] < near[:, 1]).all()                       # ... strictly: no tie for rule C5 to break
    mp, mq = src.mean(axis=0), q.mean(axis=0)
    sigma = (q - mq).T @ (src - mp) / len(src)
    tr = truth(sigma[None])
    S, gapmin, R = tr["S"][0], float(tr["gapmin"][0]), tr["R"][0]
    assert S[1] >= 1e-3 * S[0] and S[2] <= 1e-6 * S[0] and gapmin >= GAP_FLOOR * S[0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mq - R @ mp
    inv = np.linalg.inv(scene["motion"])
    assert np.abs(T - inv).max() < 1e-6                              # noise-free pairs: the truth IS the inverse motion
    return dict(T=T, R=R, mp=mp, mq=mq, S=S, gapmin=gapmin, inverse=inv, bound_R=C_ROT * EPS32 * S[0] / gapmin)


def assert_planar_first_iteration(T, want, who):
    """A record's final transformation after ONE iteration against the float64 Umeyama `want` of assert_planar_input: rotation
    within assertion 4's bound, translation within assertion 5's bound plus |dR| |mp|, hence the inverse motion; det R > 0."""
    T = np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)
    R, t = T[:3, :3], T[:3, 3]
    dR = np.abs(R - want["R"])
    bound_t = 6 * EPS32 * (np.abs(want["mq"]) + np.abs(R) @ np.abs(want["mp"])) + dR @ np.abs(want["mp"])
    dt = np.abs(t - want["T"][:3, 3])
    print("%s: |dR| %.3g (bound %.3g)  |dt| / its bound %.3g  |T - inverse motion| %.3g" % (
        who, dR.max(), want["bound_R"], (dt / bound_t).max(), np.abs(T - want["inverse"]).max()))
    assert (T[3] == [0, 0, 0, 1]).all() and np.linalg.det(R) > 0, who
    assert dR.max() <= want["bound_R"], (who, dR.max(), want["bound_R"])
    assert (dt <= bound_t).all(), (who, dt, bound_t)
    slack = np.abs(want["T"] - want["inverse"]).max()
    assert np.abs(T - want["inverse"]).max() <= max(want["bound_R"], bound_t.max()) + slack, who


def assert_planar_converged(res, want, who):
    """... with the default iteration limit: converged, and T / pose agree with the inverse motion / the motion to POSE_TOL."""
    T = np.array(res.T, np.float64).reshape(4, 4)
    pose = np.array(res.pose, np.float64).reshape(4, 4)
    print("%s: %d iterations, |T - inverse motion| %.3g, |pose - motion| %.3g" % (
        who, res.iterations, np.linalg.norm(T - want["inverse"]), np.linalg.norm(pose - np.linalg.inv(want["inverse"]))))
    assert res.converged == 1, who
    assert np.linalg.norm(T - want["inverse"]) < POSE_TOL and np.linalg.norm(pose - np.linalg.inv(want["inverse"])) < POSE_TOL, who
    assert np.linalg.det(T[:3, :3]) > 0, who
