"""The plane stage (S2, and the flags of S3) in float64, written from PCL's definitions and from nothing of this project:
numpy and the standard library only, no import from oracle/, no float32 arithmetic.

What is restated
  generator    std::mt19937 (mt19937 below), checked against the C++ standard's known answer: seed 5489, 10000th output 4123659995
  sampler      SampleConsensusModel::drawIndexSample: the identity permutation, kept across draws; a draw is three swaps,
               i = 0, 1, 2 with j = i + (mt >> 1) % (n - i); the sample is positions 0, 1, 2.  isSampleGood rejects a sample whose
               three component ratios of (p1 - p0) / (p2 - p0) are equal; here that is decided in exact arithmetic
               (cross-multiplication of fractions).  A sample whose ratios differ by less than NEAR_DEGENERATE relative is
               NEAR-DEGENERATE: a float32 implementation may legitimately decide it either way, so a case that visits one is
               inadmissible for a truth test
  hypothesis   n = (p1 - p0) x (p2 - p0) / |.|, d = -n . p0, kappa = |a| |b| / |a x b| with a = p1 - p0, b = p2 - p0
  distance     |n . p + d|
  loop         pcl::RandomSampleConsensus::computeModel: c > best updates best and k = log(1 - prob) / log(clamp(1 - w^3)),
               w = best / n; the loop runs while iterations < k (and skipped < 10 max_iterations, which is what makes
               max_iterations = 0 return no model) and ends when iterations > max_iterations
  refit        optimizeModelCoefficients: the total-least-squares plane of the inliers (float64 covariance, numpy.linalg.eigh, the
               smallest eigenvector, its sign aligned to the best model), left alone for fewer than 4 inliers as PCL leaves it

The band: how far a float32 evaluation of a hypothesis' distance may be from the float64 one
  u = 2^-24.  The float32 chain (computeModelCoefficients + the distance) and its first-order error, kappa >= 1:
    the three differences of a and of b             each component relative u
    cross product m = a x b                         two products and one subtraction per component: with the 2 u of the inputs a
                                                    product carries 3 u, the subtraction adds u of the result, so
                                                    |dm_x| <= 4 u (|a_y b_z| + |a_z b_y|) and, summing the squares (Cauchy-Schwarz:
                                                    sum_i (A - a_i^2)(B - b_i^2) <= 2 A B), |dm| <= 4 sqrt(2) u |a| |b|
    norm and division                               three squares and two additions (3 u on the squared norm, 1.5 u on the norm),
                                                    the square root (u) and the division (u): 3.5 u on the length of n
      => |dn| <= (5.66 kappa + 3.5) u <= 9.2 kappa u                                  (|a| |b| / |m| = kappa)
    d = -(n . p0)                                   three products, two additions (the factor -1 is exact): <= 3 u |p0| beside
                                                    -(n + dn) . p0
    plane_dist                                      its products and additions on terms of size |p| and |d|: <= 3 u (|p| + |d|)
                                                    <= 6 u max|p|
    thr                                             one rounding of the threshold (fold_ge): u thr <= u max|p|
  The float32 value is (n + dn) . (p - p0) + e with |e| <= 10 u max|p|, so it differs from the float64 distance by at most
    u kappa (9.2 max|p - p0| + 10 max|p|) <= 10 u kappa (3 max|p - p0| + max|p|).
  The derived constant is 10; C_BAND is the next power of two, 16, which also covers the second-order terms while kappa u < 0.1
  (near-degenerate samples are excluded long before).  It is never tuned down to make a case admissible.  Measured with the CPU
  oracle's float32 distances on six clouds of 300 to 6145 points, 300 hypotheses each: below 0.053 of the band, and not one
  classification difference between float32 and float64.
  The same count bounds the model a float32 implementation returns: |dn| <= C_BAND u kappa and |dd| <= C_BAND u kappa |p0|.

The refined model has no derived bound (pcl::eigen33 is a closed form in float32 whose error depends on the spectrum); its
tolerance is MEASURED, with the CPU oracle over the committed case set (tests/test_plane_truth_cpu.py), and written down here:"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
C_BAND = 16.0
NEAR_DEGENERATE = 1e-5
PCL_SEED = 12345
MAX_SAMPLE_CHECKS = 1000

# Measured by tests/test_plane_truth_cpu.py::test_oracle_meets_the_truth_and_sets_the_refit_tolerance: the largest angle
# (radians) between the CPU oracle's refined normal and the float64 total-least-squares normal, and the largest |d - d64|, over
# every case of tests/plane_cases.py with plane_optimize = 1.  The tolerance is twice that: the cases only sample the spectrum.
ORACLE_WORST_REFIT_ANGLE = 9.74e-7
ORACLE_WORST_REFIT_D = 2.77e-7
TOL_REFIT_ANGLE = 2.0 * ORACLE_WORST_REFIT_ANGLE
TOL_REFIT_D = 2.0 * ORACLE_WORST_REFIT_D
REFIT_ANGLE_CEILING = 1e-4      # a measured angle above this is a finding, not a tolerance


# ---- generator -----------------------------------------------------------------------------------------------------------------

def mt19937(seed, count):
    """The first `count` outputs of std::mt19937(seed), uint32."""
    mt = np.zeros(624, np.uint64)
    mt[0] = seed & 0xffffffff
    for i in range(1, 624):
        mt[i] = (1812433253 * (int(mt[i - 1]) ^ (int(mt[i - 1]) >> 30)) + i) & 0xffffffff
    out = np.empty(((count + 623) // 624) * 624, np.uint32)

    def twist(cur, nxt, far):
        y = (cur & np.uint64(0x80000000)) | (nxt & np.uint64(0x7fffffff))
        return far ^ (y >> np.uint64(1)) ^ ((y & np.uint64(1)) * np.uint64(0x9908b0df))

    for blk in range(len(out) // 624):
        # mt[i] <- mt[i + 397] ^ f(mt[i], mt[i + 1]): in runs whose inputs are all settled
        mt[0:227] = twist(mt[0:227], mt[1:228], mt[397:624])
        mt[227:454] = twist(mt[227:454], mt[228:455], mt[0:227])
        mt[454:623] = twist(mt[454:623], mt[455:624], mt[227:396])
        mt[623] = twist(mt[623:624], mt[0:1], mt[396:397])[0]
        y = mt.copy()
        y ^= y >> np.uint64(11)
        y ^= (y << np.uint64(7)) & np.uint64(0x9d2c5680)
        y ^= (y << np.uint64(15)) & np.uint64(0xefc60000)
        y ^= y >> np.uint64(18)
        out[624 * blk:624 * blk + 624] = y.astype(np.uint32)
    return out[:count]


# ---- sampler -------------------------------------------------------------------------------------------------------------------

def sample_class(p0, p1, p2):
    """(degenerate, near_degenerate) of one sample of float32 points: exact where it matters."""
    a = np.asarray(p1, np.float64) - np.asarray(p0, np.float64)
    b = np.asarray(p2, np.float64) - np.asarray(p0, np.float64)
    near = True
    for i, j in ((0, 1), (2, 1)):                      # ratio i against ratio j: a_i / b_i = a_j / b_j <=> a_i b_j = a_j b_i
        l, r = a[i] * b[j], a[j] * b[i]
        if abs(l - r) >= NEAR_DEGENERATE * max(abs(l), abs(r)) and (l != 0.0 or r != 0.0):
            near = False
    if not near:
        return False, False
    fa = [Fraction(float(p1[k])) - Fraction(float(p0[k])) for k in range(3)]
    fb = [Fraction(float(p2[k])) - Fraction(float(p0[k])) for k in range(3)]
    degenerate = fa[0] * fb[1] == fa[1] * fb[0] and fa[2] * fb[1] == fa[1] * fb[2]
    return degenerate, not degenerate


class Sampler:
    """drawIndexSample on the shuffled index vector of n points, kept as the positions that differ from the identity."""

    def __init__(self, n, rnd=None, draws=1 << 15):
        self.n = n
        self.rnd = (mt19937(PCL_SEED, draws) if rnd is None else rnd).astype(np.int64) >> 1
        self.rp = 0
        self.map = {}

    def draw(self):
        m, n = self.map, self.n
        for i in range(3):
            j = i + int(self.rnd[self.rp]) % (n - i)
            self.rp += 1
            m[i], m[j] = m.get(j, j), m.get(i, i)
        return m[0], m[1], m[2]


def draw_hypotheses(P, count):
    """The first `count` samples getSamples hands to computeModelCoefficients (exactly degenerate ones redrawn, as isSampleGood
    does).  Returns (triples int [h, 3], near bool: a near-degenerate sample was visited, rejected int: samples redrawn); h < count
    when MAX_SAMPLE_CHECKS draws in a row were degenerate ("No samples could be selected")."""
    P = np.asarray(P)
    tri, near_any, rejected = [], False, 0
    if len(P) < 3:
        return np.zeros((0, 3), np.int64), False, 0
    s = Sampler(len(P), draws=3 * (count + MAX_SAMPLE_CHECKS) + 3)
    for _ in range(count):
        good = False
        for _check in range(MAX_SAMPLE_CHECKS):
            if s.rp + 3 > len(s.rnd):
                s.rnd = mt19937(PCL_SEED, 2 * len(s.rnd)).astype(np.int64) >> 1
            t = s.draw()
            deg, near = sample_class(P[t[0]], P[t[1]], P[t[2]])
            near_any = near_any or near
            if not deg:
                good = True
                break
            rejected += 1
        if not good:
            break
        tri.append(t)
    return np.array(tri, np.int64).reshape(-1, 3), near_any, rejected


# ---- hypotheses, bands, counts ---------------------------------------------------------------------------------------------------

def plane_models(P, tri):
    """float64 (normals [h, 3], d [h], kappa [h]) of the samples."""
    P = np.asarray(P, np.float64)
    p0 = P[tri[:, 0]]
    a, b = P[tri[:, 1]] - p0, P[tri[:, 2]] - p0
    m = np.cross(a, b)
    nm = np.linalg.norm(m, axis=1)
    n = m / nm[:, None]
    return n, -np.einsum("ij,ij->i", n, p0), np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) / nm


def bands(P, tri, kappa):
    P = np.asarray(P, np.float64)
    far = np.array([np.linalg.norm(P - P[t], axis=1).max() for t in tri[:, 0]]) if len(tri) else np.zeros(0)
    return C_BAND * U * kappa * (3.0 * far + np.linalg.norm(P, axis=1).max())


def count_intervals(P, n, d, band, thr):
    """[lo, hi] per hypothesis: the points inside thr - band and inside thr + band (strictly, as PCL's `<`)."""
    dist = np.abs(n @ np.asarray(P, np.float64).T + d[:, None])
    return (dist < (thr - band)[:, None]).sum(1), (dist < (thr + band)[:, None]).sum(1)


class Intervals:
    """The count intervals of a cloud's hypotheses under one threshold, computed CHUNK hypotheses at a time as the loop asks."""
    CHUNK = 32

    def __init__(self, hyp, thr):
        self.hyp, self.thr, self.lo, self.hi = hyp, thr, np.zeros(0, np.int64), np.zeros(0, np.int64)

    def __len__(self):
        return len(self.hyp.tri)

    def __getitem__(self, h):
        while h >= len(self.lo):
            s = slice(len(self.lo), len(self.lo) + self.CHUNK)
            lo, hi = count_intervals(self.hyp.P, self.hyp.n[s], self.hyp.d[s], self.hyp.band_of(s), self.thr)
            self.lo, self.hi = np.concatenate([self.lo, lo]), np.concatenate([self.hi, hi])
        return int(self.lo[h]), int(self.hi[h])


def stop_k(c, n_points, prob):
    w = c / float(n_points)
    p = 1.0 - w ** 3
    eps = np.finfo(np.float64).eps
    p = min(max(p, eps), 1.0 - eps)
    return math.log(1.0 - prob) / math.log(p)


def replay(intervals, n_points, max_iter, prob):
    """PCL's loop on the count intervals (intervals[h] = (lo, hi), len(intervals) hypotheses drawn).  Returns (robust, iterations, best_h): robust is False as soon as an interval could change
    a comparison or the stop, or when the loop needs a hypothesis that was not drawn."""
    it, best_h = 0, -1
    best_lo = best_hi = None
    k_min = k_max = 1.0                                 # k from the interval's upper and lower end
    if max_iter * 10 <= 0:                              # skipped (0) < max_skip fails before the first draw
        return True, 0, -1
    while True:
        if it >= k_max:
            break
        if not it < k_min:
            return False, it, best_h
        if it >= len(intervals):
            return False, it, best_h
        h = it
        lo, hi = intervals[h]
        if best_lo is None or lo > best_hi:
            best_lo, best_hi, best_h = lo, hi, h
            k_max, k_min = stop_k(best_lo, n_points, prob), stop_k(best_hi, n_points, prob)
        elif hi > best_lo:
            return False, it, best_h
        it += 1
        if it > max_iter:
            break
    return True, it, best_h


def tls_plane(Q, like):
    """Total-least-squares plane of the points Q, the normal's sign aligned to `like`."""
    c = Q.mean(0)
    w, v = np.linalg.eigh((Q - c).T @ (Q - c) / len(Q))
    n = v[:, 0]
    if n @ like < 0:
        n = -n
    return n, -float(n @ c)


def refit_band(P):
    """How far the distance to a refined plane within the refit tolerance, evaluated in float32, may be from the float64 one."""
    far = float(np.linalg.norm(np.asarray(P, np.float64), axis=1).max())
    return TOL_REFIT_ANGLE * far + TOL_REFIT_D + 8.0 * U * 2.0 * far


class Hypotheses:
    """Everything of a cloud that does not depend on the parameters: samples, models, bands."""

    def __init__(self, P, count=1001):
        self.P = np.asarray(P, np.float32)
        self.tri, self.near, self.rejected = draw_hypotheses(self.P, count)
        self.wanted = count
        self.n, self.d, self.kappa = plane_models(self.P, self.tri) if len(self.tri) else (np.zeros((0, 3)), np.zeros(0), np.zeros(0))
        self._band = np.zeros(0)
        self._counts = {}

    def band_of(self, s):
        """bands of the hypotheses of slice s (computed in order, once)"""
        stop = min(s.stop, len(self.tri))
        if stop > len(self._band):
            t = slice(len(self._band), stop)
            self._band = np.concatenate([self._band, bands(self.P, self.tri[t], self.kappa[t])])
        return self._band[s]

    def counts(self, thr):
        if thr not in self._counts:
            self._counts[thr] = Intervals(self, thr)
        return self._counts[thr]


def truth(hyp, thr, max_iter, prob, optimize=1):
    """The float64 answer of pcl::SACSegmentation on hyp.P.  Keys: admissible, robust, iterations, best_h (-1: no model), normal,
    d, kappa, p0 (the best sample's first point), sure / ambiguous (inlier indices of the best model), refined_normal, refined_d,
    refined_sure / refined_ambiguous.  admissible: robust, no near-degenerate or rejected sample, and - with optimize, where the
    best model's inliers are the input of the refit - no ambiguous inlier of the best model: whether a point is part of that
    input is a comparison like any other, and one point more or less moves the refined plane by far more than any rounding."""
    P64 = hyp.P.astype(np.float64)
    robust, it, bh = replay(hyp.counts(thr), len(hyp.P), max_iter, prob) if len(hyp.P) >= 3 else (True, 0, -1)
    out = dict(robust=robust, admissible=robust and not hyp.near and hyp.rejected == 0, iterations=it, best_h=bh)
    if bh < 0 or not robust:
        return out
    n, d, band = hyp.n[bh], hyp.d[bh], hyp.band_of(slice(bh, bh + 1))[0]
    dist = np.abs(P64 @ n + d)
    sure = np.flatnonzero(dist < thr - band)
    amb = np.flatnonzero((dist < thr + band) & ~(dist < thr - band))
    out.update(normal=n, d=float(d), kappa=float(hyp.kappa[bh]), band=float(band), p0=P64[hyp.tri[bh, 0]], sure=sure, ambiguous=amb)
    out["admissible"] = out["admissible"] and not (optimize and len(amb))
    inl = np.union1d(sure, amb)
    if len(inl) < 4:
        rn, rd, rband = n, float(d), band
    else:
        rn, rd = tls_plane(P64[inl], n)
        rband = refit_band(hyp.P)
    rdist = np.abs(P64 @ rn + rd)
    out.update(refined_normal=rn, refined_d=rd, refined_band=float(rband), refined_sure=np.flatnonzero(rdist < thr - rband),
               refined_ambiguous=np.flatnonzero((rdist < thr + rband) & ~(rdist < thr - rband)))
    return out


# ---- what an implementation is held to -----------------------------------------------------------------------------------------

def angle(a, b):
    """Angle between two directions, up to sign (pcl::eigen33 does not orient its eigenvector)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(math.atan2(np.linalg.norm(np.cross(a, b)), abs(a @ b)))


def assert_against_truth(tr, status, coeff, inliers, iterations, optimize, who, measure=None):
    """One result (status, float32 coeff, inlier indices, iteration count) of an implementation against truth `tr` of an
    admissible case.  measure: a dict that collects the refined model's angle and |dd| instead of asserting them."""
    assert tr["admissible"], who
    assert iterations == tr["iterations"], (who, iterations, tr["iterations"])
    if tr["best_h"] < 0:
        assert status != 0 and len(inliers) == 0, (who, status)
        return
    assert status == 0, (who, status)
    c = np.asarray(coeff, np.float64)
    inl = np.asarray(inliers, np.int64)
    assert np.all(np.diff(inl) > 0), who
    refit = optimize and len(tr["sure"]) + len(tr["ambiguous"]) >= 4
    if not refit:
        bound = C_BAND * U * tr["kappa"]
        dn = float(np.linalg.norm(c[:3] - tr["normal"]))
        dd = abs(c[3] - tr["d"])
        assert dn <= bound, (who, "normal", dn, bound)
        assert dd <= bound * np.linalg.norm(tr["p0"]), (who, "d", dd, bound)
        sure, amb = tr["sure"], tr["ambiguous"]
    else:
        ang = angle(c[:3], tr["refined_normal"])
        sgn = 1.0 if c[:3] @ tr["refined_normal"] >= 0 else -1.0
        dd = abs(sgn * c[3] - tr["refined_d"])
        assert abs(np.linalg.norm(c[:3]) - 1.0) <= 8 * U, (who, "unit normal")
        if measure is not None:
            measure["angle"] = max(measure.get("angle", 0.0), ang)
            measure["d"] = max(measure.get("d", 0.0), dd)
            if ang > REFIT_ANGLE_CEILING:               # (the largest eigenvector is about pi / 2 away)
                raise AssertionError((who, "refined normal", ang))
        else:
            assert ang <= TOL_REFIT_ANGLE, (who, "refined normal", ang, TOL_REFIT_ANGLE)
            assert dd <= TOL_REFIT_D, (who, "refined d", dd, TOL_REFIT_D)
        sure, amb = tr["refined_sure"], tr["refined_ambiguous"]
        if measure is not None:                         # (the refined sets' band comes from the tolerance being measured)
            return
    missing = np.setdiff1d(sure, inl)
    extra = np.setdiff1d(inl, np.union1d(sure, amb))
    assert len(missing) == 0 and len(extra) == 0, (who, "inliers", missing[:8], extra[:8], len(sure), len(amb), len(inl))
