"""The plane stage held to a float64 answer written from PCL's definitions (tests/plane_reference.py), on the CPU: the reference
checks itself, the committed case set (tests/plane_cases.py) meets its conditions by the reference alone, and the CPU oracle -
which every GPU plane test is compared with, bit for bit - is held to the truth on every case.  That is what gives "GPU == oracle"
its meaning for this stage; tests/test_gpu_plane_truth.py holds the device to the same assertions directly.

Per case and parameter set (REF.assert_against_truth):
  iteration count                  equal
  unrefined model (optimize = 0)   |dn| <= C_BAND 2^-24 kappa, |dd| <= C_BAND 2^-24 kappa |p0| (derived in plane_reference.py)
  inlier indices                   a superset of the sure set, a subset of sure + ambiguous
  refined model (optimize = 1)     angle to the float64 total-least-squares normal and |dd| MEASURED here over the case set; the
                                   tolerance is twice the largest value, written into plane_reference.py with its provenance"""
import numpy as np
import pytest

import plane_cases as CS
import plane_reference as REF


def test_generator_known_answers(O):
    assert int(REF.mt19937(5489, 10000)[-1]) == 4123659995          # the C++ standard's check value of std::mt19937
    assert np.array_equal(REF.mt19937(12345, 3000), O.mt19937_stream(12345, 3000))


def test_sampler_is_a_partial_fisher_yates():
    """every sample is three distinct indices below n, and the kept permutation stays a permutation"""
    s = REF.Sampler(5)
    for _ in range(200):
        t = s.draw()
        assert len(set(t)) == 3 and all(0 <= i < 5 for i in t)
        assert sorted(s.map.get(i, i) for i in range(5)) == list(range(5))


def exact_plane_cloud(seed):
    """120 points EXACTLY on z = 0.25 + 0.5 x + 0.25 y (x, y multiples of 2^-10, so z is a float32) and 80 points at least 0.04 off"""
    rng = np.random.RandomState(seed)
    xy = rng.randint(-190, 191, (200, 2)) / 1024.0
    z = 0.25 + 0.5 * xy[:, 0] + 0.25 * xy[:, 1]
    z[120:] += rng.choice([-1.0, 1.0], 80) * rng.uniform(0.05, 0.2, 80)
    P = np.column_stack([xy, z])
    assert np.array_equal(P[:120].astype(np.float32).astype(np.float64), P[:120])
    order = rng.permutation(200)
    return P[order].astype(np.float32), np.sort(np.argsort(order)[:120])


def test_reference_on_an_exactly_constructed_plane():
    P, on_plane = exact_plane_cloud(1)
    want = np.array([-0.5, -0.25, 1.0]) / np.linalg.norm([-0.5, -0.25, 1.0])
    for optimize, max_iter, thr, prob in CS.PARAMS:
        tr = REF.truth(REF.Hypotheses(P), thr, max_iter, prob, optimize)
        assert tr["admissible"]
        if max_iter == 0:
            assert tr["best_h"] == -1 and tr["iterations"] == 0
            continue
        if max_iter == 5 and not np.isin(REF.Hypotheses(P).tri[tr["best_h"]], on_plane).all():
            continue                                    # (six hypotheses need not hold a sample of the plane)
        assert np.array_equal(tr["sure"], on_plane) and len(tr["ambiguous"]) == 0
        assert np.array_equal(tr["refined_sure"], on_plane) and len(tr["refined_ambiguous"]) == 0
        for n, d in ((tr["normal"], tr["d"]), (tr["refined_normal"], tr["refined_d"])):
            sgn = 1.0 if n @ want > 0 else -1.0
            assert np.abs(sgn * n - want).max() <= 1e-12 and abs(sgn * d + 0.25 * want[2]) <= 1e-12


def test_case_set_is_admissible_and_reaches_every_round():
    """The conditions of the case set, by the reference alone: no case is left out anywhere."""
    per_round = {1: [], 2: [], 3: [], 4: []}
    inadmissible = []
    for name, n, rnd, P, tr in CS.truth_set():
        assert len(P) == n and np.abs(P).max() <= 1.0
        cells = np.floor(P.astype(np.float64) / CS.LEAF).astype(np.int64)
        assert len(np.unique(cells, axis=0)) == n                                     # one point per voxel ...
        assert sorted(map(tuple, cells[:, ::-1])) == list(map(tuple, cells[:, ::-1]))  # ... in voxel order
        inadmissible += [(name, t) for t in CS.PARAMS if not tr[t]["admissible"]]
        it = tr[CS.DEFAULTS]["iterations"]
        lo, hi = CS.ROUND_RANGE[rnd]
        assert lo <= it <= hi, (name, it)
        per_round[rnd].append("%s:%d" % (name, it))
        assert n <= 4 or tr[(1, 5, 0.015, 0.99)]["iterations"] == 6, name    # plane_max_iterations = 5 is what stops these
    for rnd in per_round:
        print("round %d: %s" % (rnd, " ".join(per_round[rnd])))
    print("inadmissible cases: %d" % len(inadmissible))
    assert not inadmissible, inadmissible
    assert {n for _, n, _, _, _ in CS.truth_set()} == {3, 4} | set(CS.COUNTS)
    assert any(tr[CS.DEFAULTS]["iterations"] == 1001 for _, _, _, _, tr in CS.truth_set()), "no case runs to max_iterations + 1"


def test_oracle_meets_the_truth_and_sets_the_refit_tolerance(O):
    """Every case and parameter set through the CPU oracle.  The first pass measures the refined model; the constants of
    plane_reference.py must be what is measured (a value that moved is a failure), and the second pass holds the refined
    inlier sets to the band those constants give."""
    measured = {}
    results = []
    for name, n, rnd, P, tr in CS.truth_set():
        for t in CS.PARAMS:
            st, coeff, inl, it = O.segment_plane(P, CS.params(t))
            results.append((name, t, tr[t], st, coeff, inl, it))
            REF.assert_against_truth(tr[t], st, coeff, inl, it, t[0], "oracle %s %s" % (name, t), measure=measured)
    print("refined model, oracle against float64: largest angle %.6g rad, largest |dd| %.6g" % (measured["angle"], measured["d"]))
    assert measured["angle"] <= REF.REFIT_ANGLE_CEILING
    assert measured["angle"] <= REF.ORACLE_WORST_REFIT_ANGLE <= 1.01 * measured["angle"]
    assert measured["d"] <= REF.ORACLE_WORST_REFIT_D <= 1.01 * measured["d"]
    assert REF.TOL_REFIT_ANGLE == 2 * REF.ORACLE_WORST_REFIT_ANGLE and REF.TOL_REFIT_D == 2 * REF.ORACLE_WORST_REFIT_D
    for name, t, tr, st, coeff, inl, it in results:
        REF.assert_against_truth(tr, st, coeff, inl, it, t[0], "oracle %s %s" % (name, t))


class ExactIntervals:
    """The count intervals of boundary_cloud(): a sample of three points of the plane z = 0.5 gives the model (0, 0, +-1, -+0.5)
    without a rounding in float32 as in float64, and every coordinate is dyadic, so its distances are exact and its band is zero;
    every other hypothesis keeps the reference's band."""

    def __init__(self, hyp, thr, on_plane, strict=True):
        self.inner, self.hyp, self.thr, self.on_plane, self.strict = hyp.counts(thr), hyp, thr, on_plane, strict

    def __len__(self):
        return len(self.inner)

    def exact(self, h):
        return bool(self.on_plane[self.hyp.tri[h]].all())

    def __getitem__(self, h):
        if self.exact(h):
            dist = np.abs(self.hyp.P[:, 2].astype(np.float64) - 0.5)
            c = int((dist < self.thr).sum() if self.strict else (dist <= self.thr).sum())
            return c, c
        return self.inner[h]


def boundary_cloud(seed):
    """100 points exactly on z = 0.5, 60 at EXACTLY the threshold 2^-6 from it (either side), 40 far away; x and y multiples of 2^-10"""
    rng = np.random.RandomState(seed)
    xy = rng.randint(-190, 191, (200, 2)) / 1024.0
    z = np.full(200, 0.5)
    z[100:160] += rng.choice([-1.0, 1.0], 60) * 2.0 ** -6
    z[160:] += rng.choice([-1.0, 1.0], 40) * rng.randint(64, 256, 40) / 1024.0
    order = rng.permutation(200)
    P = np.column_stack([xy, z])[order].astype(np.float32)
    return P, P[:, 2] == 0.5


def test_the_threshold_is_strict(O):
    """PCL counts and selects with `<`.  No cloud of the case set has a point at exactly the threshold (0.015 and 0.004 are no
    float32 values), so this cloud has 60, around a plane whose arithmetic is exact: counted in, a sample of that plane scores
    160 instead of 100 and PCL's loop ends at another iteration."""
    thr = 2.0 ** -6
    P, on_plane = boundary_cloud(2)
    hyp = REF.Hypotheses(P)
    iv = ExactIntervals(hyp, thr, on_plane)
    robust, it, bh = REF.replay(iv, len(P), 1000, 0.99)
    assert robust and not hyp.near and hyp.rejected == 0
    seen = [h for h in range(it) if iv.exact(h)]
    assert seen and all(iv[h] == (100, 100) for h in seen)
    lax = REF.replay(ExactIntervals(hyp, thr, on_plane, strict=False), len(P), 1000, 0.99)
    print("iterations %d (best hypothesis %d); counting the 60 boundary points in: %d (best %d)" % (it, bh, lax[1], lax[2]))
    assert lax[0] and lax[1] != it, "the case must tell a lax count from a strict one"
    st, coeff, inl, iters = O.segment_plane(P, CS.params((0, 1000, thr, 0.99)))
    assert st == 0 and iters == it, (iters, it)
    if iv.exact(bh):
        assert np.array_equal(inl, np.flatnonzero(on_plane)) and np.array_equal(np.abs(coeff), np.float32([0, 0, 1, 0.5]))
