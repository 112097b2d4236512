"""Canonical rule C21 restated in numpy: the two-way registration score of a (cluster, template) pair.

This module is the specification (include/cuboid_hip.h states the rule, DESIGN.md lists it): the device
(perception_amd/csrc/k_pair_score.hip, cd_pair_score_points and the fused calls after cd_set_pair_score) and the host arithmetic
(perception_amd/csrc/pair_score_math.hpp, cd_pair_score_host) equal it bit for bit in every field of the record.  numpy only - no
GPU, no library.  Parity with a real PCL is unpinned, as for every other rule: pcl::registration::TransformationValidationEuclidean
has thresholds of its own, float sums and a k-d tree; getFitnessScore(max_range) is the forward half only.

The rule, for the cluster's n float32 xyz points src as extracted, T (row-major 4x4 float32, the result's), the m points tpl of the
result's template and max_range d (a double, finite, > 0):
  1. A_i = T src_i, evaluated once in float32, every product and sum rounded on its own:
     ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3] for r = 0, 1, 2 - the order of cd_get_cluster_points(aligned != 0) when the
     pass that produced the kept result is no longer resident.  The ICP's iterated cloud is not used;
  2. d2(p, q) = (dx dx + dy dy) + dz dz in float32, dx = p.x - q.x ...; f_i = min_j d2(A_i, tpl_j), r_j = min_i d2(tpl_j, A_i).
     A minimum over float32 values is order-free and no index is reported, so ties do not matter;
  3. tau = the largest float32 with (double) tau <= d * d (rule C8's threshold); a distance equal to tau is inside;
  4. n_source_in = #{i: f_i <= tau}, n_template_in = #{j: r_j <= tau};
  5. three order-free 64-bit integer sums of fixq(min(v, 256), 36) = rint(min(v, 256) 2^36) (rule C4): of f over the inside source
     points, of r over the inside template points, of r over all m template points.  Inside rule C4's range (|coordinate| <= 64,
     n, m <= 2^19) a d2 reaches 3 * 128^2 = 49152, whose fixq would be 2^51.6: 2^19 of them would overflow.  So a term is clamped to
     256 m^2 (a nearest neighbour 16 m away - far beyond any range a registration is judged at): a term is at most 2^44 and 2^19
     terms sum to at most 2^63, inside an unsigned 64-bit integer.  More than 2^19 points on either side are refused.
     forward_fitness_in = ((double) S 2^-36) / n_source_in, 0.0 for a count of 0; reverse_fitness_in likewise;
     reverse_fitness = ((double) S_all 2^-36) / m;
  6. coverage = (double) n_template_in / (double) m, inlier_fraction = (double) n_source_in / (double) n;
  7. valid = accepted and coverage >= min_coverage and inlier_fraction >= min_inlier_fraction (double compares, the boundary valid);
  8. status, the first that applies: CD_ERR_NO_TEMPLATE (m = 0), CD_ERR_FEW_CORRESPONDENCES (n < 3), CD_ERR_CAPACITY (n or m above
     2^19), CD_ERR_INVALID_ARG (a non-finite entry of T, or a non-finite coordinate of tpl or of A).  Such a record holds n_source,
     n_template, the status and zeros; valid = 0.
"""
import numpy as np

CD_OK, CD_ERR_INVALID_ARG, CD_ERR_CAPACITY, CD_ERR_FEW_CORRESPONDENCES, CD_ERR_NO_TEMPLATE = 0, -1, -2, -5, -7
TERM_MAX = np.float32(256.0)
SHIFT = 36
MAX_POINTS = 1 << 19
_ROWS = 512      # queries per block of the distance matrix

FIELDS = ("n_source", "n_source_in", "n_template", "n_template_in", "valid", "status", "forward_fitness_in", "reverse_fitness_in",
          "reverse_fitness", "coverage", "inlier_fraction")


def check_thresholds(max_range, min_coverage, min_inlier_fraction):
    """What cd_set_pair_score accepts."""
    return bool(np.isfinite(max_range) and max_range > 0.0 and 0.0 <= min_coverage <= 1.0 and 0.0 <= min_inlier_fraction <= 1.0)


def tau_of(max_range):
    """Step 3."""
    dd = np.float64(max_range) * np.float64(max_range)
    with np.errstate(over="ignore"):
        f = np.float32(dd)
    if np.float64(f) > dd:
        f = np.nextafter(f, np.float32(0.0))
    return np.float32(f)


def aligned(T, src):
    """Step 1: (n, 3) float32."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    p = np.ascontiguousarray(np.asarray(src, np.float32).reshape(-1, 3))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        cols = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)]
    out = np.stack(cols, axis=1)
    assert out.dtype == np.float32
    return out


def nearest_d2(queries, targets):
    """Step 2 for one direction: the float32 minimum over all targets of every query's squared distance."""
    q = np.ascontiguousarray(queries, np.float32)
    t = np.ascontiguousarray(targets, np.float32)
    out = np.empty(len(q), np.float32)
    tx, ty, tz = (np.ascontiguousarray(t[:, a]) for a in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        for r0 in range(0, len(q), _ROWS):
            r1 = min(r0 + _ROWS, len(q))
            dx = q[r0:r1, 0, None] - tx[None, :]
            dy = q[r0:r1, 1, None] - ty[None, :]
            dz = q[r0:r1, 2, None] - tz[None, :]
            d2 = (dx * dx + dy * dy) + dz * dz                      # float32 arrays: one rounding per operation
            assert d2.dtype == np.float32
            out[r0:r1] = d2.min(axis=1)
    return out


def fix_sum(values):
    """Step 5: the exact integer sum of rint(min(v, 256) 2^36) (ties to even) as a Python int."""
    v = np.minimum(np.asarray(values, np.float32), TERM_MAX).astype(np.float64)
    return sum(int(t) for t in np.rint(np.ldexp(v, SHIFT)))


def _record(n, m, status):
    return dict(n_source=int(n), n_source_in=0, n_template=int(m), n_template_in=0, valid=0, status=int(status), forward_fitness_in=0.0,
                reverse_fitness_in=0.0, reverse_fitness=0.0, coverage=0.0, inlier_fraction=0.0)


def pair_score(src, T, tpl, max_range, min_coverage=0.0, min_inlier_fraction=0.0, accepted=1, want_distances=False):
    """The rule.  Returns the record as a dict of FIELDS (with want_distances also f and r, float32, when the status is CD_OK)."""
    if not check_thresholds(max_range, min_coverage, min_inlier_fraction):
        raise ValueError("max_range must be finite and > 0, the fractions in [0, 1]")
    src = np.ascontiguousarray(np.asarray(src, np.float32).reshape(-1, 3))
    tpl = np.ascontiguousarray(np.asarray(tpl, np.float32).reshape(-1, 3))
    T = np.asarray(T, np.float32).reshape(4, 4)
    n, m = len(src), len(tpl)
    if m == 0:
        return _record(n, m, CD_ERR_NO_TEMPLATE)
    if n < 3:
        return _record(n, m, CD_ERR_FEW_CORRESPONDENCES)
    if n > MAX_POINTS or m > MAX_POINTS:
        return _record(n, m, CD_ERR_CAPACITY)
    if not np.isfinite(T).all():
        return _record(n, m, CD_ERR_INVALID_ARG)
    A = aligned(T, src)
    if not (np.isfinite(A).all() and np.isfinite(tpl).all()):
        return _record(n, m, CD_ERR_INVALID_ARG)
    tau = tau_of(max_range)
    f = nearest_d2(A, tpl)
    r = nearest_d2(tpl, A)
    fin, rin = f <= tau, r <= tau
    rec = _record(n, m, CD_OK)
    rec["n_source_in"], rec["n_template_in"] = int(fin.sum()), int(rin.sum())
    q = np.ldexp(np.float64(1.0), -SHIFT)
    if rec["n_source_in"]:
        rec["forward_fitness_in"] = float((np.float64(fix_sum(f[fin])) * q) / np.float64(rec["n_source_in"]))
    if rec["n_template_in"]:
        rec["reverse_fitness_in"] = float((np.float64(fix_sum(r[rin])) * q) / np.float64(rec["n_template_in"]))
    rec["reverse_fitness"] = float((np.float64(fix_sum(r)) * q) / np.float64(m))
    rec["coverage"] = float(np.float64(rec["n_template_in"]) / np.float64(m))
    rec["inlier_fraction"] = float(np.float64(rec["n_source_in"]) / np.float64(n))
    rec["valid"] = int(bool(accepted) and rec["coverage"] >= float(min_coverage) and rec["inlier_fraction"] >= float(min_inlier_fraction))
    if want_distances:
        rec["f"], rec["r"] = f, r
    return rec
