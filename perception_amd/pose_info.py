"""Canonical rule C23 restated in numpy: the pose information of a (cluster, lattice template) pair - which of the six directions of
a small rigid motion the cluster's correspondences pin down, by how many points' worth, and the covariance of the pose over those.

This module is the specification (include/cuboid_hip.h states the rule, DESIGN.md lists it): the device
(perception_amd/csrc/k_pose_info.hip, cd_pose_info_points and the fused calls after cd_set_pose_info) and the host arithmetic
(perception_amd/csrc/pose_info_math.hpp, cd_pose_info_host) equal it bit for bit in every field of the record.  numpy and Python
floats only - no GPU, no library.

The information counts what the template's SURFACES constrain and nothing else: a point constrains the motion along the normal of
the face its nearest template point lies on.  The outline of a partial view adds nothing (a cluster that ends where the sensor
stopped seeing a face does not pin the pose along that face), and hidden faces are not reasoned about.

The rule, for the cluster's n float32 points src as extracted, T (row-major 4x4 float32, the result's), the m points tpl of a
lattice template (perception_amd/icp_plane.py face_axes: consecutive faces, each two ascending axis tables at a constant third
coordinate), a range d and a support min_support (doubles, finite, > 0).  Everything is in the template's frame:
  1. A_i = T src_i in float32: rule C21's step 1 (pair_score.aligned);
  2. q_i, d2_i = rule C5's neighbour of A_i (the lowest index at the least canonical float32 squared distance) and w_i = the constant
     axis of q_i's face; i is kept iff d2_i <= tau(d), rule C8's threshold, the boundary inside.  n_in = the kept, n_face[a] = the
     kept with w = a;
  3. c0 = the centre of the template's bounding box, float32 (min + max) * 0.5f per axis; L = half its diagonal in double from the
     float32 extents e = (double) max - (double) min: 0.5 * sqrt((ex ex + ey ey) + ez ez), 1.0 when that is not > 0.
     p_i = A_i - c0, one float32 subtraction per axis;
  4. per kept point, a = w_i, b = (a + 1) % 3, c = (a + 2) % 3, r = q_a - A_a: the float32 terms p_c, p_b, p_c p_c, p_b p_b, p_c p_b
     and r r, one rounded operation each, summed per axis a as rule-C4 integers rint(v 2^32) (r r: 2^36), int64, order-free.
     (The three further terms of rule C17's lambda = 0 step, r p_c, r p_b and r, are the step's right-hand side: no field of the
     record reads them, and they are not formed.)
  5. a sum's double is ldexp((double)(int64), -shift).  H (6 x 6, symmetric, unknowns (L omega, t) of A' = A + omega x (A - c0) + t;
     the row of a point is ((p x e_w) / L, e_w)) starts from +0.0 and receives the axes in the order 0, 1, 2:
        H[b][b] += (S(p_c p_c) / L) / L      H[c][c] += (S(p_b p_b) / L) / L      H[b][c] = H[c][b] += -((S(p_c p_b) / L) / L)
        H[3+a][b] += S(p_c) / L              H[3+a][c] += -(S(p_b) / L)           H[3+a][3+a] += (double) n_face[a]
  6. cyclic Jacobi in double: SWEEPS sweeps over the pairs (0,1) (0,2) .. (0,5) (1,2) .. (4,5); a pair whose entry is exactly 0
     is left alone; otherwise theta = (a_qq - a_pp) / (2 a_pq), root = sqrt(theta theta + 1), t = 1 / (theta + root) for
     theta >= 0 and -1 / (root - theta) otherwise, cs = 1 / sqrt(t t + 1), sn = t cs, h = t a_pq; a_pp -= h, a_qq += h, a_pq = 0,
     a_rp = cs a_rp - sn a_rq and a_rq = sn a_rp + cs a_rq for the other r (both from the old values), and the same two lines for
     every row of V (which starts as the identity).  Eigenvalues = the diagonal, ascending, equal ones in index order, vector k =
     the matching column of V, negated when its component of largest magnitude (the first of equals) is negative;
  7. n_constrained = #{k: lambda_k >= min_support}; sigma2 = ldexp((double)(S_rr of the three axes, int64), -36) / n_in;
     C[i][j] = sigma2 * (sum over the constrained k, ascending, from +0.0, of (v_k[i] v_k[j]) / lambda_k);
     covariance[i][j] = (D_i C[i][j]) D_j with D = (1/L, 1/L, 1/L, 1, 1, 1): the covariance of (omega, t), a rotation about c0.
     Directions that are not constrained are ABSENT from it (not infinite): n_constrained says so.  weakest = v_0;
  8. well_posed = accepted and n_constrained == 6;
  9. status, the first that applies: CD_ERR_NO_TEMPLATE (m = 0), CD_ERR_INVALID_ARG (tpl is not a lattice; a non-finite entry of T
     or coordinate of A - such a record holds n_source, the status and zeros), CD_ERR_FEW_CORRESPONDENCES (n_in < 3),
     CD_ERR_CAPACITY (n > 2^19) - these two hold n_source, n_in, n_face, the status and zeros.
The integer sums stay inside int64 for every template whose half diagonal plus the range is at most 64 m (2^19 terms below 2^12
at 2^32); beyond that they wrap, here as on the
device - as long as every single term stays below 2^63 (|p| below 46340 m at 2^32), which is as far as the rule is defined: a larger
term saturates in the device's conversion and is not an integer here.
"""
import math

import numpy as np

from . import icp_plane as IP
from . import pair_score as PS

CD_OK, CD_ERR_INVALID_ARG, CD_ERR_CAPACITY, CD_ERR_FEW_CORRESPONDENCES, CD_ERR_NO_TEMPLATE = 0, -1, -2, -5, -7
SWEEPS = 5
MAX_POINTS = 1 << 19
MIN_CORR = 3
NSUMS = 18                     # per axis: p_c, p_b, p_c p_c, p_b p_b, p_c p_b (2^32), r r (2^36)
RANGE_DEFAULT = 0.005
MIN_SUPPORT_DEFAULT = 8.0

f32, f64 = np.float32, np.float64
INT_FIELDS = ("n_source", "n_in", "n_face", "n_constrained", "well_posed", "status")
FLOAT_FIELDS = ("eigenvalues", "eigenvectors", "weakest", "sigma2", "covariance", "centre", "length")
FIELDS = INT_FIELDS + FLOAT_FIELDS
PAIRS = tuple((p, q) for p in range(5) for q in range(p + 1, 6))


def check_setting(max_range, min_support):
    """What cd_set_pose_info accepts."""
    return bool(np.isfinite(max_range) and max_range > 0.0 and np.isfinite(min_support) and min_support > 0.0)


def box_of(tpl):
    """Step 3: (c0 float32[3], L float)."""
    t = np.asarray(tpl, f32).reshape(-1, 3)
    lo, hi = t.min(axis=0), t.max(axis=0)
    c0 = ((lo + hi) * f32(0.5)).astype(f32)
    e = [float(f64(hi[a]) - f64(lo[a])) for a in range(3)]
    L = 0.5 * math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return c0, (L if L > 0.0 else 1.0)


def _wrap(v):
    """A Python integer as the int64 the device's 64-bit sum holds."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def sums_of(A, q_w, w, c0):
    """Step 4 over the kept points: (18 Python ints, n_face).  A: (k, 3) float32, q_w: the neighbours' coordinate on their face's
    constant axis, w: that axis."""
    S, nf = [0] * NSUMS, [0, 0, 0]
    p = (A - c0[None, :]).astype(f32)
    for a in range(3):
        sel = w == a
        nf[a] = int(sel.sum())
        if not nf[a]:
            continue
        b, c = (a + 1) % 3, (a + 2) % 3
        pc, pb = p[sel, c], p[sel, b]
        r = (q_w[sel] - A[sel, a]).astype(f32)
        with np.errstate(over="ignore"):
            terms = (pc, pb, pc * pc, pb * pb, pc * pb, r * r)
        for j, t in enumerate(terms):
            assert t.dtype == f32
            S[6 * a + j] = _wrap(sum(int(x) for x in np.rint(np.ldexp(t.astype(f64), 36 if j == 5 else 32))))
    return S, nf


def info_matrix(S, nf, L):
    """Step 5: H as six lists of Python floats."""
    H = [[0.0] * 6 for _ in range(6)]
    s = [float(np.ldexp(f64(v), -32)) for v in S]

    def add(i, j, v):
        H[i][j] = H[i][j] + v
        if i != j:
            H[j][i] = H[i][j]

    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        add(b, b, (s[6 * a + 2] / L) / L)
        add(c, c, (s[6 * a + 3] / L) / L)
        add(b, c, -((s[6 * a + 4] / L) / L))
        add(3 + a, b, s[6 * a + 0] / L)
        add(3 + a, c, -(s[6 * a + 1] / L))
        add(3 + a, 3 + a, float(nf[a]))
    return H


def jacobi(H, sweeps=SWEEPS):
    """Step 6 before the ordering: (the diagonal, V as rows of columns, the largest off-diagonal magnitude left)."""
    a = [row[:] for row in H]
    v = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            root = math.sqrt(theta * theta + 1.0)
            t = 1.0 / (theta + root) if theta >= 0.0 else -1.0 / (root - theta)
            cs = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * cs
            h = t * apq
            a[p][p] = a[p][p] - h
            a[q][q] = a[q][q] + h
            a[p][q] = a[q][p] = 0.0
            for r in range(6):
                if r == p or r == q:
                    continue
                arp, arq = a[r][p], a[r][q]
                a[r][p] = a[p][r] = cs * arp - sn * arq
                a[r][q] = a[q][r] = sn * arp + cs * arq
            for k in range(6):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p] = cs * vkp - sn * vkq
                v[k][q] = sn * vkp + cs * vkq
    off = max(abs(a[i][j]) for i in range(6) for j in range(6) if i != j)
    return [a[k][k] for k in range(6)], v, off


def eigen(H, sweeps=SWEEPS):
    """Step 6: (eigenvalues ascending, eigenvectors as rows)."""
    d, v, _ = jacobi(H, sweeps)
    order = sorted(range(6), key=lambda k: d[k])          # (stable: equal values keep their index order)
    lam = [d[k] for k in order]
    vec = []
    for k in order:
        col = [v[i][k] for i in range(6)]
        big = max(range(6), key=lambda i: (abs(col[i]), -i))
        vec.append([-x for x in col] if col[big] < 0.0 else col)
    return lam, vec


def _record(n, status, n_in=0, nf=(0, 0, 0)):
    return dict(n_source=int(n), n_in=int(n_in), n_face=[int(x) for x in nf], n_constrained=0, well_posed=0, status=int(status),
                eigenvalues=[0.0] * 6, eigenvectors=[0.0] * 36, weakest=[0.0] * 6, sigma2=0.0, covariance=[0.0] * 36, centre=[0.0] * 3, length=0.0)


def pose_info(src, T, tpl, max_range=RANGE_DEFAULT, min_support=MIN_SUPPORT_DEFAULT, accepted=1, want_matrix=False):
    """The rule.  Returns the record as a dict of FIELDS (with want_matrix also "H", when the status is CD_OK)."""
    if not check_setting(max_range, min_support):
        raise ValueError("max_range and min_support must be finite and > 0")
    src = np.ascontiguousarray(np.asarray(src, f32).reshape(-1, 3))
    tpl = np.ascontiguousarray(np.asarray(tpl, f32).reshape(-1, 3))
    T = np.asarray(T, f32).reshape(4, 4)
    n, m = len(src), len(tpl)
    if m == 0:
        return _record(n, CD_ERR_NO_TEMPLATE)
    try:
        face_w = IP.face_axes(tpl)
    except ValueError:
        return _record(n, CD_ERR_INVALID_ARG)
    if not np.isfinite(T).all():
        return _record(n, CD_ERR_INVALID_ARG)
    A = PS.aligned(T, src)
    if not np.isfinite(A).all():
        return _record(n, CD_ERR_INVALID_ARG)
    c0, L = box_of(tpl)
    idx, d2 = IP.nearest(tpl, A)
    keep = d2 <= PS.tau_of(max_range)
    w = face_w[idx[keep]]
    S, nf = sums_of(A[keep], tpl[idx[keep], w], w, c0)
    n_in = int(keep.sum())
    if n_in < MIN_CORR:
        return _record(n, CD_ERR_FEW_CORRESPONDENCES, n_in, nf)
    if n > MAX_POINTS:
        return _record(n, CD_ERR_CAPACITY, n_in, nf)
    H = info_matrix(S, nf, L)
    lam, vec = eigen(H)
    rec = _record(n, CD_OK, n_in, nf)
    constrained = [k for k in range(6) if lam[k] >= float(min_support)]
    rec["n_constrained"] = len(constrained)
    rec["well_posed"] = int(bool(accepted) and len(constrained) == 6)
    rec["eigenvalues"] = lam
    rec["eigenvectors"] = [x for row in vec for x in row]
    rec["weakest"] = vec[0][:]
    sigma2 = float(np.ldexp(f64(_wrap(S[5] + S[11] + S[17])), -36)) / float(n_in)
    rec["sigma2"] = sigma2
    D = [1.0 / L] * 3 + [1.0] * 3
    cov = []
    for i in range(6):
        for j in range(6):
            acc = 0.0
            for k in constrained:
                acc = acc + (vec[k][i] * vec[k][j]) / lam[k]
            cov.append((D[i] * (sigma2 * acc)) * D[j])
    rec["covariance"] = cov
    rec["centre"] = [float(x) for x in c0]
    rec["length"] = L
    if want_matrix:
        rec["H"] = H
    return rec


def ros_covariance(rec, T):
    """cd_pose_info_ros_covariance in float64 numpy: the covariance of the published pose P = T^-1 (the template in the camera frame)
    in geometry_msgs/PoseWithCovariance order - position, then rotation about the fixed axes of the parent frame - as J S J^T with
    S the record's covariance over (omega, t), R_P the rotation of P (the transpose of T's) and
    J = [[-R_P [c0]x, -R_P], [-R_P, 0]].  Unconstrained directions are absent from S, and so from the result."""
    R = np.asarray(T, np.float64).reshape(4, 4)[:3, :3].T
    c = rec["centre"]
    cx = np.array([[0.0, -c[2], c[1]], [c[2], 0.0, -c[0]], [-c[1], c[0], 0.0]])
    J = np.zeros((6, 6))
    J[:3, :3], J[:3, 3:], J[3:, :3] = -R @ cx, -R, -R
    return J @ np.asarray(rec["covariance"], np.float64).reshape(6, 6) @ J.T
