"""Canonical rule C20 restated in numpy: the table prism - keep only the object points above the convex hull of the plane inliers
(pcl::ConvexHull of the inliers + pcl::ExtractPolygonalPrismData).

This module is the specification (include/cuboid_hip.h states the rule, DESIGN.md lists it): the device
(perception_amd/csrc/k_prism.hip, cd_table_prism and the fused calls after cd_set_table_prism) and the host arithmetic
(perception_amd/csrc/prism_math.hpp) equal it bit for bit - the kept set, the record and the hull.  numpy only - no GPU, no
library.  Parity with a real PCL is unpinned, as for every other rule: PCL's hull comes from qhull in floating point, its
polygon test is a crossing-number test whose boundary cases are its own.

The rule, for the plane (a, b, c, d) as float32, the plane inliers, the object points and the limits height_min <= height_max:
  1. all arithmetic is double, every product and every sum rounded on its own in the order written.  s = -1 if d < 0 else +1;
     n = s (a, b, c), dd = s d: the sensor at the origin is on the positive side;
  2. h(p) = ((n0 x + n1 y) + n2 z) + dd;
  3. p' = p - h n per component, as x - (h n0);
  4. k0 = argmax(|a|, |b|, |c|), compared as float32, the lowest index on a tie, is dropped; (k1, k2) are the other two ascending;
  5. u = floor(p'[k1] 65536), v = floor(p'[k2] 65536), each clamped to [-2^29, 2^29 - 1] (a NaN to -2^29) and stored as int32;
     everything from here on is integer, cross products of differences fit int64;
  6. the hull: the strict vertices of the convex hull of the inliers' (u, v) - no duplicate, no point on an edge between two
     others - counter-clockwise from the lexicographically smallest.  Fewer than 3 vertices: nothing is kept.  More than
     MAX_HULL: the record says overflow, reports no vertex, and nothing is kept;
  7. a point is kept iff height_min <= h <= height_max and cross(B - A, P - A) >= 0 for every hull edge A -> B; the kept points
     stay in their order;
  8. the record: n_before, n_kept, n_below (h < height_min), n_above (neither below nor h <= height_max: a NaN height counts
     here), n_outside (passed the height test, failed the hull or had none), hull_vertices, axis_u = k1, axis_v = k2, overflow.
A frame of a fused call without a plane passes untouched (have_plane=False): n_kept = n_before, every other field 0.
"""
import numpy as np

MAX_HULL = 1024                 # CD_PRISM_MAX_HULL
LDS_POINTS = 4096               # CD_PRISM_LDS_POINTS: the pruned inliers the kernel keeps in LDS; more are read from global memory
SCALE = 65536.0
QMIN, QMAX = -(1 << 29), (1 << 29) - 1
STAT_FIELDS = ("n_before", "n_kept", "n_below", "n_above", "n_outside", "hull_vertices", "axis_u", "axis_v", "overflow")


def check_limits(height_min, height_max):
    if not (np.isfinite(height_min) and np.isfinite(height_max) and height_min <= height_max):
        raise ValueError("height_min and height_max must be finite with height_min <= height_max")


def _points(a):
    a = np.asarray(a, np.float32)
    return a if a.ndim == 2 else a.reshape(-1, 3)


def orient(coeff):
    """Step 1: (n (3 doubles), dd)."""
    c = np.asarray(coeff, np.float32).reshape(4)
    s = np.float64(-1.0) if c[3] < 0 else np.float64(1.0)
    return s * c[:3].astype(np.float64), s * np.float64(c[3])


def axes(coeff):
    """Step 4: (k1, k2)."""
    c = np.abs(np.asarray(coeff, np.float32).reshape(4)[:3])
    k0 = 0
    if c[1] > c[k0]:
        k0 = 1
    if c[2] > c[k0]:
        k0 = 2
    return tuple(a for a in range(3) if a != k0)


def project(coeff, xyz):
    """Steps 1 - 5 for (n, >= 3) float32 points: (height float64 (n), uv int32 (n, 2), (k1, k2))."""
    p = _points(xyz)[:, :3].astype(np.float64)
    n, dd = orient(coeff)
    k = axes(coeff)
    uv = np.zeros((len(p), 2), np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = ((n[0] * p[:, 0] + n[1] * p[:, 1]) + n[2] * p[:, 2]) + dd
        for j in range(2):
            t = np.floor((p[:, k[j]] - (h * n[k[j]])) * np.float64(SCALE))
            t = np.where(t >= QMIN, np.minimum(t, np.float64(QMAX)), np.float64(QMIN))
            uv[:, j] = t.astype(np.int64).astype(np.int32)
    return h, uv, k


def hull(uv):
    """Step 6 without the cap: the strict hull vertices of integer points (n, 2), counter-clockwise from the lexicographically
    smallest, as an (m, 2) int32 array (Andrew's monotone chain over the distinct points, Python integers)."""
    a = np.asarray(uv, np.int64).reshape(-1, 2)
    pts = [tuple(r) for r in np.unique(a, axis=0).tolist()] if len(a) else []
    if len(pts) > 2:
        def cross(o, p, q):
            return (p[0] - o[0]) * (q[1] - o[1]) - (p[1] - o[1]) * (q[0] - o[0])
        lower, upper = [], []
        for p in pts:
            while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
                lower.pop()
            lower.append(p)
        for p in reversed(pts):
            while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
                upper.pop()
            upper.append(p)
        pts = lower[:-1] + upper[:-1]
    return np.array(pts, np.int32).reshape(-1, 2)


def inside(hull_uv, uv):
    """Step 7's hull test of integer points (n, 2) against at least 3 hull vertices: a bool array; the boundary is inside."""
    H = np.asarray(hull_uv, np.int64).reshape(-1, 2)
    P = np.asarray(uv, np.int64).reshape(-1, 2)
    ok = np.ones(len(P), bool)
    for i in range(len(H)):
        A, B = H[i], H[(i + 1) % len(H)]
        ok &= (B[0] - A[0]) * (P[:, 1] - A[1]) - (B[1] - A[1]) * (P[:, 0] - A[0]) >= 0
    return ok


def extremes(uv):
    """The kernel's first pass: the inliers' extreme points in 8 directions, counter-clockwise from the left, (8, 2) int64; each
    is the maximum of an integer key (direction value, then a tie-breaker), so it does not depend on the order of the points."""
    a = np.asarray(uv, np.int64).reshape(-1, 2)
    u, v = a[:, 0], a[:, 1]
    keys = [(-u, -v), (-u - v, -u), (-v, u), (u - v, u), (u, v), (u + v, u), (v, -u), (v - u, -u)]
    out = np.zeros((8, 2), np.int64)
    for i, (w, t) in enumerate(keys):
        out[i] = a[int(np.argmax(w * (1 << 32) + (t + (1 << 31))))]
    return out


def prune_survivors(uv):
    """The kernel's second pass: the inliers that are not strictly inside the polygon of extremes() (every hull vertex is among
    them), as a bool array.  The hull of the survivors is the hull of all."""
    a = np.asarray(uv, np.int64).reshape(-1, 2)
    if len(a) == 0:
        return np.zeros(0, bool)
    E = extremes(a)
    strict = np.ones(len(a), bool)
    edges = 0
    for i in range(8):
        A, B = E[i], E[(i + 1) % 8]
        if A[0] == B[0] and A[1] == B[1]:
            continue
        edges += 1
        strict &= (B[0] - A[0]) * (a[:, 1] - A[1]) - (B[1] - A[1]) * (a[:, 0] - A[0]) > 0
    return ~strict if edges else np.ones(len(a), bool)


def table_prism(plane_xyz, coeff, xyz, height_min, height_max, have_plane=True):
    """The rule.  plane_xyz (n_plane, >= 3) and xyz (n, >= 3) float32.  Returns dict(indices int32 ascending, stats (a dict of
    STAT_FIELDS), hull (hull_vertices, 2) int32, height float64 (n))."""
    check_limits(height_min, height_max)
    pts = _points(xyz)
    n = len(pts)
    if not have_plane:
        st = dict.fromkeys(STAT_FIELDS, 0)
        st.update(n_before=n, n_kept=n)
        return dict(indices=np.arange(n, dtype=np.int32), stats=st, hull=np.zeros((0, 2), np.int32), height=np.zeros(n, np.float64))
    _, puv, k = project(coeff, plane_xyz)
    H = hull(puv)
    overflow = int(len(H) > MAX_HULL)
    if overflow:
        H = np.zeros((0, 2), np.int32)
    h, uv, _ = project(coeff, pts)
    with np.errstate(invalid="ignore"):
        below = h < np.float64(height_min)
        in_height = ~below & (h <= np.float64(height_max))
    above = ~below & ~in_height
    keep = in_height & inside(H, uv) if len(H) >= 3 else np.zeros(n, bool)
    st = dict(n_before=n, n_kept=int(keep.sum()), n_below=int(below.sum()), n_above=int(above.sum()), n_outside=int((in_height & ~keep).sum()),
              hull_vertices=len(H), axis_u=k[0], axis_v=k[1], overflow=overflow)
    return dict(indices=np.flatnonzero(keep).astype(np.int32), stats=st, hull=H, height=h)


def filter_cloud(plane_xyz, coeff, records, height_min, height_max, have_plane=True):
    """The kept rows of an (n, k >= 3) record array of 4-byte items (x y z first), whole rows in their order, and the rule's dict."""
    r = np.asarray(records)
    xyz = np.ascontiguousarray(r[:, :3]).view(np.float32) if r.dtype != np.float32 else r[:, :3]
    o = table_prism(plane_xyz, coeff, xyz, height_min, height_max, have_plane)
    return r[o["indices"]], o
