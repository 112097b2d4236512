"""Canonical rule C24 restated in numpy: the box fit - a resting cuboid's dimensions, yaw and centre from the table plane and the
points of its cluster, with no template, no search and no iteration.

This module is the specification (include/cuboid_hip.h states the rule, DESIGN.md lists it): the device
(perception_amd/csrc/k_box_fit.hip, cd_box_fit_points and the fused calls after cd_set_box_fit) and the host arithmetic
(perception_amd/csrc/box_fit_math.hpp, cd_box_fit_host) equal it bit for bit, every field of the record.  numpy only - no GPU,
no library.  The rule assumes that the cuboid rests on the plane with a face up; a tilted or stacked box gets a record whose
rectangularity says so, and nothing else.

The rule, for the plane (a, b, c, d) as float32, n float32 points and band (a double, finite, 0 < band <= 64):
  1. all real arithmetic is double, every product and every sum rounded on its own in the order written.  (nrm, dd) is rule C20's
     step 1 (table_prism.orient); h(p) = ((nrm0 x + nrm1 y) + nrm2 z) + dd;
  2. the metric in-plane basis: k0 is rule C20's step 4, k1 = (k0 + 1) mod 3; t_j = [j == k1] - (nrm[k1] nrm_j);
     len = sqrt((t0 t0 + t1 t1) + t2 t2), eu_j = t_j / len; ev = nrm x eu, each component as (nrm_a eu_b) - (nrm_b eu_a);
  3. per point qh = floor(h 65536), u = floor(((eu0 x + eu1 y) + eu2 z) 65536), v likewise with ev, each clamped to
     [-2^29, 2^29 - 1] (a NaN to -2^29) and stored as int32.  From here on everything is integer unless a conversion is written;
  4. the top set: k = 1 + n // 64, href = the k-th largest qh (one stray high point does not set the level);
     top = {qh >= href - floor(band 65536)}; height = ((double) sum_top qh / (double) n_top) / 65536 (the sum an int64);
  5. the hull of the top set's (u, v) is table_prism.hull, capped at table_prism.MAX_HULL vertices;
  6. per hull edge i (A = H[i], B = H[i + 1 mod m], e = B - A), over all hull vertices P: along = (P - A) . e,
     across = e_u (P - A)_v - e_v (P - A)_u (int64); w = max - min of along, g = max - min of across, l2 = e . e;
     area_i = ((double) w (double) g) / (double) l2.  The smallest area wins, a tie goes to the lowest i;
  7. s = sqrt((double) l2), p = ((double) w / s) / 65536, q = ((double) g / s) / 65536; L = max(p, q), W = min(p, q), H = height.
     The long axis in (u, v) is e when p >= q, else (-e_v, e_u); negated when its u component is negative, or zero with a negative
     v component; divided by s;
  8. fa = (double)(amin + amax) / (double)(2 l2), fc = (double)(cmin + cmax) / (double)(2 l2);
     cu = ((double) A_u + fa (double) e_u) + fc (double)(-e_v), cv = ((double) A_v + fa (double) e_v) + fc (double) e_u;
     centre_j = ((cu / 65536) eu_j + (cv / 65536) ev_j) + ((H / 2) - dd) nrm_j;
     ex_j = (ax_u eu_j) + (ax_v ev_j); ey = nrm x ex (as ev); pose is the row-major 4 x 4 box -> camera with the columns ex, ey,
     nrm, centre - the convention of cd_cluster_result.pose and synth.truth_poses;
  9. area = area_min / 65536^2; rectangularity = (((double) shoelace / 2) / 65536^2) / area, shoelace = sum_i (H_i x H_i+1), int64;
     height_ref = (double) href / 65536;
 10. the status is a result, not a failure of the call; the record holds the counts reached so far and zeros elsewhere:
     n < 3: CD_ERR_FEW_CORRESPONDENCES; a non-finite coordinate or |coordinate| > 64: CD_ERR_INVALID_ARG; no plane (have_plane
     false, a non-finite coefficient or a = b = c = 0) or a hull of fewer than 3 vertices: CD_ERR_NO_MODEL; more than MAX_HULL
     vertices: CD_ERR_CAPACITY with overflow = 1 and hull_vertices = 0.
match_slot = -1 and match_cost = 0 unless the selection (cd_set_box_select) filled them: in a fused call with the selection on every
CD_OK record carries match()'s slot and cost over the loaded slots, and in a template_slot = -1 call a cluster with a matched slot is
registered against that slot alone.
"""
import numpy as np

from . import table_prism as TP

BAND_DEFAULT = 0.006            # CD_BOX_FIT_BAND_DEFAULT
BAND_MAX = 64.0
COORD_MAX = 64.0
LDS_POINTS = 2048               # CD_BOX_FIT_LDS_POINTS: the (qh, u, v) of a cluster the kernel keeps in LDS; a larger one is recomputed
MAX_HULL = TP.MAX_HULL
SCALE = 65536.0
CD_OK, CD_ERR_INVALID_ARG, CD_ERR_NO_MODEL, CD_ERR_FEW_CORRESPONDENCES, CD_ERR_CAPACITY = 0, -1, -4, -5, -2
INT_FIELDS = ("n", "n_top", "hull_vertices", "edge", "status", "overflow", "match_slot")
REAL_FIELDS = ("height_ref", "dims", "pose", "area", "rectangularity", "match_cost")


def check_band(band):
    if not (np.isfinite(band) and 0.0 < band <= BAND_MAX):
        raise ValueError("band must be finite, > 0 and <= 64")


def _empty(n, status, **kw):
    r = dict(n=int(n), n_top=0, hull_vertices=0, edge=0, status=int(status), overflow=0, match_slot=-1, height_ref=0.0,
             dims=np.zeros(3, np.float64), pose=np.zeros(16, np.float64), area=0.0, rectangularity=0.0, match_cost=0.0)
    r.update(kw)
    return r


def basis(coeff):
    """Steps 1 and 2: (nrm, dd, eu, ev), doubles."""
    c = np.asarray(coeff, np.float32).reshape(4)
    nrm, dd = TP.orient(c)
    k0 = ({0, 1, 2} - set(TP.axes(c))).pop()
    k1 = (k0 + 1) % 3
    t = np.array([(np.float64(1.0) if j == k1 else np.float64(0.0)) - (nrm[k1] * nrm[j]) for j in range(3)], np.float64)
    ln = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    eu = t / ln
    return nrm, dd, eu, cross(nrm, eu)


def cross(a, b):
    return np.array([(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])], np.float64)


def _quantise(t):
    t = np.floor(t * np.float64(SCALE))
    t = np.where(t >= TP.QMIN, np.minimum(t, np.float64(TP.QMAX)), np.float64(TP.QMIN))
    return t.astype(np.int64).astype(np.int32)


def quantise(coeff, xyz):
    """Step 3 of (n, 3) float32 points: (qh, u, v), int32 arrays."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    nrm, dd, eu, ev = basis(coeff)
    with np.errstate(over="ignore", invalid="ignore"):
        qh = _quantise(((nrm[0] * p[:, 0] + nrm[1] * p[:, 1]) + nrm[2] * p[:, 2]) + dd)
        u = _quantise((eu[0] * p[:, 0] + eu[1] * p[:, 1]) + eu[2] * p[:, 2])
        v = _quantise((ev[0] * p[:, 0] + ev[1] * p[:, 1]) + ev[2] * p[:, 2])
    return qh, u, v


def plane_ok(coeff):
    c = np.asarray(coeff, np.float32).reshape(4)
    return bool(np.all(np.isfinite(c)) and np.any(c[:3] != 0))


def box_fit(coeff, xyz, band=BAND_DEFAULT, have_plane=True):
    """The rule: a dict of INT_FIELDS (Python ints) and REAL_FIELDS (float64; dims (3), pose (16))."""
    check_band(band)
    pts = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(pts)
    if n < 3:
        return _empty(n, CD_ERR_FEW_CORRESPONDENCES)
    with np.errstate(invalid="ignore"):
        if not np.all(np.abs(pts) <= np.float32(COORD_MAX)):     # (a NaN fails the comparison)
            return _empty(n, CD_ERR_INVALID_ARG)
    if not have_plane or not plane_ok(coeff):
        return _empty(n, CD_ERR_NO_MODEL)
    nrm, dd, eu, ev = basis(coeff)
    qh, u, v = quantise(coeff, pts)
    # 4
    k = 1 + n // 64
    href = int(np.sort(qh)[n - k])
    top = qh.astype(np.int64) >= href - int(np.floor(np.float64(band) * np.float64(SCALE)))
    n_top = int(top.sum())
    qsum = int(qh[top].astype(np.int64).sum())
    height = (np.float64(qsum) / np.float64(n_top)) / np.float64(SCALE)
    # 5
    H = TP.hull(np.stack([u[top], v[top]], axis=1)).astype(np.int64)
    m = len(H)
    if m > MAX_HULL:
        return _empty(n, CD_ERR_CAPACITY, n_top=n_top, overflow=1)
    if m < 3:
        return _empty(n, CD_ERR_NO_MODEL, n_top=n_top, hull_vertices=m)
    # 6
    best = None
    for i in range(m):
        A = H[i]
        e = H[(i + 1) % m] - A
        d = H - A
        along = d[:, 0] * e[0] + d[:, 1] * e[1]
        across = e[0] * d[:, 1] - e[1] * d[:, 0]
        w, g, l2 = int(along.max() - along.min()), int(across.max() - across.min()), int(e[0] * e[0] + e[1] * e[1])
        area = (np.float64(w) * np.float64(g)) / np.float64(l2)
        if best is None or area < best[0]:
            best = (area, i, w, g, l2, int(along.min() + along.max()), int(across.min() + across.max()), A, e)
    area, edge, w, g, l2, asum, csum, A, e = best
    # 7
    s = np.sqrt(np.float64(l2))
    p = (np.float64(w) / s) / np.float64(SCALE)
    q = (np.float64(g) / s) / np.float64(SCALE)
    au, av = (int(e[0]), int(e[1])) if p >= q else (-int(e[1]), int(e[0]))
    if au < 0 or (au == 0 and av < 0):
        au, av = -au, -av
    axu, axv = np.float64(au) / s, np.float64(av) / s
    dims = np.array([max(p, q), min(p, q), height], np.float64)
    # 8
    fa = np.float64(asum) / np.float64(2 * l2)
    fc = np.float64(csum) / np.float64(2 * l2)
    cu = (np.float64(A[0]) + fa * np.float64(e[0])) + fc * np.float64(-e[1])
    cv = (np.float64(A[1]) + fa * np.float64(e[1])) + fc * np.float64(e[0])
    cus, cvs = cu / np.float64(SCALE), cv / np.float64(SCALE)
    up = (height / np.float64(2.0)) - dd
    centre = np.array([((cus * eu[j]) + (cvs * ev[j])) + (up * nrm[j]) for j in range(3)], np.float64)
    ex = np.array([(axu * eu[j]) + (axv * ev[j]) for j in range(3)], np.float64)
    ey = cross(nrm, ex)
    pose = np.zeros(16, np.float64)
    for j in range(3):
        pose[4 * j:4 * j + 4] = (ex[j], ey[j], nrm[j], centre[j])
    pose[15] = 1.0
    # 9
    shoelace = 0
    for i in range(m):
        a, b = H[i], H[(i + 1) % m]
        shoelace += int(a[0]) * int(b[1]) - int(a[1]) * int(b[0])
    s2 = np.float64(SCALE) * np.float64(SCALE)
    area_m = area / s2
    return dict(n=n, n_top=n_top, hull_vertices=m, edge=edge, status=CD_OK, overflow=0, match_slot=-1, height_ref=float(np.float64(href) / np.float64(SCALE)),
                dims=dims, pose=pose, area=float(area_m), rectangularity=float(((np.float64(shoelace) / np.float64(2.0)) / s2) / area_m), match_cost=0.0)


def match(dims, slot_dims, loaded_mask, tolerance):
    """cd_box_fit_match: (slot, cost).  slot_dims (n_slots, 3) doubles, each slot's first two sorted descending here; cost =
    max(|L - Ls|, |W - Ws|, |H - Hs|) in double; the lowest cost wins, a tie goes to the lowest slot; slot = -1 (with the best cost)
    when no slot is loaded (cost 0 then) or the best cost exceeds the tolerance."""
    d = np.asarray(dims, np.float64).reshape(3)
    sd = np.asarray(slot_dims, np.float64).reshape(-1, 3)
    best, cost = -1, np.float64(0.0)
    for s in range(len(sd)):
        if not (int(loaded_mask) >> s) & 1:
            continue
        ls, ws = max(sd[s, 0], sd[s, 1]), min(sd[s, 0], sd[s, 1])
        c = max(abs(d[0] - ls), abs(d[1] - ws), abs(d[2] - sd[s, 2]))
        if best < 0 or c < cost:
            best, cost = s, c
    if best >= 0 and cost > np.float64(tolerance):
        best = -1
    return best, float(cost)


def record_bits(r):
    """A record as comparable bits: the integer fields and the bit patterns of every double."""
    reals = np.concatenate([np.atleast_1d(np.asarray(r[k], np.float64)).ravel() for k in REAL_FIELDS])
    return tuple(int(r[k]) for k in INT_FIELDS) + tuple(int(b) for b in reals.view(np.uint64))
