"""Inputs for the box-fit tests (rule C24), CPU only: the known-answer lattices, the oracle's clusters of the synth frames with the
truth each belongs to, and the record comparisons the CPU and GPU tests share."""
import functools

import numpy as np

from perception_amd import box_fit as BF, capi, synth

STEP = 2.0 ** -10   # the lattice unit of the known answers: every coordinate is a multiple of it, every floor exact


def lattice_box(na, nb, step_a, step_b, height, origin=(0.0, 0.0), normal_axis=2, d_sign=1, plane_offset=0.5, side_rows=2):
    """A box's top face as an integer lattice and a few points down one side, on the plane `axis = const`.

    The in-plane coordinates are (origin + i step_a + j step_b) STEP for 0 <= i <= na, 0 <= j <= nb (step_* integer pairs,
    perpendicular), along the rule's (eu, ev) of that plane; the top is `height` above the plane, `side_rows` rows hang below it
    outside the band.  Returns (coeff float32 (4), xyz float32 (n, 3), dict of what the rule must find)."""
    k0 = normal_axis
    k1, k2 = (k0 + 1) % 3, (k0 + 2) % 3
    # the plane: coordinate k0 = plane_offset seen from the origin side, so n = -e_k0 and dd = plane_offset (or both negated in the
    # coefficients: d < 0 is oriented back by step 1)
    coeff = np.zeros(4, np.float32)
    coeff[k0] = -1.0 * d_sign
    coeff[3] = plane_offset * d_sign
    nrm = np.zeros(3)
    nrm[k0] = -1.0
    eu = np.zeros(3)
    eu[k1] = 1.0
    ev = np.cross(nrm, eu)
    i, j = np.meshgrid(np.arange(na + 1), np.arange(nb + 1), indexing="ij")
    U = (origin[0] + i.ravel() * step_a[0] + j.ravel() * step_b[0]) * STEP
    V = (origin[1] + i.ravel() * step_a[1] + j.ravel() * step_b[1]) * STEP
    Hh = np.full(U.shape, float(height))
    # the side below the edge j = 0
    si = np.arange(na + 1)
    for r in range(1, side_rows + 1):
        U = np.concatenate([U, (origin[0] + si * step_a[0]) * STEP])
        V = np.concatenate([V, (origin[1] + si * step_a[1]) * STEP])
        Hh = np.concatenate([Hh, np.full(si.shape, height - r * 0.0078125)])
    xyz = U[:, None] * eu + V[:, None] * ev + (Hh - plane_offset)[:, None] * nrm
    la, lb = np.hypot(*step_a) * na * STEP, np.hypot(*step_b) * nb * STEP
    cu = (origin[0] + 0.5 * (na * step_a[0] + nb * step_b[0])) * STEP
    cv = (origin[1] + 0.5 * (na * step_a[1] + nb * step_b[1])) * STEP
    centre = cu * eu + cv * ev + (height / 2 - plane_offset) * nrm
    return coeff, xyz.astype(np.float32), dict(L=max(la, lb), W=min(la, lb), H=float(height), centre=centre, n_top=(na + 1) * (nb + 1), nrm=nrm, eu=eu, ev=ev)


def default_prm():
    return capi.default_params()


def config5_prm():
    prm = capi.default_params()
    prm.rgb_offset = 12
    prm.crop_x_min, prm.crop_x_max = -synth.CONFIG5_CROP_X, synth.CONFIG5_CROP_X
    prm.crop_z_max = prm.crop2_z_max = 1.2
    return prm


def _clusters_of(frame, prm, template):
    from oracle import oracle_py as O
    o = O.process_frame(frame, prm, template, want_clouds=True)
    r = o["result"]
    obj, labels = o["objects"], o["labels"]
    return np.array(list(r.plane), np.float32), [np.ascontiguousarray(obj[labels == k]) for k in range(r.n_clusters)]


def _with_truth(plane, clusters, scene):
    """Every cluster with the truth box whose centre is nearest its centroid: (plane, points, truth pose 4 x 4, dims, box index)."""
    poses = synth.truth_poses(scene)
    out = []
    for pts in clusters:
        c = pts.astype(np.float64).mean(0)
        b = int(np.argmin([np.linalg.norm(T[:3, 3] - c) for T in poses]))
        out.append((plane, pts, poses[b], 2.0 * scene["boxes"][b]["half"], b))
    return out


@functools.lru_cache(maxsize=None)
def synth_clusters(first, count):
    """The oracle's clusters of synth.frame(first .. first + count) at default parameters, each with its truth."""
    from perception_amd import templates
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    prm = default_prm()
    prm.icp_max_iterations = 1
    out = []
    for i in range(first, first + count):
        plane, cl = _clusters_of(synth.frame(i), prm, tpl)
        out += _with_truth(plane, cl, synth.scene_for(i))
    return out


@functools.lru_cache(maxsize=None)
def config5_clusters(first, count, width=640, height=480):
    from perception_amd import templates
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    prm = config5_prm()
    prm.icp_max_iterations = 1
    out = []
    for i in range(first, first + count):
        sc = synth.scene_config5(i)
        plane, cl = _clusters_of(synth.render(sc, width=width, height=height), prm, tpl)
        out += _with_truth(plane, cl, sc)
    return out


def errors(rec, truth_pose, truth_dims):
    """(dL, dW, dH, centre distance, yaw error in degrees) of an OK record against the truth."""
    L, W = max(truth_dims[0], truth_dims[1]), min(truth_dims[0], truth_dims[1])
    P = np.asarray(rec["pose"], np.float64).reshape(4, 4)
    tx = truth_pose[:3, 0] if truth_dims[0] >= truth_dims[1] else truth_pose[:3, 1]
    cosv = abs(float(np.dot(P[:3, 0], tx)))       # (an axis, not a direction: the box is symmetric under a half turn)
    yaw = np.degrees(np.arccos(min(1.0, cosv)))
    return rec["dims"][0] - L, rec["dims"][1] - W, rec["dims"][2] - truth_dims[2], float(np.linalg.norm(P[:3, 3] - truth_pose[:3, 3])), yaw


def random_cloud(seed, n):
    """A seeded box-like cloud on a tilted plane: (coeff, xyz)."""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=3)
    nrm /= np.linalg.norm(nrm)
    d = rng.uniform(0.3, 0.8) * (1 if seed % 2 else -1)
    coeff = np.r_[nrm, d].astype(np.float32)
    a = np.cross(nrm, [0.3, 0.5, 0.8])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    yaw = rng.uniform(0, np.pi)
    ex, ey = np.cos(yaw) * a + np.sin(yaw) * b, -np.sin(yaw) * a + np.cos(yaw) * b
    top = int(n * 0.7)
    s = rng.uniform(-1, 1, (n, 2)) * [0.1, 0.04]
    h = np.where(np.arange(n) < top, 0.05 + rng.normal(0, 0.0007, n), rng.uniform(0, 0.05, n))
    s[top:, 1] = -0.04
    base = -d * nrm / np.dot(nrm, nrm)
    xyz = base + s[:, :1] * ex + s[:, 1:] * ey + h[:, None] * nrm * np.sign(d if d else 1)
    return coeff, xyz.astype(np.float32)


def same_record(got, want):
    """Every field of two records (dicts of box_fit's fields) bit for bit; returns the names that differ."""
    bad = [k for k in BF.INT_FIELDS if int(got[k]) != int(want[k])]
    for k in BF.REAL_FIELDS:
        a = np.atleast_1d(np.asarray(got[k], np.float64)).view(np.uint64)
        b = np.atleast_1d(np.asarray(want[k], np.float64)).view(np.uint64)
        if not np.array_equal(a, b):
            bad.append(k)
    return bad


# ---- integer clouds on the plane z = 0 seen from above: u = floor(x 65536), v = floor(y 65536), qh = floor(z 65536) -------------------
COEFF_Z = np.array([0.0, 0.0, 1.0, 0.0], np.float32)


def uv_cloud(uv, qh):
    """(n, 3) float32 points that quantise to the integer (u, v) and height qh (a scalar or (n,)) under COEFF_Z."""
    a = np.asarray(uv, np.int64).reshape(-1, 2)
    q = np.broadcast_to(np.asarray(qh, np.int64), (len(a),))
    p = ((np.c_[a, q].astype(np.float64) + 0.5) / 65536.0).astype(np.float32)
    assert np.array_equal(np.floor(p.astype(np.float64) * 65536.0).astype(np.int64), np.c_[a, q]), "not exact in float32"
    return p


def _filled(n, seed, span=3000, qh=4000, low=0):
    """n points: n - low on an integer rectangle's top at qh +- 20, `low` far below the band."""
    rng = np.random.RandomState(seed)
    uv = np.c_[rng.randint(-span, span, n), rng.randint(-span // 2, span // 2, n)]
    q = qh + rng.randint(-20, 21, n)
    q[:low] = qh - 2000 - rng.randint(0, 500, low)
    return uv_cloud(uv, q)


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """name -> (coeff, xyz, band): the sizes and shapes at which k_box_fit takes another path.  Read only."""
    band = BF.BAND_DEFAULT
    bq = int(np.floor(band * 65536.0))
    out = {}
    for n in (3, 63, 64, 65):                                   # k = 1 + n // 64 switches at 64
        out["n_%d" % n] = (COEFF_Z, _filled(n, n, low=0 if n == 3 else n // 3), band)
    # one stray high point: with n = 64 (k = 2) it does not set the level, with n = 63 (k = 1) it does
    for n in (63, 64):
        p = _filled(n, 100 + n).copy()
        p[5, 2] = np.float32((9000 + 0.5) / 65536.0)
        out["stray_%d" % n] = (COEFF_Z, p, band)
    out["lds_cap"] = (COEFF_Z, _filled(BF.LDS_POINTS, 7, low=500), band)
    out["lds_cap_plus_1"] = (COEFF_Z, _filled(BF.LDS_POINTS + 1, 8, low=500), band)
    out["large"] = (COEFF_Z, _filled(3 * BF.LDS_POINTS + 77, 9, low=1500), band)
    out["top_of_3"] = (COEFF_Z, uv_cloud([(0, 0), (900, 50), (300, 700)] + [(10 * i, 7 * i) for i in range(30)], [5000] * 3 + [100] * 30), band)
    out["top_collinear"] = (COEFF_Z, uv_cloud([(3 * i, 5 * i) for i in range(40)] + [(50, 3)] * 8, [5000] * 40 + [100] * 8), band)
    out["top_one_point"] = (COEFF_Z, uv_cloud([(7, 7)] * 20 + [(1, 2), (3, 4)], [5000] * 20 + [0, 0]), band)
    out["hull_4"] = (COEFF_Z, uv_cloud([(0, 0), (1000, 0), (1000, 500), (0, 500), (500, 250), (0, 250), (500, 0)], 3000), band)
    out["duplicates"] = (COEFF_Z, uv_cloud([(0, 0), (1200, 300), (900, 1500), (-300, 1200)] * 40 + [(400, 700)] * 9, 3000), band)
    t = 2.0 * np.pi * np.arange(5000) / 5000
    circle = np.floor(np.stack([np.cos(t), np.sin(t)], 1) * 0.08 * 65536.0).astype(np.int64)
    out["circle"] = (COEFF_Z, uv_cloud(circle, 2000), band)      # 656 strict vertices: more edges than threads
    i = np.arange(MAX_HULL_PLUS, dtype=np.int64)
    para = np.stack([i, i * i], 1)
    out["parabola_max_hull"] = (COEFF_Z, uv_cloud(para[:BF.MAX_HULL], 2000), band)
    out["parabola_overflow"] = (COEFF_Z, uv_cloud(para, 2000), band)
    # a qh exactly on href - band (in the top set) and one unit below it (not)
    sq = [(0, 0), (800, 0), (800, 400), (0, 400)]
    out["on_the_band"] = (COEFF_Z, uv_cloud(sq + [(2000, 2000), (3000, -50)], [5000] * 4 + [5000 - bq, 5000 - bq - 1]), band)
    out["wide_band"] = (COEFF_Z, _filled(300, 11, low=100), 0.05)
    for name, args in KNOWN.items():
        co, xyz, _ = lattice_box(**args)
        out["known_" + name] = (co, xyz, band)
    for seed in (1, 2, 3, 4):
        co, xyz = random_cloud(seed, 700 + 333 * seed)
        out["random_%d" % seed] = (co, xyz, band)
    bad = _filled(100, 12).copy()
    bad[17, 1] = np.nan
    out["nan_coordinate"] = (COEFF_Z, bad, band)
    far = _filled(100, 13).copy()
    far[3, 0] = 64.5
    out["beyond_range"] = (COEFF_Z, far, band)
    out["no_plane"] = (np.zeros(4, np.float32), _filled(100, 14), band)
    out["two_points"] = (COEFF_Z, _filled(2, 15), band)
    return out


MAX_HULL_PLUS = BF.MAX_HULL + 1
# the known answers: a 3-4-5 rectangle, an axis-aligned one, a square; d < 0; the dominant axis x, y and z
KNOWN = {
    "rect_345": dict(na=40, nb=20, step_a=(3, 4), step_b=(-4, 3), height=0.0625, origin=(7, -9)),
    "rect_axis": dict(na=50, nb=30, step_a=(4, 0), step_b=(0, 4), height=0.03125, origin=(-60, 11)),
    "square": dict(na=24, nb=24, step_a=(4, 0), step_b=(0, 4), height=0.046875, origin=(5, 5), side_rows=0),
    "d_negative": dict(na=40, nb=20, step_a=(3, 4), step_b=(-4, 3), height=0.0625, origin=(7, -9), d_sign=-1),
    "axis_x": dict(na=40, nb=20, step_a=(3, 4), step_b=(-4, 3), height=0.0625, origin=(7, -9), normal_axis=0),
    "axis_y": dict(na=40, nb=20, step_a=(3, 4), step_b=(-4, 3), height=0.0625, origin=(7, -9), normal_axis=1),
}
