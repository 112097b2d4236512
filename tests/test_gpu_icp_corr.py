"""The ICP maximum correspondence distance (cd_set_icp_max_correspondence_distance, rule C8) on the GPU, in every ICP driver.

The oracle has no bound, and needs none: the moment and MSE sums are order-free integers (rule C4), so an ICP over P u Q whose
bound rejects exactly Q at every iteration is bit for bit an unbounded ICP over P alone - which the oracle checks.  Every
bounded result below is also shown to differ from the unbounded one, so a setter that stores the value and does nothing
else fails here."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, rot_xyz
from perception_amd import capi, pcd, synth, templates

pytestmark = pytest.mark.gpu
NPIX = synth.WIDTH * synth.HEIGHT

# driver modes (environment read when a context is created): the lattice path, then the generic searches
LAT = ("lat", {})
GENERIC = [("auto", {"CUBOID_ICP_LATTICE": "0"}),
           ("sliced", {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_MODE": "sliced"}),
           ("sliced-multi", {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_MODE": "sliced", "CUBOID_ICP_PERSIST": "0"}),
           ("cluster", {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_MODE": "cluster"}),
           ("pipe", {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_MODE": "pipe"})]
ENV_KEYS = ("CUBOID_ICP_LATTICE", "CUBOID_ICP_MODE", "CUBOID_ICP_PERSIST")


def make_ctx(monkeypatch, env, templates_by_slot, max_points=NPIX, max_frames=1, dist=None):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = capi.Context(max_points=max_points, max_frames=max_frames)
    for slot, t in templates_by_slot.items():
        c.set_template(slot, t)
    if dist is not None:
        c.set_icp_max_correspondence_distance(dist)
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    return c


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def xform(T, p):
    """The kernels' canonical 4x4 x point product (icp_solve.hpp xform), float32, one rounding per operation."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], 1).astype(np.float32)


def fitness(O, tpl, src, T):
    """getFitnessScore() of T over ALL of src, unbounded (rule 4 of C8), as the library sums it (rule C4)."""
    _, d2 = O.nn(tpl, xform(T, src))
    s = np.rint(d2.astype(np.float64) * 2.0 ** 36).astype(np.int64).sum()
    return float(np.ldexp(float(s), -36)) / len(src)


def same_icp(a, b):
    return (list(a.T) == list(b.T) and a.iterations == b.iterations and a.converged == b.converged)


def cluster_near(tpl, n, seed):
    """A source that starts near the template: a subset moved by a small rigid motion, plus 1 mm of noise."""
    rng = np.random.default_rng(seed)
    p = tpl[rng.choice(len(tpl), size=min(n, len(tpl)), replace=False)].astype(np.float64)
    R = rot_xyz(*np.deg2rad(rng.uniform(-3, 3, 3)))
    p = p @ R.T + rng.uniform(-0.01, 0.01, 3) + rng.normal(0, 0.001, p.shape)
    return p.astype(np.float32)


def far_points(tpl, n, seed):
    """n points at least 0.4 m from every template point."""
    rng = np.random.default_rng(seed)
    c = tpl.mean(0) + np.array([0.0, 0.0, 0.6], np.float32)
    q = (c + rng.uniform(-0.05, 0.05, (n, 3))).astype(np.float32)
    return q


def interleave(P, Q, seed):
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(len(P) + len(Q), size=len(Q), replace=False))
    mask = np.zeros(len(P) + len(Q), bool)
    mask[pos] = True
    out = np.empty((len(P) + len(Q), 3), np.float32)
    out[mask], out[~mask] = Q, P
    return out


@pytest.fixture(scope="module")
def tpl_default():
    return templates.template_xyz32(**templates.DEFAULT_TEMPLATE)


@pytest.fixture(scope="module")
def tpl_eraser():
    return pcd.read_xyz(os.path.join(GOLDEN, "eraser_ascii.pcd"))


@pytest.fixture(scope="module")
def tpl_big():
    t = pcd.read_xyz(os.path.join(GOLDEN, "template_cuboid_L200_W100_H75.pcd"))
    assert len(t) == 21400
    return t


# ---- 1. unbounded changes nothing ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"CUBOID_ICP_LATTICE": "0"}], ids=["lat", "generic"])
def test_unbounded_is_the_default_path_byte_for_byte(monkeypatch, tpl_default, env):
    frames = np.stack([synth.frame(i) for i in range(32)], 0)
    prm = capi.default_params()
    recs = []
    for d in (None, float("inf"), float(np.sqrt(np.finfo(np.float64).max)), 1e30):
        c = make_ctx(monkeypatch, env, {0: tpl_default}, max_frames=32, dist=d)
        try:
            res, _, _ = c.process_batch(frames, prm)
            recs.append(capi.results_to_array(res).copy())
            assert c.icp_max_correspondence_distance() == (float("inf") if d is None else d)
        finally:
            c.close()
    for r in recs[1:]:
        assert np.array_equal(r, recs[0])


# ---- 2. subset identity in every driver ---------------------------------------------------------------------------------
def _subset_identity(O, monkeypatch, env, tpl, P, seed):
    Q = far_points(tpl, 300, seed)
    X = interleave(P, Q, seed)
    prm = capi.default_params()
    s0, ro, _ = O.icp(tpl, P, prm, nn_mode=1)
    cb = make_ctx(monkeypatch, env, {0: tpl}, max_points=len(X), dist=0.1)
    cu = make_ctx(monkeypatch, env, {0: tpl}, max_points=len(X))
    try:
        sb, rb, _ = cb.icp(0, X, prm)
        su, ru, _ = cu.icp(0, P, prm)
        _, rx, _ = cu.icp(0, X, prm)
    finally:
        cb.close()
        cu.close()
    assert sb == su == capi.CD_OK and s0 == 0
    assert same_icp(rb, ru) and same_icp(rb, ro), (rb.iterations, ru.iterations, ro.iterations)
    assert rb.iterations > 0 and rb.converged == 1
    assert list(rx.T) != list(rb.T), "the bound made no difference"
    f = fitness(O, tpl, X, rb.T)
    assert abs(rb.fitness - f) <= 1e-12 * abs(f)
    assert ru.fitness != rb.fitness


@pytest.mark.parametrize("mode", [LAT] + GENERIC, ids=lambda m: m[0])
def test_subset_identity_default_template(O, monkeypatch, tpl_default, mode):
    _subset_identity(O, monkeypatch, mode[1], tpl_default, cluster_near(tpl_default, 900, 1), 11)


@pytest.mark.parametrize("mode", GENERIC, ids=lambda m: m[0])
def test_subset_identity_scanned_template(O, monkeypatch, tpl_eraser, mode):
    _subset_identity(O, monkeypatch, mode[1], tpl_eraser, cluster_near(tpl_eraser, 700, 2), 12)


def test_subset_identity_big_template(O, monkeypatch, tpl_big):
    _subset_identity(O, monkeypatch, {"CUBOID_ICP_LATTICE": "0"}, tpl_big, cluster_near(tpl_big, 800, 3), 13)


# ---- 3. boundary and rounding -------------------------------------------------------------------------------------------
def _below_bottom_face(O, tpl):
    """Points straight below the middle of the bottom face (z = -H/2) at distances near 0.1 m, with their float d2."""
    zb = tpl[:, 2].min()
    bottom = tpl[tpl[:, 2] == zb]
    t = bottom[np.argmin(np.abs(bottom[:, 0]) + np.abs(bottom[:, 1]))]
    h = np.float32(0.1) + np.arange(-4000, 4000, dtype=np.float32) * np.float32(2.0 ** -27)
    q = np.stack([np.full_like(h, t[0]), np.full_like(h, t[1]), (np.float32(zb) - h).astype(np.float32)], 1)
    idx, d2 = O.nn(tpl, q)
    return q, d2


@pytest.mark.parametrize("mode", [LAT, GENERIC[0]], ids=lambda m: m[0])
def test_boundary_is_kept_and_rounding_goes_down(O, monkeypatch, tpl_default, mode):
    q, d2 = _below_bottom_face(O, tpl_default)
    vals = set(d2.view(np.uint32).tolist())
    # a float s that some point reaches exactly, and whose successor another point reaches
    s = next(np.uint32(v).view(np.float32) for v in sorted(vals) if v + 1 in vals)
    s_next = np.nextafter(s, np.float32(np.inf))
    q_eq, q_up = q[d2 == s][:1], q[d2 == s_next][:1]
    # the d for which tau == s: d*d in [s, next(s)), here just above s
    d = float(np.sqrt(np.float64(s)))
    while np.float64(d) * d < np.float64(s):
        d = float(np.nextafter(d, np.inf))
    tau, bounded = capi.icp_correspondence_threshold(d)
    assert bounded == 1 and np.float32(tau) == s
    # a d whose (float)(d*d) rounds UP to s_next: tau is s, so a point with d2 == (float)(d*d) is rejected
    d_up = float(np.sqrt(np.float64(s_next) - 0.25 * (np.float64(s_next) - np.float64(s))))
    assert np.float32(np.float64(d_up) * d_up) == s_next and np.float32(capi.icp_correspondence_threshold(d_up)[0]) == s

    P = cluster_near(tpl_default, 600, 4)
    prm = capi.default_params()
    prm.icp_max_iterations = 1      # only the first correspondence set counts
    env = mode[1]
    X = interleave(P, np.concatenate([q_eq, q_up, far_points(tpl_default, 50, 5)]), 6)
    with_eq = interleave(P, q_eq, 7)
    cb = make_ctx(monkeypatch, env, {0: tpl_default}, max_points=len(X))
    cu = make_ctx(monkeypatch, env, {0: tpl_default}, max_points=len(X))
    try:
        for dist in (d, d_up):
            cb.set_icp_max_correspondence_distance(dist)
            _, rb, _ = cb.icp(0, X, prm)
            _, rp, _ = cu.icp(0, P, prm)
            _, re, _ = cu.icp(0, with_eq, prm)
            _, rx, _ = cu.icp(0, X, prm)
            # both distances have tau == s: the point with d2 == tau is kept, the one at the next float is not (for d_up that
            # is the point with d2 == (float)(d_up * d_up), which a threshold rounded to nearest would keep)
            assert rb.iterations == 1
            assert same_icp(rb, re) and not same_icp(rb, rp) and not same_icp(rb, rx)
        # and alone: with d_up, a point with d2 == (float)(d_up * d_up) changes nothing
        cb.set_icp_max_correspondence_distance(d_up)
        X2 = interleave(P, q_up, 8)
        _, rb2, _ = cb.icp(0, X2, prm)
        _, rp2, _ = cu.icp(0, P, prm)
        _, rx2, _ = cu.icp(0, X2, prm)
        assert same_icp(rb2, rp2) and not same_icp(rb2, rx2)
    finally:
        cb.close()
        cu.close()


# ---- 4. too few correspondences -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [LAT] + GENERIC, ids=lambda m: m[0])
def test_too_few_correspondences_stop_before_the_update(O, monkeypatch, tpl_default, mode):
    zb = tpl_default[:, 2].min()
    src = tpl_default[tpl_default[:, 2] == zb][::7] + np.float32([0.0, 0.0, 0.05])   # 5 cm off the bottom face
    prm = capi.default_params()
    c = make_ctx(monkeypatch, mode[1], {0: tpl_default}, max_points=len(src), dist=1e-3)
    try:
        st, r, al = c.icp(0, src, prm, want_aligned=True)
        assert st == capi.CD_ERR_FEW_CORRESPONDENCES
        assert (r.iterations, r.converged, r.accepted) == (0, 0, 0)
        assert list(r.T) == list(np.eye(4, dtype=np.float32).ravel())
        assert abs(r.fitness - fitness(O, tpl_default, src, np.eye(4))) <= 1e-12 * r.fitness
        assert np.array_equal(al, src)
        G = rigid(rot_xyz(0.01, -0.02, 0.015), [0.002, -0.001, 0.003]).astype(np.float32)
        prm.icp_use_guess = capi.CD_GUESS_PARAMS
        prm.icp_guess[:] = list(G.ravel())
        st, r, _ = c.icp(0, src, prm)
        assert st == capi.CD_ERR_FEW_CORRESPONDENCES and (r.iterations, r.converged) == (0, 0)
        assert list(r.T) == list(G.ravel())
        assert abs(r.fitness - fitness(O, tpl_default, src, G)) <= 1e-12 * r.fitness
        # unbounded again: the ICP runs
        c.set_icp_max_correspondence_distance(None)
        st, r, _ = c.icp(0, src, prm)
        assert st == capi.CD_OK and r.iterations > 0 and r.converged == 1
        # bad arguments leave the setting as it is
        c.set_icp_max_correspondence_distance(0.25)
        for bad in (-1.0, float("nan")):
            with pytest.raises(capi.CuboidError):
                c.set_icp_max_correspondence_distance(bad)
            assert c.icp_max_correspondence_distance() == 0.25
    finally:
        c.close()


@pytest.mark.parametrize("mode", [LAT, GENERIC[0]], ids=lambda m: m[0])
def test_reference_line_175_in_a_batch(monkeypatch, tpl_default, mode):
    """Config-3 frames, identity guess, d = 0.05 (the reference's commented-out line): every cluster lies ~0.55 m from the
    object-centred template, so every pair stops at iteration 0 - a result, not an error."""
    frames = np.stack([synth.frame(i) for i in range(4)], 0)
    prm = capi.default_params()
    cu = make_ctx(monkeypatch, mode[1], {0: tpl_default}, max_frames=4)
    cb = make_ctx(monkeypatch, mode[1], {0: tpl_default}, max_frames=4, dist=0.05)
    try:
        ru, _, _ = cu.process_batch(frames, prm)
        rb, _, _ = cb.process_batch(frames, prm)
    finally:
        cu.close()
        cb.close()
    eye = list(np.eye(4, dtype=np.float32).ravel())
    n = 0
    for f in range(4):
        assert rb[f].status == capi.CD_OK
        for fld in ("n_cropped", "n_voxels", "n_plane", "n_objects", "n_clusters", "ransac_iterations", "flags"):
            assert getattr(rb[f], fld) == getattr(ru[f], fld)
        assert bytes(rb[f].plane) == bytes(ru[f].plane)
        for k in range(min(rb[f].n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME)):
            a, b = rb[f].clusters[k], ru[f].clusters[k]
            assert (a.iterations, a.converged, a.accepted) == (0, 0, 0) and list(a.T) == eye
            assert b.iterations > 0
            n += 1
    assert n > 0


# ---- 5. batch == single call, across drivers, on real scenes, with a per-frame guess -----------------------------------
def _perturb(T, rng):
    P = rigid(rot_xyz(*np.deg2rad(rng.uniform(-2, 2, 3))), rng.uniform(-0.01, 0.01, 3) / np.sqrt(3))
    return (P @ np.asarray(T, np.float64).reshape(4, 4)).astype(np.float32)


def _tracking(O, monkeypatch, tpl, prm, frames, modes, depth=None):
    F = len(frames)
    batch = np.stack(frames, 0)
    # unbounded pass: each frame's best T, perturbed by a small seeded motion
    c0 = make_ctx(monkeypatch, {}, {0: tpl}, max_frames=F)
    try:
        r0, _, _ = c0.process_batch(batch, prm)
        rng = np.random.default_rng(21)
        guesses = np.stack([_perturb(min((r0[f].clusters[k] for k in range(min(r0[f].n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME))),
                                         key=lambda r: r.fitness).T if r0[f].n_clusters else np.eye(4), rng) for f in range(F)], 0)
        # the distance: a quantile of the first correspondence distances under the guesses, so that some are rejected while
        # every pair keeps enough to start
        dists, clusters = [], []
        for f in range(F):
            for k in range(min(r0[f].n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME)):
                pts = c0.cluster_points(f, k, aligned=False)[:, :3].copy()
                _, d2 = O.nn(tpl, xform(guesses[f], pts))
                dists.append(np.sqrt(d2.astype(np.float64)))
                clusters.append((f, k, pts))
    finally:
        c0.close()
    assert clusters
    d = float(np.quantile(np.concatenate(dists), 0.8))
    assert all((x <= d).sum() >= 3 for x in dists)
    gprm = capi.default_params()
    for fld, _ in capi.CdParams._fields_:
        setattr(gprm, fld, getattr(prm, fld))
    gprm.icp_use_guess = capi.CD_GUESS_PER_FRAME
    recs = {}
    for name, env in modes:
        c = make_ctx(monkeypatch, env, {0: tpl}, max_frames=F, dist=d)
        try:
            c.set_frame_guesses(guesses)
            res, _, _ = c.process_batch(batch, gprm)
            recs[name] = capi.results_to_array(res).copy()
            if depth is not None and name == modes[0][0]:
                dimg, cimg, cam = depth
                rd, _, _ = c.process_depth_batch(dimg, cimg, cam, gprm)
                clouds = np.stack([c.depth_to_cloud(cam, dimg[f], cimg[f]).view(np.float32) for f in range(F)], 0)
                rc, _, _ = c.process_batch(clouds, gprm)
                assert np.array_equal(capi.results_to_array(rd), capi.results_to_array(rc))
        finally:
            c.close()
    first = recs[modes[0][0]]
    for name in recs:
        assert np.array_equal(recs[name], first), name
    res = capi.results_from_array(first)
    # each record == cd_icp on that cluster's points with the same guess and d; and the bound made a difference
    cs = make_ctx(monkeypatch, modes[0][1], {0: tpl}, dist=d)
    cu = make_ctx(monkeypatch, modes[0][1], {0: tpl}, max_frames=F)
    try:
        cu.set_frame_guesses(guesses)
        ru, _, _ = cu.process_batch(batch, gprm)
        differs = False
        for f, k, pts in clusters:
            sp = capi.default_params()
            for fld, _ in capi.CdParams._fields_:
                setattr(sp, fld, getattr(prm, fld))
            sp.icp_use_guess = capi.CD_GUESS_PARAMS
            sp.icp_guess[:] = list(guesses[f].ravel())
            st, r, _ = cs.icp(0, pts, sp)
            b = res[f].clusters[k]
            assert st == capi.CD_OK
            assert same_icp(r, b) and r.fitness == b.fitness and r.accepted == b.accepted, (f, k)
            assert b.iterations > 0
            differs |= bytes(b) != bytes(ru[f].clusters[k])
        assert differs, "the bound made no difference"
    finally:
        cs.close()
        cu.close()


def _depth_inputs(F):
    cam = capi.default_depth_camera()
    cam.width, cam.height = synth.WIDTH, synth.HEIGHT
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params()
    cam.depth_scale = synth.DEPTH_SCALE
    cam.color = capi.CD_COLOR_RGB8
    imgs = [synth.depth_frame(i, k_obj=1) for i in range(F)]
    return np.stack([a for a, _ in imgs], 0), np.stack([b for _, b in imgs], 0), cam


def test_tracking_config3(O, monkeypatch, tpl_default):
    F = 16
    frames = [synth.frame(i, k_obj=1) for i in range(F)]
    _tracking(O, monkeypatch, tpl_default, capi.default_params(), frames, [LAT] + GENERIC, depth=_depth_inputs(F))


def test_tracking_object_launch(O, monkeypatch):
    tpl = pcd.read_xyz(os.path.join(GOLDEN, "eraser_ascii_tf.pcd"))
    prm = capi.default_params()
    prm.leaf_size = 0.001
    prm.plane_distance_threshold = 0.01
    frames = [synth.frame(i, k_obj=1) for i in range(16)]
    _tracking(O, monkeypatch, tpl, prm, frames, GENERIC)


def test_tracking_big_template_pipe_big(O, monkeypatch, tpl_big):
    frames = [synth.frame(i, k_obj=1) for i in range(4)]
    _tracking(O, monkeypatch, tpl_big, capi.default_params(), frames,
              [("pipe", {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_MODE": "pipe"}), ("sliced", {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_MODE": "sliced"})])


# ---- 6. state is per context --------------------------------------------------------------------------------------------
def test_state_is_per_context_and_pipeline_forwards_it(monkeypatch, tpl_default):
    from perception_amd.batch import BatchPipeline
    frames = np.stack([synth.frame(i) for i in range(2)], 0)
    prm = capi.default_params()
    a = make_ctx(monkeypatch, {}, {0: tpl_default}, max_frames=2)
    b = make_ctx(monkeypatch, {}, {0: tpl_default}, max_frames=2)
    try:
        ref, _, _ = b.process_batch(frames, prm)
        ref = capi.results_to_array(ref).copy()
        a.set_icp_max_correspondence_distance(0.05)
        assert b.icp_max_correspondence_distance() == float("inf")
        ra, _, _ = a.process_batch(frames, prm)
        rb, _, _ = b.process_batch(frames, prm)
        assert np.array_equal(capi.results_to_array(rb), ref)
        assert not np.array_equal(capi.results_to_array(ra), ref)
    finally:
        a.close()
        b.close()
    p = BatchPipeline(NPIX, 2, {0: tpl_default}, inflight=2, icp_max_correspondence_distance=0.05)
    try:
        assert [cx.icp_max_correspondence_distance() for cx in p.contexts] == [0.05, 0.05]
    finally:
        p.close()
    p = BatchPipeline(NPIX, 2, {0: tpl_default}, inflight=1)
    try:
        assert p.contexts[0].icp_max_correspondence_distance() == float("inf")
    finally:
        p.close()
