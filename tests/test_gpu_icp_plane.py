"""Rule C17 on the GPU: k_icp_plane and its driver against the numpy module (perception_amd/icp_plane.py), bit for bit - the
words of T, iterations, converged, accepted, the bits of the fitness, the three counters and the aligned points.  No tolerances.
The mirror's nearest neighbour is a brute force, so the iteration limit is capped where the full ICP would take it long."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, rot_xyz
from perception_amd import capi, cluster_frame as cf, icp_plane as IP, pcd, synth, templates

pytestmark = pytest.mark.gpu
NPIX = synth.WIDTH * synth.HEIGHT
W0, D0 = capi.CD_ICP_PLANE_WEIGHT_DEFAULT, capi.CD_ICP_PLANE_SWITCH_DEFAULT
ENV_KEYS = ("CUBOID_ICP_LATTICE", "CUBOID_ICP_MODE", "CUBOID_ICP_PERSIST", "CUBOID_ICP_MAX_WG")


def make_ctx(monkeypatch, templates_by_slot, max_points=4096, max_frames=1, plane=(W0, D0), env=None):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    c = capi.Context(max_points=max_points, max_frames=max_frames)
    for slot, t in templates_by_slot.items():
        c.set_template(slot, t)
    if plane is not None:
        c.set_icp_plane_weight(*plane)
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    return c


def params(max_iter=None, guess=None):
    p = capi.default_params()
    if max_iter is not None:
        p.icp_max_iterations = max_iter
    if guess is not None:
        p.icp_use_guess = capi.CD_GUESS_PARAMS
        p.icp_guess[:] = [float(v) for v in np.asarray(guess, np.float32).ravel()]
    return p


def bits(x):
    return np.float64(x).view(np.uint64)


def assert_same(r, stats, m, aligned=None, where=""):
    """A library result (cd_cluster_result + one row of cluster_plane_stats) against the module's."""
    assert list(np.asarray(list(r.T), np.float32).view(np.uint32)) == list(m.T.view(np.uint32).ravel()), where
    assert (r.iterations, r.converged, r.accepted) == (m.iterations, m.converged, m.accepted), where
    assert bits(r.fitness) == bits(m.fitness), (where, r.fitness, m.fitness)
    assert [int(v) for v in stats[:3]] == [m.plane_iterations, m.first_plane_iteration, m.stopped_singular], where
    if aligned is not None:
        assert np.array_equal(aligned.view(np.uint32), m.aligned.view(np.uint32)), where


def run_icp(c, slot, src, prm):
    """cd_icp and its counters; the status is OK, or FEW_CORRESPONDENCES for a stop (too few or singular)."""
    st, r, al = c.icp(slot, src, prm, want_aligned=True)
    stats = c.cluster_plane_stats(0)
    assert stats.shape == (1, 4)
    return st, r, al, stats[0]


def check_against_mirror(c, slot, tpl, axes, src, prm, plane=(W0, D0), guess=None, d2_max=None, where=""):
    st, r, al, stats = run_icp(c, slot, src, prm)
    m = IP.icp(tpl, axes, src, prm, plane[0], plane[1], guess=guess, d2_max=d2_max)
    assert_same(r, stats, m, al, where)
    assert st == (capi.CD_ERR_FEW_CORRESPONDENCES if (m.stopped_singular or m.stopped_few) else capi.CD_OK), where
    return r, m


def moved_subset(tpl, n, seed, deg=3.0, shift=0.01, noise=0.001):
    """A subset of the template moved by a small rigid motion, plus noise (repeats when n exceeds the template)."""
    rng = np.random.default_rng(seed)
    p = tpl[rng.choice(len(tpl), size=n, replace=n > len(tpl))].astype(np.float64)
    R = rot_xyz(*np.deg2rad(rng.uniform(-deg, deg, 3)))
    return (p @ R.T + rng.uniform(-shift, shift, 3) + rng.normal(0, noise, p.shape)).astype(np.float32)


def beside_faces(tpl, n, seed):
    """Points below the bottom face and beside the side faces, beyond their rims: the correspondences sit on face edges."""
    rng = np.random.default_rng(seed)
    lo, hi = tpl.min(0), tpl.max(0)
    p = rng.uniform(lo - 0.004, hi + 0.004, (n, 3))
    p[0::3, 2] = lo[2] - rng.uniform(0.0005, 0.003, len(p[0::3]))
    p[1::3, 1] = lo[1] - rng.uniform(0.0005, 0.003, len(p[1::3]))
    p[2::3, 0] = lo[0] - rng.uniform(0.0005, 0.003, len(p[2::3]))
    return p.astype(np.float32)


def two_plates():
    """Three lattice faces, two of them on one axis: the general face loop over three faces (not one face per axis)."""
    X = np.arange(-0.05, 0.05, 0.002)
    Y = np.arange(-0.03, 0.03, 0.002)
    Z = np.arange(-0.02, 0.02, 0.002)
    xx, yy = np.meshgrid(X, Y)
    yz, zz = np.meshgrid(Y, Z)
    lo = np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, -0.02)], 1)
    hi = np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, 0.02)], 1)
    end = np.stack([np.full(yz.size, -0.05), yz.ravel(), zz.ravel()], 1)
    return np.round(np.concatenate([lo, hi, end], 0), 6).astype(np.float32)


@pytest.fixture(scope="module")
def tpl():
    return templates.template_xyz32(**templates.DEFAULT_TEMPLATE)


@pytest.fixture(scope="module")
def axes(tpl):
    return IP.face_axes(tpl)


# ---- pass and wave edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["moved", "beside"])
def test_pass_and_wave_edges(monkeypatch, tpl, axes, place):
    c = make_ctx(monkeypatch, {0: tpl})
    try:
        prm = params(max_iter=10)
        ran = 0
        for n in (3, 4, 63, 64, 65, 255, 256, 257, 1500):
            src = moved_subset(tpl, n, 100 + n) if place == "moved" else beside_faces(tpl, n, 200 + n)
            r, m = check_against_mirror(c, 0, tpl, axes, src, prm, where="n=%d" % n)
            ran += m.iterations
        assert ran > 20
    finally:
        c.close()


def test_plane_weights_from_the_first_iteration_and_other_weights(monkeypatch, tpl, axes):
    c = make_ctx(monkeypatch, {0: tpl})
    try:
        src = moved_subset(tpl, 700, 7)
        seen = set()
        for plane in ((W0, float("inf")), (1.0 / 1024.0, 0.01), (1.0, 0.01), (0.3, 0.0), (W0, 0.002)):
            c.set_icp_plane_weight(*plane)
            r, m = check_against_mirror(c, 0, tpl, axes, src, params(max_iter=8), plane=plane, where=str(plane))
            seen.add(bytes(r.T))
        assert len(seen) >= 4   # the setting reaches the kernel
    finally:
        c.close()


# ---- template shapes: one face per axis, the general loop over three faces, over six ---------------------------------------------------
@pytest.mark.parametrize("name", ["L200_W100_H75_3faces", "L200_W75_H100_3faces", "L200_W100_H75", "two_plates"])
def test_template_shapes(monkeypatch, name):
    t = two_plates() if name == "two_plates" else pcd.read_xyz(os.path.join(GOLDEN, "template_cuboid_%s.pcd" % name)).astype(np.float32)
    ax = IP.face_axes(t)
    distinct = capi.lattice_axes(t)[0]
    c = make_ctx(monkeypatch, {1: t})
    try:
        nface = c.template_lattice_faces(1)
        assert (nface, distinct) == {"L200_W100_H75": (6, 0), "two_plates": (3, 0)}.get(name, (3, 1))
        for n, seed in ((300, 1), (130, 2)):
            for src in (moved_subset(t, n, seed, deg=2.0, shift=0.004), beside_faces(t, n, seed + 10)):
                check_against_mirror(c, 1, t, ax, src, params(max_iter=8), where="%s n=%d" % (name, n))
    finally:
        c.close()


# ---- ties: mid-cell queries enter the tie walk ---------------------------------------------------------------------------------------
def test_mid_cell_queries(monkeypatch, tpl, axes):
    bottom = np.nonzero(axes == 2)[0].reshape(50, 100)
    a, b = tpl[bottom[5:45:2, 5:95:3]].reshape(-1, 3), tpl[bottom[6:46:2, 6:96:3]].reshape(-1, 3)
    mid = ((a + b) * np.float32(0.5)).astype(np.float32)          # the middle of a cell: four lattice points at one distance
    half = ((a + tpl[bottom[5:45:2, 6:96:3]].reshape(-1, 3)) * np.float32(0.5)).astype(np.float32)   # the middle of an edge: two
    src = np.concatenate([mid, half, a], 0)
    src[:, 2] += np.float32(0.0004)
    idx, d2 = IP.nearest(tpl, src[:len(mid)])
    ties = ((src[:len(mid), None, :] - tpl[None, bottom[5:47, 5:97].ravel(), :]) ** 2).sum(-1)
    assert (np.isclose(ties, ties.min(1, keepdims=True), rtol=0, atol=0).sum(1) > 1).sum() > len(mid) // 4   # exact float ties exist
    c = make_ctx(monkeypatch, {0: tpl})
    try:
        check_against_mirror(c, 0, tpl, axes, src, params(max_iter=4), where="ties")
    finally:
        c.close()


# ---- queue refill and restaging: more pairs than workgroups, two templates ------------------------------------------------------------
def test_refill_two_templates_every_pair_equals_its_own_icp(monkeypatch, tpl, frames4):
    t1 = pcd.read_xyz(os.path.join(GOLDEN, "template_cuboid_L200_W100_H75_3faces.pcd")).astype(np.float32)
    frames = np.stack(frames4, 0)
    prm = capi.default_params()
    # one workgroup slot's worth of grid (two workgroups), so that every workgroup runs several pairs of both templates in turn
    c = make_ctx(monkeypatch, {0: tpl, 1: t1}, max_points=NPIX, max_frames=4, env={"CUBOID_ICP_MAX_WG": "1"})
    s = make_ctx(monkeypatch, {0: tpl, 1: t1}, max_points=NPIX, max_frames=1)
    try:
        per_slot = {}
        for slot in (0, 1, -1):
            prm.template_slot = slot
            res, _, _ = c.process_batch(frames, prm)
            assert all(res[f].status == capi.CD_OK for f in range(4))
            per_slot[slot] = [(c.cluster_results(f), c.cluster_plane_stats(f)) for f in range(4)]
            if slot == -1:
                clusters = [[c.cluster_points(f, k, aligned=False)[:, :3].copy() for k in range(res[f].n_clusters)] for f in range(4)]
        n_pairs = 0
        for f in range(4):
            assert len(clusters[f]) > 0
            for k, pts in enumerate(clusters[f]):
                alone = {}
                for slot in (0, 1):
                    st, r, _, stats = run_icp(s, slot, pts, capi.default_params())
                    assert st == capi.CD_OK and r.iterations > 0
                    got, gstats = per_slot[slot][f][0][k], per_slot[slot][f][1][k]
                    assert (list(got.T), got.iterations, got.converged, got.accepted, bits(got.fitness), got.template_slot, got.size) == \
                        (list(r.T), r.iterations, r.converged, r.accepted, bits(r.fitness), slot, len(pts))
                    assert list(gstats) == list(stats)
                    alone[slot] = (r, stats)
                    n_pairs += 1
                # all pairs in one stage: the cluster keeps the lower fitness, ties the lower slot - and that pair's counters
                best = 1 if alone[1][0].fitness < alone[0][0].fitness else 0
                got, gstats = per_slot[-1][f][0][k], per_slot[-1][f][1][k]
                assert got.template_slot == best and list(got.T) == list(alone[best][0].T) and got.iterations == alone[best][0].iterations
                assert bits(got.fitness) == bits(alone[best][0].fitness) and list(gstats) == list(alone[best][1])
        assert n_pairs >= 8   # more pairs than the two workgroups of the launch
    finally:
        c.close()
        s.close()


# ---- with rule C8 ------------------------------------------------------------------------------------------------------------------------
def test_with_correspondence_bound(monkeypatch, tpl, axes):
    P = moved_subset(tpl, 600, 31)
    rng = np.random.default_rng(32)
    far = (tpl.mean(0) + np.float32([0, 0, 0.6]) + rng.uniform(-0.05, 0.05, (150, 3))).astype(np.float32)
    X = np.concatenate([P[:300], far, P[300:]], 0)
    c = make_ctx(monkeypatch, {0: tpl})
    try:
        prm = params(max_iter=6)
        # a bound that rejects some correspondences (the far points), against the unbounded ICP of the same cloud
        tau, bounded = capi.icp_correspondence_threshold(0.1)
        assert bounded == 1
        c.set_icp_max_correspondence_distance(0.1)
        rb, _ = check_against_mirror(c, 0, tpl, axes, X, prm, d2_max=tau, where="bounded")
        c.set_icp_max_correspondence_distance(None)
        ru, _ = check_against_mirror(c, 0, tpl, axes, X, prm, where="unbounded")
        assert list(rb.T) != list(ru.T)
        # the boundary value: a distance whose threshold is exactly some point's first d2 keeps that point
        _, d2 = IP.nearest(tpl, P)
        s = np.sort(d2)[len(d2) // 2]
        d = float(np.sqrt(np.float64(s)))
        while np.float64(d) * d < np.float64(s):
            d = float(np.nextafter(d, np.inf))
        tau, _ = capi.icp_correspondence_threshold(d)
        assert np.float32(tau) == s
        c.set_icp_max_correspondence_distance(d)
        r_eq, m_eq = check_against_mirror(c, 0, tpl, axes, P, params(max_iter=1), d2_max=tau, where="boundary")
        m_below = IP.icp(tpl, axes, P, params(max_iter=1), W0, D0, d2_max=np.nextafter(np.float32(tau), np.float32(0)))
        assert not np.array_equal(m_eq.T, m_below.T)
        # fewer than three kept: stops before the update
        zb = tpl[:, 2].min()
        off = tpl[tpl[:, 2] == zb][::7] + np.float32([0.0, 0.0, 0.05])
        c.set_icp_max_correspondence_distance(1e-3)
        st, r, al, stats = run_icp(c, 0, off, capi.default_params())
        assert st == capi.CD_ERR_FEW_CORRESPONDENCES and (r.iterations, r.converged, r.accepted) == (0, 0, 0)
        assert list(r.T) == list(np.eye(4, dtype=np.float32).ravel()) and np.array_equal(al, off) and list(stats) == [0, 0, 0, 0]
        m = IP.icp(tpl, axes, off, capi.default_params(), W0, D0, d2_max=capi.icp_correspondence_threshold(1e-3)[0])
        assert m.stopped_few == 1 and bits(m.fitness) == bits(r.fitness)
    finally:
        c.close()


# ---- with every guess mode, fused --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_clusters(O, tpl, frames4):
    prm = capi.default_params()
    t_rec = cf.shape_frame(tpl)
    out = []
    for f in frames4:
        o = O.process_frame(f, prm, tpl, want_clouds=True)
        srcs = [o["objects"][o["labels"] == k] for k in range(o["result"].n_clusters)]
        out.append([(s, np.asarray(cf.guess(cf.shape_frame(s), t_rec)[0], np.float32)) for s in srcs])
    return out


@pytest.mark.parametrize("mode", ["params", "per_frame", "cluster"])
def test_guess_modes_on_a_batch(monkeypatch, tpl, axes, frames4, oracle_clusters, mode):
    prm = params(max_iter=8)
    c = make_ctx(monkeypatch, {0: tpl}, max_points=NPIX, max_frames=4)
    try:
        if mode == "params":
            prm.icp_use_guess = capi.CD_GUESS_PARAMS
            prm.icp_guess[:] = [float(v) for v in oracle_clusters[0][0][1].ravel()]
            guess_of = lambda f, k: oracle_clusters[0][0][1]
        elif mode == "per_frame":
            prm.icp_use_guess = capi.CD_GUESS_PER_FRAME
            c.set_frame_guesses(np.stack([oracle_clusters[f][0][1] for f in range(4)], 0))
            guess_of = lambda f, k: oracle_clusters[f][0][1]
        else:
            prm.icp_use_guess = capi.CD_GUESS_CLUSTER
            guess_of = lambda f, k: oracle_clusters[f][k][1]
        res, _, _ = c.process_batch(np.stack(frames4, 0), prm)
        n = 0
        for f in range(4):
            assert res[f].status == capi.CD_OK and res[f].n_clusters == len(oracle_clusters[f])
            stats = c.cluster_plane_stats(f)
            assert len(stats) == res[f].n_clusters
            for k, (src, _) in enumerate(oracle_clusters[f]):
                m = IP.icp(tpl, axes, src, prm, W0, D0, guess=guess_of(f, k))
                assert_same(res[f].clusters[k], stats[k], m, where="%s f=%d k=%d" % (mode, f, k))
                assert res[f].clusters[k].size == len(src)
                n += 1
        assert n >= 4 and c.timing().icp_search == 1
    finally:
        c.close()


def test_depth_call_and_frame_call_equal_the_cloud_call(monkeypatch, tpl):
    F = 2
    cam = capi.default_depth_camera()
    cam.width, cam.height = synth.WIDTH, synth.HEIGHT
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params()
    cam.depth_scale = synth.DEPTH_SCALE
    cam.color = capi.CD_COLOR_RGB8
    imgs = [synth.depth_frame(i, k_obj=1) for i in range(F)]
    dimg, cimg = np.stack([a for a, _ in imgs], 0), np.stack([b for _, b in imgs], 0)
    prm = capi.default_params()
    c = make_ctx(monkeypatch, {0: tpl}, max_points=NPIX, max_frames=F)
    try:
        rd, _, _ = c.process_depth_batch(dimg, cimg, cam, prm)
        sd = [c.cluster_plane_stats(f) for f in range(F)]
        clouds = np.stack([c.depth_to_cloud(cam, dimg[f], cimg[f]).view(np.float32) for f in range(F)], 0)
        rc, _, _ = c.process_batch(clouds, prm)
        assert np.array_equal(capi.results_to_array(rd), capi.results_to_array(rc))
        n = 0
        for f in range(F):
            assert np.array_equal(sd[f], c.cluster_plane_stats(f)) and len(sd[f]) == rc[f].n_clusters
            n += int(sd[f][:, 0].sum())
        assert n > 0   # plane iterations were run
        want = [bytes(rc[f].clusters[0]) for f in range(F)]
        for f in range(F):   # cd_process_frame is the fused call on one frame
            r1, _, _ = c.process_frame(clouds[f], prm)
            assert r1.n_clusters == rc[f].n_clusters and bytes(r1.clusters[0]) == want[f]
            assert np.array_equal(c.cluster_plane_stats(0), sd[f])
    finally:
        c.close()


# ---- singular stop ---------------------------------------------------------------------------------------------------------------------------
def test_singular_stop(monkeypatch, tpl, axes):
    # one line parallel to the bottom face, coordinates on a 2^-9 grid: M is exact, hence exactly singular (tests/test_icp_plane_cpu.py)
    x = (np.arange(81, dtype=np.float32) - np.float32(40)) * np.float32(2.0 ** -9)
    line = np.stack([x, np.full(81, 2.0 ** -6, np.float32), np.full(81, -2.0 ** -6, np.float32)], 1).astype(np.float32)
    c = make_ctx(monkeypatch, {0: tpl})
    try:
        for plane in ((W0, float("inf")), (W0, D0)):
            c.set_icp_plane_weight(*plane)
            st, r, al, stats = run_icp(c, 0, line, capi.default_params())
            m = IP.icp(tpl, axes, line, capi.default_params(), plane[0], plane[1])
            assert m.stopped_singular == 1
            assert st == capi.CD_ERR_FEW_CORRESPONDENCES and b"singular" in c.lib.cd_last_error(c.h)
            assert_same(r, stats, m, al, where=str(plane))
            assert (r.iterations, r.converged, r.accepted) == (0, 0, 0) and list(stats[:3]) == [0, 0, 1]
        # the next call of the context is an ordinary one
        check_against_mirror(c, 0, tpl, axes, moved_subset(tpl, 200, 5), params(max_iter=5), where="after")
        # fewer than three points never reach the kernel: the library's own status, zero counters
        st, r, _, stats = run_icp(c, 0, tpl[:2].copy(), capi.default_params())
        assert st == capi.CD_ERR_FEW_CORRESPONDENCES and r.iterations == 0 and list(stats) == [0, 0, 0, 0]
    finally:
        c.close()


# ---- off is off --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"CUBOID_ICP_LATTICE": "0"}], ids=["lat", "generic"])
def test_off_is_off(monkeypatch, tpl, frames4, env):
    frames = np.stack(frames4, 0)
    prm = capi.default_params()
    never = make_ctx(monkeypatch, {0: tpl}, max_points=NPIX, max_frames=4, plane=None, env=env)
    off = make_ctx(monkeypatch, {0: tpl}, max_points=NPIX, max_frames=4, plane=(W0, D0), env=env)
    try:
        r_never, _, _ = never.process_batch(frames, prm)
        a = capi.results_to_array(r_never).copy()
        r_on, _, _ = off.process_batch(frames, prm)
        on = capi.results_to_array(r_on).copy()
        off.set_icp_plane_weight(0.0, 123.0)
        assert off.icp_plane_weight() == (0.0, D0)
        r_off, _, _ = off.process_batch(frames, prm)
        assert np.array_equal(capi.results_to_array(r_off), a)
        assert not np.array_equal(on, a)   # ... and on is on, in either configuration
        assert off.timing().icp_search == (1 if not env else 0)
        with pytest.raises(capi.CuboidError):
            off.cluster_plane_stats(0)
        with pytest.raises(capi.CuboidError):
            never.cluster_plane_stats(0)
        st, r, _ = never.icp(0, moved_subset(tpl, 300, 3), prm)
        assert st == capi.CD_OK
        with pytest.raises(capi.CuboidError):
            never.cluster_plane_stats(0)
    finally:
        never.close()
        off.close()


# ---- settings ----------------------------------------------------------------------------------------------------------------------------------
def test_settings_and_refusals(monkeypatch, tpl):
    from perception_amd.batch import BatchPipeline
    a = make_ctx(monkeypatch, {0: tpl}, plane=None)
    b = make_ctx(monkeypatch, {0: tpl}, plane=None)
    try:
        assert a.icp_plane_weight() == (0.0, D0)
        a.set_icp_plane_weight(0.25, 0.02)
        assert a.icp_plane_weight() == (0.25, 0.02) and b.icp_plane_weight() == (0.0, D0)   # per context
        for bad in ((2.0, 0.01), (1.0 / 2048.0, 0.01), (-0.5, 0.01), (float("nan"), 0.01), (float("inf"), 0.01),
                    (0.25, -1.0), (0.25, float("nan")), (0.25, float("-inf"))):
            with pytest.raises(capi.CuboidError) as e:
                a.set_icp_plane_weight(*bad)
            assert e.value.status == capi.CD_ERR_INVALID_ARG
            assert a.icp_plane_weight() == (0.25, 0.02)   # a refused change keeps the old setting
        for good in ((1.0, 0.0), (1.0 / 1024.0, float("inf")), (W0, D0)):
            a.set_icp_plane_weight(*good)
            assert a.icp_plane_weight() == good
        a.set_icp_plane_weight(None)
        assert a.icp_plane_weight()[0] == 0.0
    finally:
        a.close()
        b.close()
    p = BatchPipeline(4096, 1, {0: tpl}, inflight=2, icp_plane_weight=(W0, 0.02))
    try:
        assert [cx.icp_plane_weight() for cx in p.contexts] == [(W0, 0.02), (W0, 0.02)]
    finally:
        p.close()
    p = BatchPipeline(4096, 1, {0: tpl}, inflight=1)
    try:
        assert p.contexts[0].icp_plane_weight()[0] == 0.0
    finally:
        p.close()


def test_a_template_that_is_no_lattice_is_refused(monkeypatch, tpl, frames4):
    eraser = pcd.read_xyz(os.path.join(GOLDEN, "eraser_ascii.pcd")).astype(np.float32)
    c = make_ctx(monkeypatch, {0: tpl, 1: eraser}, max_points=NPIX, max_frames=1)
    try:
        assert c.template_lattice_faces(1) == 0
        src = moved_subset(tpl, 200, 9)
        with pytest.raises(capi.CuboidError) as e:
            c.icp(1, src, capi.default_params())
        assert e.value.status == capi.CD_ERR_INVALID_ARG and "lattice" in str(e.value)
        prm = capi.default_params()
        for slot in (1, -1):   # the slot itself, and every loaded template
            prm.template_slot = slot
            with pytest.raises(capi.CuboidError) as e:
                c.process_batch(frames4[0][None], prm)
            assert e.value.status == capi.CD_ERR_INVALID_ARG and "lattice" in str(e.value)
            with pytest.raises(capi.CuboidError):
                c.process_frame(frames4[0], prm)
        prm.template_slot = 0   # the lattice slot alone is fine, and so is everything once the mode is off
        res, _, _ = c.process_batch(frames4[0][None], prm)
        assert res[0].status == capi.CD_OK
        c.set_icp_plane_weight(0)
        st, _, _ = c.icp(1, src, params(max_iter=2))
        assert st == capi.CD_OK
    finally:
        c.close()
