"""The box fit (rule C24) on the GPU, bit for bit: cd_box_fit_points against the numpy specification (perception_amd/box_fit.py) at
every size and shape where k_box_fit takes another path, and the fused call with the step on against the reference composed on
the CPU (tests/box_fit_reference.py).  The preconditions that make the scenarios show something are asserted on the CPU
(tests/test_box_fit_cpu.py)."""
import functools

import numpy as np
import pytest

import box_fit_reference as BR
import box_fit_scenarios as S
from perception_amd import box_fit as BF, capi, synth

pytestmark = pytest.mark.gpu
ENV_KEYS = ("CUBOID_ICP_LATTICE", "CUBOID_ICP_MODE", "CUBOID_ICP_PERSIST", "CUBOID_ICP_MAX_WG")
FILTER = (16, 1.0)
PRISM = (0.0, 0.5)


# ---- cd_box_fit_points against the module ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx1():
    c = capi.Context(max_points=8192, max_frames=1)
    yield c
    c.close()


def against_module(ctx, names):
    cases = [S.kernel_cases()[k] for k in names]
    band = cases[0][2]
    assert all(c[2] == band for c in cases)
    got = ctx.box_fit_points([c[0] for c in cases], [c[1] for c in cases], band)
    assert len(got) == len(cases)
    for name, g, c in zip(names, got, cases):
        want = BF.box_fit(c[0], c[1], band)
        print("%s: n %d status %d n_top %d hull %d edge %d" % (name, g["n"], g["status"], g["n_top"], g["hull_vertices"], g["edge"]))
        assert S.same_record(g, want) == [], name
    return got


@pytest.mark.parametrize("name", sorted(S.kernel_cases()))
def test_every_path_of_the_kernel(ctx1, name):
    """n = 3, 63, 64, 65 (the switch of k), the LDS cap and cap + 1, a top set of 3 points, a collinear one, hulls of 3, 4, 656
    (more edges than threads), CD_PRISM_MAX_HULL and one more, duplicates, a qh exactly on href - band, the known answers, every
    status."""
    against_module(ctx1, [name])


def test_sets_with_different_planes_in_one_launch(ctx1):
    names = ["known_rect_345", "known_axis_x", "random_1", "two_points", "known_d_negative", "top_collinear", "random_2", "known_axis_y", "no_plane"]
    got = against_module(ctx1, names)
    assert [g["status"] for g in got] == [0, 0, 0, capi.CD_ERR_FEW_CORRESPONDENCES, 0, capi.CD_ERR_NO_MODEL, 0, 0, capi.CD_ERR_NO_MODEL]
    # a window of a longer array: offsets that do not start at 0
    co, xyz, band = S.kernel_cases()["random_3"]
    lib, out = ctx1.lib, (capi.CdBoxFit * 1)()
    pts = np.ascontiguousarray(np.r_[np.full((11, 3), np.nan, np.float32), xyz])
    off = np.array([11, 11 + len(xyz)], np.int32)
    import ctypes as C
    assert lib.cd_box_fit_points(ctx1.h, capi._ptr(np.ascontiguousarray(co)), capi._ptr(pts), 12, off.ctypes.data_as(C.POINTER(C.c_int32)), 1, band, out) == capi.CD_OK
    assert S.same_record(out[0].as_dict(), BF.box_fit(co, xyz, band)) == []


@pytest.mark.parametrize("max_wg", ["1", "2"])
def test_many_sets_on_few_workgroups(monkeypatch, max_wg):
    """CUBOID_ICP_MAX_WG caps the kernel's grid: a workgroup goes round its loop many times - histogram, sums, hull and the queue word
    set up again - through clusters in LDS, clusters beyond the cap and every early exit, in the queue's order (largest first)."""
    monkeypatch.setenv("CUBOID_ICP_MAX_WG", max_wg)
    c = capi.Context(max_points=8192, max_frames=1)
    monkeypatch.delenv("CUBOID_ICP_MAX_WG")
    try:
        names = [k for k in sorted(S.kernel_cases()) if S.kernel_cases()[k][2] == BF.BAND_DEFAULT]
        assert len(names) >= 16 * int(max_wg)
        got = against_module(c, names + names[::-1])
        assert len({g["status"] for g in got}) == 5
    finally:
        c.close()


def test_arguments_and_setting(ctx1):
    co, xyz, band = S.kernel_cases()["hull_4"]
    for bad in (0.0, -0.006, float("nan"), float("inf"), 65.0):
        with pytest.raises(capi.CuboidError) as e:
            ctx1.box_fit_points([co], [xyz], bad)
        assert e.value.status == capi.CD_ERR_INVALID_ARG
        with pytest.raises(capi.CuboidError):
            ctx1.set_box_fit(True, bad)
    assert ctx1.box_fit_setting() == (0, capi.CD_BOX_FIT_BAND_DEFAULT)
    ctx1.set_box_fit(True, 0.01)
    assert ctx1.box_fit_setting() == (1, 0.01)
    ctx1.set_box_fit(False, float("nan"))                                  # off: the band is not looked at and stays
    assert ctx1.box_fit_setting() == (0, 0.01)
    with pytest.raises(capi.CuboidError):
        ctx1.cluster_box_fits(0)                                           # no fused call with the step


# ---- the fused call against the composed reference ----------------------------------------------------------------------------------
def make_ctx(monkeypatch, template, N, F):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    c = capi.Context(max_points=N, max_frames=F)
    c.set_template(0, template)
    return c


def snapshot(ctx, F, res, pi, lb):
    """Everything a fused call leaves besides the box records: plain bytes and arrays."""
    snap = dict(res=bytes(res), pi=pi.copy(), lb=lb.copy())
    snap["clusters"] = [[bytes(c) for c in ctx.cluster_results(f)] for f in range(F)]
    snap["points"] = [[(ctx.cluster_points(f, k, aligned=False).copy(), ctx.cluster_points(f, k, aligned=True).copy())
                       for k in range(len(snap["clusters"][f]))] for f in range(F)]
    snap["obj"] = [ctx.frame_cloud(f, capi.CD_CLOUD_OBJECTS, 16, 12).copy() for f in range(F)]
    return snap


def same_snapshot(a, b):
    assert a["res"] == b["res"] and np.array_equal(a["pi"], b["pi"]) and np.array_equal(a["lb"], b["lb"]) and a["clusters"] == b["clusters"]
    for x, y in zip(a["obj"], b["obj"]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for fa, fb in zip(a["points"], b["points"]):
        assert len(fa) == len(fb)
        for (p0, p1), (q0, q1) in zip(fa, fb):
            assert np.array_equal(p0.view(np.uint32), q0.view(np.uint32)) and np.array_equal(p1.view(np.uint32), q1.view(np.uint32))


def check_fits(ctx, exp, res):
    n_ok = 0
    for f, e in enumerate(exp):
        assert (res[f].status, res[f].n_plane, res[f].n_objects, res[f].n_clusters) == (e["status"], e["counts"][2], e["counts"][3], e["counts"][4]), f
        got = [r.as_dict() for r in ctx.cluster_box_fits(f)]
        assert len(got) == len(e["box_fits"]) == e["counts"][4], f
        for k, want in enumerate(e["box_fits"]):
            assert np.array_equal(ctx.cluster_points(f, k)[:, :3].view(np.uint32), e["clusters"][k].points.view(np.uint32)), (f, k)
            assert S.same_record(got[k], want) == [], (f, k)
            n_ok += want["status"] == capi.CD_OK
    with pytest.raises(capi.CuboidError):
        ctx.cluster_box_fits(len(exp))
    return n_ok


@functools.lru_cache(maxsize=None)
def frames03():
    return np.ascontiguousarray(np.stack([synth.frame(i) for i in range(4)]))


def params():
    prm = capi.default_params()
    prm.rgb_offset = 12
    return prm


@pytest.mark.parametrize("prism,filter", [(None, None), (PRISM, None), (None, FILTER), (PRISM, FILTER)], ids=["plain", "prism", "filter", "prism+filter"])
def test_fused_cloud_call(monkeypatch, template, prism, filter):
    """Synth frames 0..3 as clouds: the records are the module's on the clusters as clustered - after the table prism and the outlier
    filter when those are on; with the step on every other output is byte for byte what it is with the step off; off, the read-back
    refuses; a context that set and cleared the setting returns the bytes of one that never touched it."""
    frames, prm = frames03(), params()
    exp = BR.expected(list(frames), prm, {0: template}, prism=prism, filter=filter, keys=[("synth", i) for i in range(4)])
    c = make_ctx(monkeypatch, template, frames.shape[1], 4)
    try:
        c.set_table_prism(prism is not None, *(prism or PRISM))
        c.set_outlier_filter(*(filter or (0,)))
        never = snapshot(c, 4, *c.process_batch(frames, prm, want_indices=True))
        c.set_box_fit(True)
        res, pi, lb = c.process_batch(frames, prm, want_indices=True)
        assert check_fits(c, exp, res) >= 4
        on = snapshot(c, 4, res, pi, lb)
        same_snapshot(on, never)
        part = [r.as_dict() for r in c.cluster_box_fits(0, first=0, count=1)]
        assert len(part) == 1 and S.same_record(part[0], exp[0]["box_fits"][0]) == []
        c.set_box_fit(False)
        off = snapshot(c, 4, *c.process_batch(frames, prm, want_indices=True))
        same_snapshot(off, never)
        with pytest.raises(capi.CuboidError) as e:
            c.cluster_box_fits(0)
        assert e.value.status == capi.CD_ERR_INVALID_ARG
        c.set_box_fit(True, 0.004)                                          # another band, and another compute call invalidates
        res, _, _ = c.process_batch(frames, prm)
        for f, e in enumerate(exp):
            e4 = BR.fits_of(e, 0.004)
            got = [r.as_dict() for r in c.cluster_box_fits(f)]
            assert len(got) == len(e4) and all(S.same_record(g, w) == [] for g, w in zip(got, e4))
        c.icp(0, exp[0]["clusters"][0].points, prm)
        with pytest.raises(capi.CuboidError):
            c.cluster_box_fits(0)
    finally:
        c.close()


def test_fused_depth_call(monkeypatch, template):
    pairs = [synth.depth_frame(i) for i in range(4)]
    depth = np.ascontiguousarray(np.stack([p[0] for p in pairs]))
    color = np.ascontiguousarray(np.stack([p[1] for p in pairs]))
    cam = capi.default_depth_camera()
    cam.width, cam.height = synth.WIDTH, synth.HEIGHT
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params()
    cam.depth_scale = synth.DEPTH_SCALE
    cam.color = capi.CD_COLOR_RGB8
    prm = params()
    exp = BR.expected_depth(depth, color, cam, prm, {0: template})
    c = make_ctx(monkeypatch, template, synth.WIDTH * synth.HEIGHT, 4)
    try:
        c.set_box_fit(True)
        res, _, _ = c.process_depth_batch(depth, color, cam, prm)
        assert check_fits(c, exp, res) >= 4
    finally:
        c.close()


def test_fused_frame_without_a_plane_and_clusters_beyond_the_record(monkeypatch, template):
    """Frame 0: all NaN - no plane, no cluster, no record.  Frame 1: twelve small cuboids - more clusters than the
    CD_MAX_CLUSTERS_PER_FRAME slots of a frame record (a second extraction round); every one has its box record."""
    grid = synth.render(synth.scene_grid(3))
    nan = np.full_like(grid, np.nan)
    frames = np.ascontiguousarray(np.stack([nan, grid]))
    prm = params()
    exp = BR.expected(list(frames), prm, {0: template})
    K = exp[1]["counts"][4]
    assert exp[0]["counts"][4] == 0 and exp[0]["status"] != capi.CD_OK and K > capi.CD_MAX_CLUSTERS_PER_FRAME
    c = make_ctx(monkeypatch, template, frames.shape[1], 2)
    try:
        c.set_box_fit(True)
        res, _, _ = c.process_batch(frames, prm)
        assert check_fits(c, exp, res) > capi.CD_MAX_CLUSTERS_PER_FRAME
        assert c.cluster_box_fits(0) == [] and c.cluster_box_fits(1, first=K) == []
        tail = [r.as_dict() for r in c.cluster_box_fits(1, first=capi.CD_MAX_CLUSTERS_PER_FRAME, count=3)]
        assert len(tail) == min(3, K - capi.CD_MAX_CLUSTERS_PER_FRAME) and all(S.same_record(g, w) == [] for g, w in zip(tail, exp[1]["box_fits"][capi.CD_MAX_CLUSTERS_PER_FRAME:]))
    finally:
        c.close()


# ---- the selection ---------------------------------------------------------------------------------------------------------------------
CONFIG5 = np.array([d[:3] for d in synth.CONFIG5_DIMS], np.float64)
TOLERANCE = 0.0125


@functools.lru_cache(maxsize=None)
def config5_case():
    """(frame, templates by slot, the composed reference at TOLERANCE) of config-5 scene 0 at 640 x 480.  Read only."""
    from perception_amd import templates
    frame = synth.render(synth.scene_config5(0), width=640, height=480)
    tpls = {s: templates.template_xyz32(L, W, H, d) for s, (L, W, H, d) in enumerate(synth.CONFIG5_DIMS)}
    return frame, tpls, BR.expected_selection(frame, S.config5_prm(), tpls, CONFIG5, TOLERANCE)


def same_result(got, want):
    return (got.size, got.iterations, got.converged, got.accepted, got.fitness, list(got.T)) == \
        (want.size, want.iterations, want.converged, want.accepted, want.fitness, list(want.T))


def pair_tests(ctx):
    t = ctx.timing()
    return (t.icp_pair_tests_hi << 32) | (t.icp_pair_tests_lo & 0xffffffff)


def test_selection_registers_each_cluster_against_its_matched_slot(monkeypatch):
    """One config-5 scene, five templates, template_slot = -1.  The records' template_slot are the matched slots; each result is,
    byte for byte, what the single-slot call gives that cluster (and the oracle's bits); the call makes fewer ICP pair tests than
    the all-pairs call; a tolerance of 1e-6 matches nothing and is the all-pairs call byte for byte; a context that set and
    cleared both settings returns the bytes of one that never touched them."""
    frame, tpls, exp = config5_case()
    assert len(exp) == 5 and all(e["box"]["match_slot"] >= 0 for e in exp) and sorted(e["slot"] for e in exp) == [0, 1, 2, 3, 4]
    assert any(e["slot"] != e["all_pairs_slot"] for e in exp)                    # the selection changes what the call reports
    prm = S.config5_prm()
    prm.template_slot = -1
    frames = np.ascontiguousarray(frame[None])
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    c = capi.Context(max_points=frames.shape[1], max_frames=1)
    try:
        for s, t in tpls.items():
            c.set_template(s, t)
        with pytest.raises(capi.CuboidError) as e:
            c.set_box_select(True, CONFIG5, TOLERANCE)                            # needs the box fit on
        assert e.value.status == capi.CD_ERR_INVALID_ARG and c.box_select_setting()[0] == 0
        never = snapshot(c, 1, *c.process_batch(frames, prm, want_indices=True))
        all_pairs = pair_tests(c)
        for k, e in enumerate(exp):                                               # the all-pairs call keeps the lowest fitness
            assert c.cluster_results(0)[k].template_slot == e["all_pairs_slot"] and same_result(c.cluster_results(0)[k], e["all_pairs_result"]), k
        single = {}
        for s in tpls:                                                            # the single-slot calls
            prm.template_slot = s
            c.process_batch(frames, prm)
            single[s] = [bytes(r) for r in c.cluster_results(0)]
        prm.template_slot = -1
        c.set_box_fit(True)
        c.set_box_select(True, CONFIG5, TOLERANCE)
        on, sd, tol = c.box_select_setting()
        assert on == 1 and tol == TOLERANCE and np.array_equal(sd[:5], CONFIG5) and not sd[5:].any()
        res, _, _ = c.process_batch(frames, prm)
        selected = pair_tests(c)
        got, boxes = c.cluster_results(0), [r.as_dict() for r in c.cluster_box_fits(0)]
        assert res[0].n_clusters == len(got) == len(boxes) == 5
        for k, e in enumerate(exp):
            assert S.same_record(boxes[k], e["box"]) == [], k
            assert got[k].template_slot == e["slot"] == boxes[k]["match_slot"], k
            assert bytes(got[k]) == single[e["slot"]][k] and same_result(got[k], e["result"]), k
            assert bytes(res[0].clusters[k]) == bytes(got[k]), k
        print("ICP pair tests: all pairs %d, selected %d" % (all_pairs, selected))
        assert 0 < selected < all_pairs
        prm.template_slot = 3                                                     # a single-slot call: the selection does not act
        c.process_batch(frames, prm)
        assert [bytes(r) for r in c.cluster_results(0)] == single[3] and all(r.match_slot >= 0 for r in c.cluster_box_fits(0))
        prm.template_slot = -1
        c.set_box_select(True, CONFIG5, 1e-6)                                     # nothing matches: the all-pairs call
        tight = snapshot(c, 1, *c.process_batch(frames, prm, want_indices=True))
        same_snapshot(tight, never)
        assert pair_tests(c) == all_pairs and all(r.match_slot == -1 and r.match_cost > 1e-6 for r in c.cluster_box_fits(0))
        c.set_box_select(False)
        c.set_box_fit(False)
        assert c.box_select_setting()[0] == 0 and c.box_fit_setting()[0] == 0
        cleared = snapshot(c, 1, *c.process_batch(frames, prm, want_indices=True))
        same_snapshot(cleared, never)
        with pytest.raises(capi.CuboidError):
            c.cluster_box_fits(0)
        c.set_box_fit(True)
        c.set_box_select(True, CONFIG5, TOLERANCE)
        c.set_box_fit(False)                                                      # the selection goes off with the step
        assert c.box_select_setting()[0] == 0
    finally:
        c.close()
