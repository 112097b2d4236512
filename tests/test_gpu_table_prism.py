"""The table prism (rule C20) on the GPU, bit for bit: cd_table_prism against the numpy specification
(perception_amd/table_prism.py) - kept indices, record and hull - and the fused call with the step on against the reference
composed on the CPU (tests/prism_reference.py) - records, clouds, labels, point labels, the step's records and hulls.  The
preconditions that make the fused scenarios show something are asserted on the CPU (tests/test_prism_reference_cpu.py)."""
import numpy as np
import pytest

import prism_reference as PR
import prism_scenarios as PS
from perception_amd import capi, synth, table_prism as TP

pytestmark = pytest.mark.gpu
FILTER = (16, 1.0)


# ---- cd_table_prism against the module ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx1():
    c = capi.Context(max_points=20480, max_frames=1)
    yield c
    c.close()


def same_as_module(ctx, c):
    o = TP.table_prism(c["plane"], c["coeff"], c["xyz"], *c["limits"])
    idx, stats, hull = ctx.table_prism(c["plane"], c["coeff"], c["xyz"], *c["limits"])
    print("n_plane %d n %d -> kept %d, hull %d, overflow %d" % (len(c["plane"]), len(c["xyz"]), stats["n_kept"], stats["hull_vertices"], stats["overflow"]))
    assert stats == o["stats"]
    assert idx.dtype == np.int32 and np.array_equal(idx, o["indices"])
    assert hull.dtype == np.int32 and np.array_equal(hull, o["hull"])
    return o


@pytest.mark.parametrize("name", sorted(PS.small_cases()))
def test_tiny_and_degenerate_sets(ctx1, name):
    same_as_module(ctx1, PS.small_cases()[name])       # ("no_object_point": n = 0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, 20000])
def test_small_range_grids(ctx1, n):
    """wave, workgroup and tile edges of the inlier passes; collinearity and duplicates everywhere"""
    o = same_as_module(ctx1, PS.grid_case(n, 40 + n))
    assert n < 64 or (o["stats"]["hull_vertices"] >= 4 and min(o["stats"][k] for k in ("n_kept", "n_below", "n_above", "n_outside")) > 0)


def test_wide_grid_fits_lds_after_pruning(ctx1):
    c = PS.wide_grid_case(20000, 2)
    assert TP.prune_survivors(TP.project(c["coeff"], c["plane"])[1]).sum() <= TP.LDS_POINTS
    o = same_as_module(ctx1, c)
    assert o["stats"]["hull_vertices"] > 8 and 0 < o["stats"]["n_kept"] < o["stats"]["n_before"]


@pytest.mark.parametrize("radius", [0.4, 0.05])
def test_circle_is_marched_in_global_memory(ctx1, radius):
    """5000 points on a circle: pruning removes (next to) nothing, the survivors exceed what the kernel stages in LDS.  At 0.4 m
    the integer hull has more than CD_PRISM_MAX_HULL vertices (overflow, by the rule); at 0.05 m it has some 550."""
    c = PS.circle_case(5000, radius)
    assert TP.prune_survivors(TP.project(c["coeff"], c["plane"])[1]).sum() > capi.CD_PRISM_LDS_POINTS
    o = same_as_module(ctx1, c)
    assert (o["stats"]["overflow"], o["stats"]["n_kept"]) == (1, 0) if radius == 0.4 else (o["stats"]["hull_vertices"] > 500 and o["stats"]["n_kept"] > 0)


@pytest.mark.parametrize("n", [1024, 1025])
def test_parabola_at_the_cap_and_beyond(ctx1, n):
    o = same_as_module(ctx1, PS.parabola_case(n))
    assert (o["stats"]["overflow"], o["stats"]["hull_vertices"]) == ((0, 1024) if n == 1024 else (1, 0))


def test_points_on_edges_and_vertices_and_a_tilted_plane(ctx1):
    o = same_as_module(ctx1, PS.edge_case())
    assert o["stats"]["n_kept"] == 15
    rng = np.random.RandomState(11)
    coeff = np.array([0.1, -0.7, -0.7, 0.5], np.float32)
    plane = (rng.uniform(-0.5, 0.5, (3000, 3)) + [0, 0.3, 0.4]).astype(np.float32)
    xyz = (rng.uniform(-0.6, 0.6, (1500, 3)) + [0, 0.3, 0.4]).astype(np.float32)
    xyz[7] = np.nan
    for cf in (coeff, -coeff):
        o = same_as_module(ctx1, dict(plane=plane, coeff=cf, xyz=xyz, limits=(-0.1, 0.2)))
        assert min(o["stats"][k] for k in ("n_kept", "n_below", "n_above", "n_outside")) > 0


def test_arguments(ctx1):
    c = PS.small_cases()["square"]
    for bad in ((0.1, 0.0), (float("nan"), 1.0), (0.0, float("inf"))):
        with pytest.raises(capi.CuboidError) as e:
            ctx1.table_prism(c["plane"], c["coeff"], c["xyz"], *bad)
        assert e.value.status == capi.CD_ERR_INVALID_ARG
        with pytest.raises(capi.CuboidError):
            ctx1.set_table_prism(True, *bad)
    assert ctx1.table_prism_setting() == (False, 0.0, 0.5)                 # a refused setting stays
    with pytest.raises(capi.CuboidError) as e:
        ctx1.table_prism(c["plane"], c["coeff"], c["xyz"], capacity=3)     # 7 are kept
    assert e.value.status == capi.CD_ERR_CAPACITY
    with pytest.raises(capi.CuboidError) as e:
        ctx1.table_prism(np.zeros((20481, 3), np.float32), c["coeff"], c["xyz"])
    assert e.value.status == capi.CD_ERR_CAPACITY
    ctx1.set_table_prism(True, -0.25, 0.75)
    assert ctx1.table_prism_setting() == (True, -0.25, 0.75)
    ctx1.set_table_prism(False)
    with pytest.raises(capi.CuboidError):
        ctx1.prism_stats(0)                                                # no fused call with the step


# ---- the fused call against the composed reference ----------------------------------------------------------------------------------
def make_ctx(template, N, F):
    c = capi.Context(max_points=N, max_frames=F)
    c.set_template(0, template)
    return c


def run(ctx, frames, prm, prism=None, filter=None, rects=None):
    """Sets the options, makes the call and reads back everything it leaves: plain arrays and bytes only."""
    frames = np.ascontiguousarray(np.stack(frames, 0))
    F = len(frames)
    ctx.set_table_prism(prism is not None, *(prism or (0.0, 0.5)))
    ctx.set_outlier_filter(*(filter or (0,)))
    ctx.set_frame_bboxes(rects)
    ctx.set_bbox_source(capi.CD_BBOX_PER_FRAME if rects is not None else capi.CD_BBOX_PARAMS)
    res, pi, lb = ctx.process_batch(frames, prm, want_indices=True)
    snap = dict(res=bytes(res), pi=pi.copy(), lb=lb.copy())
    snap["vox"] = [ctx.frame_cloud(f, capi.CD_CLOUD_VOXELS, 16, 12).copy() for f in range(F)]
    snap["obj"] = [ctx.frame_cloud(f, capi.CD_CLOUD_OBJECTS, 16, 12).copy() for f in range(F)]
    snap["clusters"] = [[bytes(c) for c in ctx.cluster_results(f)] for f in range(F)]
    snap["points"] = [[(ctx.cluster_points(f, k, aligned=False).copy(), ctx.cluster_points(f, k, aligned=True).copy())
                       for k in range(len(snap["clusters"][f]))] for f in range(F)]
    if prism is not None:
        snap["prism"] = [ctx.prism_stats(f) for f in range(F)]
        snap["hull"] = [ctx.prism_hull(f) for f in range(F)]
        with pytest.raises(capi.CuboidError):
            ctx.prism_stats(F)
    else:
        with pytest.raises(capi.CuboidError):
            ctx.prism_stats(0)
        with pytest.raises(capi.CuboidError):
            ctx.prism_hull(0)
        snap["prism"] = snap["hull"] = None
    snap["outlier"] = [ctx.outlier_stats(f) for f in range(F)] if filter is not None else None
    snap["point_labels"] = ctx.label_points_last(frames).copy()
    return snap


def same_snapshot(a, b):
    assert a["res"] == b["res"] and a["clusters"] == b["clusters"]
    for key in ("pi", "lb", "point_labels"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("vox", "obj"):
        assert len(a[key]) == len(b[key]) and all(np.array_equal(x, y) for x, y in zip(a[key], b[key])), key
    for pa, pb in zip(a["points"], b["points"]):
        assert len(pa) == len(pb) and all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(pa, pb))
    assert a["prism"] == b["prism"] and (a["hull"] is None) == (b["hull"] is None)
    if a["hull"] is not None:
        assert all(np.array_equal(x, y) for x, y in zip(a["hull"], b["hull"]))


def _bits(v):
    return int(np.float64(v).view(np.uint64))


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(snap, exp, where):
    """The snapshot of a call against the composed reference: everything prism_reference.expected returns."""
    res = (capi.CdFrameResult * len(exp)).from_buffer_copy(snap["res"])
    for f, e in enumerate(exp):
        r, w = res[f], "%s frame %d" % (where, f)
        n_plane, n_o, K = e["counts"][2], e["counts"][3], e["counts"][4]
        print(w, "counts", e["counts"], "prism", e["prism"])
        assert r.status == e["status"], w
        assert (r.n_cropped, r.n_voxels, r.n_plane, r.n_objects, r.n_clusters) == e["counts"], w
        assert (r.ransac_iterations, r.flags) == (e["ransac_iterations"], e["flags"]), w
        assert np.array_equal(_u32(list(r.plane)), _u32(e["plane"])), w
        assert np.array_equal(snap["pi"][f][:n_plane], e["plane_inliers"]) and (snap["pi"][f][n_plane:] == -1).all(), w
        assert np.array_equal(snap["lb"][f][:n_o], e["labels"]) and (snap["lb"][f][n_o:] == -1).all(), w
        assert np.array_equal(snap["vox"][f], e["voxels"]), w
        assert np.array_equal(snap["obj"][f], e["objects"]), w
        got = [capi.CdClusterResult.from_buffer_copy(b) for b in snap["clusters"][f]]
        assert len(got) == K == len(e["clusters"]), w
        for k, c in enumerate(e["clusters"]):
            g = got[k]
            assert (g.size, g.iterations, g.converged, g.accepted, g.template_slot, g.reserved) == (c.size, c.iterations, c.converged, c.accepted, c.slot, 0), (w, k)
            assert np.array_equal(_u32(list(g.T)), _u32(c.T).ravel()) and _bits(g.fitness) == _bits(c.fitness), (w, k)
            assert np.array_equal(np.array(list(g.pose), np.float64).view(np.uint64), np.asarray(c.pose, np.float64).view(np.uint64)), (w, k)
            if k < capi.CD_MAX_CLUSTERS_PER_FRAME:
                assert bytes(r.clusters[k]) == snap["clusters"][f][k], (w, k)
            orig, al = snap["points"][f][k]
            assert np.array_equal(_u32(orig[:, :3]), _u32(c.points)) and np.array_equal(_u32(al[:, :3]), _u32(c.aligned)), (w, k)
        if e["prism"] is not None:
            assert snap["prism"][f] == e["prism"], (w, snap["prism"][f], e["prism"])
            assert np.array_equal(snap["hull"][f], e["hull"]), w
        if e["outlier"] is not None:
            o, x = snap["outlier"][f], e["outlier"]
            assert (o["n_before"], o["n_removed"]) == (x["n_before"], x["n_removed"]), w
            assert [_bits(o[k]) for k in ("mean", "stddev", "threshold")] == [_bits(x[k]) for k in ("mean", "stddev", "threshold")], w
        assert np.array_equal(snap["point_labels"][f], e["point_labels"]), (w, "point labels", int((snap["point_labels"][f] != e["point_labels"]).sum()))


@pytest.fixture(scope="module")
def ctx8(template):
    c = make_ctx(template, synth.WIDTH * synth.HEIGHT, 8)
    yield c
    c.close()


def test_scenario_a_removes_nothing(ctx8, template):
    frames, prm, limits, keys = PS.scenario("a")
    exp = PR.expected(frames, prm, {0: template}, prism=limits, keys=keys)
    for lo in (0, 8):                                                    # two calls of eight frames
        on = run(ctx8, frames[lo:lo + 8], prm, prism=limits)
        check(on, exp[lo:lo + 8], "a[%d:]" % lo)
        assert all(s["n_kept"] == s["n_before"] for s in on["prism"])
    off = run(ctx8, frames[8:], prm)                                     # every record equals the step off
    for key in ("res", "clusters"):
        assert on[key] == off[key]
    assert np.array_equal(on["lb"], off["lb"]) and np.array_equal(on["point_labels"], off["point_labels"])
    assert all(np.array_equal(x, y) for x, y in zip(on["obj"], off["obj"]))


@pytest.mark.parametrize("name", ["b", "c"])
def test_scenarios_b_and_c(ctx8, template, name):
    frames, prm, limits, keys = PS.scenario(name)
    check(run(ctx8, frames, prm, prism=limits), PR.expected(frames, prm, {0: template}, prism=limits, keys=keys), name)


def test_step_together_with_the_outlier_filter(ctx8, template):
    frames, prm, limits, keys = PS.scenario("b")
    frames = frames + PS.scenario("c")[0][1:2]
    prm = PS.finite_table_params()
    prm.rgb_offset = 12
    exp = PR.expected(frames, prm, {0: template}, prism=(0.0, 0.04), filter=FILTER)
    assert all(e["prism"]["n_above"] > 1000 for e in exp[:3]) and exp[3]["prism"]["n_kept"] == exp[3]["prism"]["n_before"]
    assert all(e["outlier"]["n_removed"] > 0 and e["outlier"]["n_before"] == e["prism"]["n_kept"] for e in exp)
    check(run(ctx8, frames, prm, prism=(0.0, 0.04), filter=FILTER), exp, "prism + filter")


def test_step_together_with_per_frame_gate_rectangles(ctx8, template):
    frames = PS.scenario("b")[0][:2] + PS.scenario("c")[0][1:3]
    prm = PS.finite_table_params()
    prm.rgb_offset = 12
    fx, fy, cx, cy = synth.depth_camera_params()
    prm.bbox_enable = 1
    prm.bbox_P[:] = [fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1, 0]
    rects = np.array([[0, 0, synth.WIDTH, synth.HEIGHT], [150, 100, 640, 400], [250, 150, 420, 330], [0, 0, 1, 1]], np.int32)
    exp = PR.expected(frames, prm, {0: template}, prism=(0.0, 0.5), rects=rects)
    assert exp[0]["prism"]["n_outside"] > 0 and exp[3]["prism"]["n_before"] == 0 and exp[2]["prism"]["n_kept"] > 0
    check(run(ctx8, frames, prm, prism=(0.0, 0.5), rects=rects), exp, "prism + rects")


def test_batch_with_an_all_nan_frame_at_exactly_the_contexts_capacity(template):
    """an all-NaN frame and a frame without a plane among normal ones; the context holds exactly this batch, scene (b) last"""
    N = synth.WIDTH * synth.HEIGHT
    allnan = np.full((N, 4), np.nan, np.float32)
    allnan[:, 3] = 0.0
    noplane = allnan.copy()
    noplane[1000, :3] = (0.01, 0.02, 0.5)
    noplane[2000, :3] = (-0.05, 0.03, 0.6)
    frames = [PS.scenario("c")[0][1], allnan, noplane, PS.scenario("b")[0][2]]
    prm = PS.finite_table_params()
    prm.rgb_offset = 12
    exp = PR.expected(frames, prm, {0: template}, prism=(0.0, 0.5))
    assert exp[1]["counts"][1] == 0 and exp[2]["status"] == capi.CD_ERR_NO_MODEL and exp[2]["prism"]["n_kept"] == exp[2]["prism"]["n_before"] == 2
    assert exp[3]["counts"][4] == 1 and exp[3]["prism"]["n_outside"] > 1000
    ctx = make_ctx(template, N, len(frames))
    try:
        check(run(ctx, frames, prm, prism=(0.0, 0.5)), exp, "mixed")
    finally:
        ctx.close()


def test_one_context_through_on_off_on(ctx8, template):
    frames, prm, limits, _ = PS.scenario("b")
    fresh = make_ctx(template, synth.WIDTH * synth.HEIGHT, len(frames))
    try:
        never = run(fresh, frames, prm)
    finally:
        fresh.close()
    on = run(ctx8, frames, prm, prism=limits)
    off = run(ctx8, frames, prm)                 # (run() asserts that cd_get_prism_stats and cd_get_prism_hull refuse)
    same_snapshot(off, never)
    same_snapshot(run(ctx8, frames, prm, prism=limits), on)
    assert on["res"] != off["res"]
    ctx8.table_prism(np.zeros((3, 3), np.float32), PS.COEFF_Z, np.zeros((1, 3), np.float32))
    with pytest.raises(capi.CuboidError):        # another compute call invalidates the records with the other read-backs
        ctx8.prism_stats(0)
    ctx8.set_table_prism(False)
