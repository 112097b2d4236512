"""The fused call with its opt-in steps combined - the outlier filter (C16), the plane-weighted ICP (C17), the correspondence bound
(C8), every guess mode, template_slot = -1, depth input and the per-frame gate - against the reference composed on the CPU
(tests/fused_reference.py), bit for bit: no tolerance, nothing left out of a comparison.

  a. an option table in which every pair of option values the reference can express occurs, one fresh context per row;
  b. ICP stops inside a batch (a singular step, too few correspondences) and the pairs a workgroup runs after them;
  c. clusters of one and two points next to a real one;
  d. the one-pass-per-template fallback with the filter and C17 on;
  e. one context through a sequence of settings, every call equal to its fresh-context result.

Everything above the first test is plain CPU code: tests/test_fused_reference_cpu.py imports the scenarios and asserts, from the
reference alone, every precondition that makes a scenario show something."""
import collections
import functools

import numpy as np
import pytest

import fused_reference as FR
from perception_amd import capi, cluster_frame as cf, synth, templates

pytestmark = pytest.mark.gpu

W, H = synth.WIDTH, synth.HEIGHT
W0, D0 = capi.CD_ICP_PLANE_WEIGHT_DEFAULT, capi.CD_ICP_PLANE_SWITCH_DEFAULT
INF = float("inf")
FILTER = (16, 1.0)
SURFACE_THR = 0.004
ENV_KEYS = ("CUBOID_ICP_LATTICE", "CUBOID_ICP_MODE", "CUBOID_ICP_PERSIST", "CUBOID_ICP_MAX_WG")

# ---- a. the option table -----------------------------------------------------------------------------------------------------------
# filter: off / (16, 1.0).  plane: off / (default, default) / (default, inf).  bound: none / a distance in metres - 0.01 where a
# guess has brought the clusters onto the template (a box's far points are more than 1 cm from a template smaller than the box),
# 0.55 without a guess (the clusters lie 0.5 .. 0.6 m from the origin, where the template is).  guess: none / per_frame / cluster /
# surface.  slot: 0 / -1.  depth: point records / depth + colour images.  gate: off / per-frame rectangles.
# The bound needs C17 (fused_reference's docstring); with that, every pair of values occurs in a row (asserted on the CPU).
Row = collections.namedtuple("Row", "id filter plane bound guess slot depth gate")
TABLE = (
    Row("r00", FILTER, None, None, "none", -1, True, True),
    Row("r01", None, None, None, "per_frame", 0, True, False),
    Row("r02", None, None, None, "cluster", 0, False, True),
    Row("r03", FILTER, None, None, "surface", -1, False, False),
    Row("r04", FILTER, (W0, D0), 0.55, "none", 0, False, False),
    Row("r05", None, (W0, D0), 0.01, "per_frame", -1, True, True),
    Row("r06", FILTER, (W0, D0), 0.01, "cluster", -1, True, False),
    Row("r07", FILTER, (W0, D0), None, "surface", 0, True, True),
    Row("r08", None, (W0, INF), None, "none", 0, True, False),
    Row("r09", FILTER, (W0, INF), 0.01, "per_frame", -1, False, True),
    Row("r10", None, (W0, INF), None, "cluster", -1, True, True),
    Row("r11", None, (W0, INF), 0.01, "surface", -1, False, True),
)
ROWS = {r.id: r for r in TABLE}
RECTS = np.array([[180, 100, 420, 380], [0, 0, W, H], [250, 150, 420, 330], [0, 0, W, H], [0, 0, 1, 1]], np.int32)
SEQUENCE = ("r09", "r00", "r10", "stops", "r04", "r11", "r01")   # (e): every option on, off and on again


class Case(object):
    """One fused call: its input, parameters, templates and options, and how to read it back."""

    def __init__(self, id, frames, prm, tpls, opt, depth=None, rgb=-1, last_slot_resident=False):
        self.id, self.frames, self.prm, self.tpls, self.opt, self.depth, self.rgb = id, frames, prm, tpls, opt, depth, rgb
        self.last_slot_resident = last_slot_resident    # (d): one ICP pass per template, only the last slot's aligned points stay
        self.N = frames.shape[1]
        self.F = frames.shape[0]

    @functools.lru_cache(maxsize=None)
    def expected(self):
        return FR.expected(self.depth if self.depth is not None else self.frames, self.prm, self.tpls, self.opt)

    def records(self):
        """The point records of the call (a depth call: the records its images deproject to)."""
        if self.depth is None:
            return self.frames
        return np.ascontiguousarray(np.stack([e["records"] for e in self.expected()]))


@functools.lru_cache(maxsize=None)
def small_templates():
    return {0: templates.template_xyz32(0.05, 0.05, 0.03, 0.002), 1: templates.template_xyz32(0.06, 0.04, 0.02, 0.002)}


@functools.lru_cache(maxsize=None)
def table_batch():
    """The five frames of the table: 12 clusters (more than a record holds), two boxes, flying pixels, no object, no plane."""
    noplane = np.full((W * H, 4), np.nan, np.float32)
    noplane[:, 3] = 0.0
    noplane[1000, :3] = (0.01, 0.02, 0.5)
    noplane[2000, :3] = (-0.05, 0.03, 0.6)
    frames = [synth.render(synth.scene_grid(3)), synth.frame(1), synth.flying_pixels(synth.frame(0), W, H, seed=7, frac=0.5),
              synth.frame(4, k_obj=0), noplane]
    return np.ascontiguousarray(np.stack(frames, 0))


@functools.lru_cache(maxsize=None)
def table_depth():
    pairs = [FR.depth_of_records(fr, H, W) for fr in table_batch()]
    return np.ascontiguousarray(np.stack([p[0] for p in pairs])), np.ascontiguousarray(np.stack([p[1] for p in pairs]))


def camera():
    cam = capi.default_depth_camera()
    cam.width, cam.height = W, H
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params()
    cam.depth_scale = synth.DEPTH_SCALE
    cam.color = capi.CD_COLOR_RGB8
    return cam


def first_cluster_guesses(frames, prm, tpl):
    """A guess per frame: rule C13's guess of the frame's first cluster (no filter, no gate) against tpl; identity without one."""
    from oracle import oracle_py as O
    t_rec = cf.shape_frame(tpl)
    out = []
    q = FR.copy_params(prm)
    q.bbox_enable = 0
    q.icp_max_iterations = 1
    for fr in frames:
        o = O.process_frame(fr, q, tpl, want_clouds=True)
        g = FR.IDENT
        if o["result"].n_clusters > 0:
            g = cf.guess(cf.shape_frame(o["objects"][o["labels"] == 0]), t_rec)[0]
        out.append(np.asarray(g, np.float32))
    return np.stack(out)


def table_params():
    prm = capi.default_params()
    prm.cluster_min_size = 60
    prm.icp_max_iterations = 8
    prm.rgb_offset = 12
    return prm


@functools.lru_cache(maxsize=None)
def table_guesses():
    return first_cluster_guesses(table_batch(), table_params(), small_templates()[0])


@functools.lru_cache(maxsize=None)
def table_case(row_id):
    row = ROWS[row_id]
    prm = table_params()
    prm.template_slot = row.slot
    prm.icp_use_guess = FR.GUESS_MODES[row.guess]
    if row.gate:
        fx, fy, cx, cy = synth.depth_camera_params()
        prm.bbox_enable = 1
        prm.bbox_P[:] = [fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1, 0]
    opt = FR.options(filter=row.filter, plane=row.plane, bound=row.bound, guess=row.guess,
                     frame_guesses=table_guesses() if row.guess == "per_frame" else None, surface_threshold=SURFACE_THR,
                     rects=RECTS if row.gate else None, cam=camera() if row.depth else None)
    return Case(row.id, table_batch(), prm, small_templates(), opt, depth=table_depth() if row.depth else None, rgb=12)


# ---- b. stops inside a batch -------------------------------------------------------------------------------------------------------
SW, SH = 128, 96     # the grid scene at this size has clusters of fewer points than the line's 41: pairs that run after its stop
LINE_FRAME = 1
IDENTITY_FRAME = 2


@functools.lru_cache(maxsize=None)
def stop_batch():
    """An ordinary frame, the line frame (a 4 mm grid plane patch at z = 0.75 and 41 points on a line parallel to the template's
    bottom face, coordinates on a 2^-7 grid: every term of the step's system is exact, so it is exactly singular), an ordinary
    frame that is given the identity as its guess, the first frame again."""
    grid = synth.render(synth.scene_grid(3), width=SW, height=SH)
    gx, gy = np.meshgrid(np.arange(-0.19, 0.19, 0.004), np.arange(-0.14, 0.14, 0.004))
    patch = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.75)], 1)
    k = np.arange(-20, 21, dtype=np.float64)
    line = np.stack([k * 2.0 ** -7, np.full(41, 2.0 ** -6), np.full(41, 0.5)], 1)
    lf = np.full((SW * SH, 4), np.nan, np.float32)
    lf[:, 3] = 0.0
    lf[:len(patch) + 41, :3] = np.concatenate([patch, line]).astype(np.float32)
    return np.ascontiguousarray(np.stack([grid, lf, synth.frame(1, width=SW, height=SH), grid], 0))


@functools.lru_cache(maxsize=None)
def stop_case(kind):
    """kind: "unbounded", "bounded" (0.1 m) or "slots" (unbounded, template_slot = -1)."""
    prm = capi.default_params()
    prm.cluster_min_size = 30
    prm.icp_max_iterations = 8
    prm.template_slot = -1 if kind == "slots" else 0
    prm.icp_use_guess = capi.CD_GUESS_PER_FRAME
    frames = stop_batch()
    g = first_cluster_guesses(frames, prm, small_templates()[0])
    g[LINE_FRAME] = FR.IDENT
    g[LINE_FRAME][2, 3] = -(0.5 + 2.0 ** -6)
    g[IDENTITY_FRAME] = FR.IDENT
    opt = FR.options(plane=(W0, D0), bound=0.1 if kind == "bounded" else None, guess="per_frame", frame_guesses=g)
    return Case("stops-" + kind, frames, prm, small_templates(), opt)


# ---- c. tiny clusters --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiny_cloud():
    """A plane, a real cluster (a box top of 12 x 10 points), five single points and four pairs, each further than the cluster
    tolerance (0.02) from everything else; the points of a pair are 0.012 apart: two voxels of the 5 mm grid, one cluster."""
    gx, gy = np.meshgrid(np.arange(-0.19, 0.19, 0.004), np.arange(-0.14, 0.14, 0.004))
    plane = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.7)], 1)
    bx, by = np.meshgrid(np.arange(12) * 0.006 - 0.15, np.arange(10) * 0.006 - 0.1)
    box = np.stack([bx.ravel(), by.ravel(), np.full(bx.size, 0.5) + 0.0007 * bx.ravel()], 1)
    singles = [(-0.02 + 0.04 * i, 0.06, 0.5 + 0.01 * i) for i in range(5)]
    pairs = []
    for i in range(4):
        pairs += [(-0.02 + 0.05 * i, -0.03, 0.45), (-0.02 + 0.05 * i + 0.012, -0.03, 0.45)]
    cloud = np.concatenate([plane, box, np.array(singles), np.array(pairs)]).astype(np.float32)
    return np.ascontiguousarray(np.c_[cloud, np.zeros(len(cloud), np.float32)][None])


@functools.lru_cache(maxsize=None)
def tiny_case(plane_on):
    prm = capi.default_params()
    prm.cluster_min_size = 1
    prm.icp_max_iterations = 8
    return Case("tiny-%d" % plane_on, tiny_cloud(), prm, {0: small_templates()[0]}, FR.options(plane=(W0, D0) if plane_on else None))


# ---- d. the per-template fallback --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fallback_case():
    """Three dense balls that are over half of the frame's points (tests/test_gpu_many_clusters.py): two copies of the ICP
    sources do not fit the frame's segment, so template_slot = -1 runs one ICP pass per template."""
    rng = np.random.default_rng(12)
    plane = np.c_[rng.uniform(-0.19, 0.19, (1500, 2)), np.full(1500, 0.6)]
    balls = []
    for cx in (-0.12, 0.0, 0.12):
        d = rng.normal(size=(1400, 3))
        d *= (0.04 * rng.uniform(0, 1, (1400, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        balls.append(d + [cx, 0.0, 0.5])
    cloud = np.concatenate([plane] + balls).astype(np.float32)
    cloud = np.c_[cloud, np.zeros(len(cloud), np.float32)]
    prm = capi.default_params()
    prm.leaf_size = 0.002
    prm.plane_distance_threshold = 0.01
    prm.cluster_min_size = 100
    prm.icp_max_iterations = 6
    prm.template_slot = -1
    # (the filter at 2 sigma: at 1 sigma it takes a fifth of a uniform ball and the rest no longer is half of the frame)
    return Case("fallback", np.ascontiguousarray(cloud[None]), prm, small_templates(), FR.options(filter=(16, 2.0), plane=(W0, D0)),
                last_slot_resident=True)


# ---- running a case and comparing it -----------------------------------------------------------------------------------------------
def make_ctx(monkeypatch, N, F, tpls, env=None):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    c = capi.Context(max_points=N, max_frames=F)
    for slot, t in tpls.items():
        c.set_template(slot, t)
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    return c


def run(ctx, case):
    """Sets every option of the case on the context (so that a context can go from any case to any other), makes the call and
    reads back everything it leaves.  Returns the snapshot: plain arrays and bytes only."""
    opt = case.opt
    ctx.set_outlier_filter(*(opt["filter"] or (0,)))
    ctx.set_icp_plane_weight(*(opt["plane"] or (None,)))
    ctx.set_icp_max_correspondence_distance(opt["bound"])
    ctx.set_surface_distance_threshold(opt["surface_threshold"])
    ctx.set_frame_guesses(opt["frame_guesses"])
    ctx.set_frame_bboxes(opt["rects"])
    ctx.set_bbox_source(capi.CD_BBOX_PER_FRAME if opt["rects"] is not None else capi.CD_BBOX_PARAMS)
    if case.depth is not None:
        res, pi, lb = ctx.process_depth_batch(case.depth[0], case.depth[1], opt["cam"], case.prm, want_indices=True)
    else:
        res, pi, lb = ctx.process_batch(case.frames, case.prm, want_indices=True)
    F = case.F
    snap = dict(res=bytes(res), pi=pi.copy(), lb=lb.copy(), regime=ctx.timing().icp_regime)
    snap["vox"] = [ctx.frame_cloud(f, capi.CD_CLOUD_VOXELS, 16, case.rgb).copy() for f in range(F)]
    snap["obj"] = [ctx.frame_cloud(f, capi.CD_CLOUD_OBJECTS, 16, case.rgb).copy() for f in range(F)]
    snap["clusters"] = [[bytes(c) for c in ctx.cluster_results(f)] for f in range(F)]
    snap["points"] = [[(ctx.cluster_points(f, k, aligned=False).copy(), ctx.cluster_points(f, k, aligned=True).copy())
                       for k in range(len(snap["clusters"][f]))] for f in range(F)]
    if opt["plane"] is not None:
        snap["pstats"] = [ctx.cluster_plane_stats(f) for f in range(F)]
    else:
        with pytest.raises(capi.CuboidError):
            ctx.cluster_plane_stats(0)
        snap["pstats"] = None
    if opt["filter"] is not None:
        snap["outlier"] = [ctx.outlier_stats(f) for f in range(F)]
    else:
        with pytest.raises(capi.CuboidError):
            ctx.outlier_stats(0)
        snap["outlier"] = None
    snap["point_labels"] = ctx.label_points_last(case.records()).copy()
    return snap


def same_snapshot(a, b, where):
    """Byte for byte."""
    assert a["res"] == b["res"], where
    for key in ("pi", "lb", "point_labels"):
        assert np.array_equal(a[key], b[key]), (where, key)
    for key in ("vox", "obj"):
        assert len(a[key]) == len(b[key]) and all(np.array_equal(x, y) for x, y in zip(a[key], b[key])), (where, key)
    assert a["clusters"] == b["clusters"], where
    for pa, pb in zip(a["points"], b["points"]):
        assert len(pa) == len(pb) and all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(pa, pb)), where
    assert (a["pstats"] is None) == (b["pstats"] is None) and (a["outlier"] is None) == (b["outlier"] is None), where
    if a["pstats"] is not None:
        assert all(np.array_equal(x, y) for x, y in zip(a["pstats"], b["pstats"])), where
    if a["outlier"] is not None:
        assert [[_bits(v) for v in o.values()] for o in a["outlier"]] == [[_bits(v) for v in o.values()] for o in b["outlier"]], where


def _bits(v):
    return int(np.float64(v).view(np.uint64))


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def aligned_of(case, c):
    """The aligned points cd_get_cluster_points returns for a cluster.  When the passes ran one per template, only the last
    slot's iterated cloud is resident; a cluster that kept another slot gets final_transformation * cluster, evaluated once."""
    if case.last_slot_resident and c.slot != max(case.tpls):
        return FR.IP.xform(c.T, c.points)
    return c.aligned


def check_cluster(got, c, where):
    assert (got.size, got.iterations, got.converged, got.accepted, got.template_slot, got.reserved) == \
        (c.size, c.iterations, c.converged, c.accepted, c.slot, 0), where
    assert np.array_equal(_u32(list(got.T)), _u32(c.T).ravel()), (where, "T")
    assert _bits(got.fitness) == _bits(c.fitness), (where, got.fitness, c.fitness)
    pose = np.array(list(got.pose), np.float64)
    assert np.array_equal(pose.view(np.uint64), np.asarray(c.pose, np.float64).view(np.uint64)) or \
        (np.isnan(pose).all() and np.isnan(c.pose).all()), (where, "pose")


def check(case, snap):
    """The snapshot of a call against the composed reference: everything fused_reference.expected returns."""
    exp = case.expected()
    res = (capi.CdFrameResult * case.F).from_buffer_copy(snap["res"])
    for f, e in enumerate(exp):
        r, where = res[f], "%s frame %d" % (case.id, f)
        n_plane, n_o, K = e["counts"][2], e["counts"][3], e["counts"][4]
        assert r.status == e["status"], where
        assert (r.n_cropped, r.n_voxels, r.n_plane, r.n_objects, r.n_clusters) == e["counts"], where
        assert (r.ransac_iterations, r.flags) == (e["ransac_iterations"], e["flags"]), where
        assert np.array_equal(_u32(list(r.plane)), _u32(e["plane"])), where
        assert np.array_equal(snap["pi"][f][:n_plane], e["plane_inliers"]) and (snap["pi"][f][n_plane:] == -1).all(), where
        assert np.array_equal(snap["lb"][f][:n_o], e["labels"]) and (snap["lb"][f][n_o:] == -1).all(), where
        assert np.array_equal(snap["vox"][f], e["voxels"]), where
        assert np.array_equal(snap["obj"][f], e["objects"]), where
        got = [capi.CdClusterResult.from_buffer_copy(b) for b in snap["clusters"][f]]
        assert len(got) == K == len(e["clusters"]), where
        for k, c in enumerate(e["clusters"]):
            wk = "%s cluster %d" % (where, k)
            check_cluster(got[k], c, wk)
            if k < capi.CD_MAX_CLUSTERS_PER_FRAME:
                assert bytes(r.clusters[k]) == snap["clusters"][f][k], wk
            orig, al = snap["points"][f][k]
            assert np.array_equal(_u32(orig[:, :3]), _u32(c.points)) and (orig[:, 3] == 1.0).all(), (wk, "points")
            assert np.array_equal(_u32(al[:, :3]), _u32(aligned_of(case, c))) and (al[:, 3] == 1.0).all(), (wk, "aligned points")
        for k in range(K, capi.CD_MAX_CLUSTERS_PER_FRAME):
            assert bytes(r.clusters[k]) == bytes(capi.CdClusterResult()), where
        if case.opt["plane"] is not None:
            ps = snap["pstats"][f]
            assert ps.shape == (K, 4) and [tuple(int(v) for v in row) for row in ps] == [c.plane_stats + (0,) for c in e["clusters"]], where
        if case.opt["filter"] is not None:
            o, w = snap["outlier"][f], e["outlier"]
            assert (o["n_before"], o["n_removed"]) == (w["n_before"], w["n_removed"]), where
            assert [_bits(o[k]) for k in ("mean", "stddev", "threshold")] == [_bits(w[k]) for k in ("mean", "stddev", "threshold")], where
        assert np.array_equal(snap["point_labels"][f], e["point_labels"]), (where, "point labels", int((snap["point_labels"][f] != e["point_labels"]).sum()))


def check_windows(ctx, case, snap):
    """cd_get_cluster_results and cd_get_cluster_plane_stats with first / count, beyond the record's eight clusters."""
    for f, e in enumerate(case.expected()):
        K = e["counts"][4]
        first = min(capi.CD_MAX_CLUSTERS_PER_FRAME, K)
        part = ctx.cluster_results(f, first=first, count=3)
        assert [bytes(c) for c in part] == snap["clusters"][f][first:first + 3]
        assert ctx.cluster_results(f, first=K) == []
        if case.opt["plane"] is not None:
            lo = max(K - 3, 0)
            assert np.array_equal(ctx.cluster_plane_stats(f, first=lo, count=2), snap["pstats"][f][lo:lo + 2])
            assert len(ctx.cluster_plane_stats(f, first=K, count=4)) == 0


FRESH = {}     # the fresh-context snapshot of every case that has run, for (e)


def fresh(monkeypatch, case, env=None, windows=True):
    c = make_ctx(monkeypatch, case.N, case.F, case.tpls, env)
    try:
        snap = run(c, case)
        if windows:
            check_windows(c, case, snap)
    finally:
        c.close()
    FRESH[case.id] = snap
    return snap


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", [r.id for r in TABLE])
def test_option_table(monkeypatch, row_id):
    case = table_case(row_id)
    check(case, fresh(monkeypatch, case))


@pytest.mark.parametrize("kind", ["unbounded", "bounded", "slots"])
def test_stops_inside_a_batch(monkeypatch, kind):
    """Every pair, stopped or not, equals the reference - in particular those a workgroup runs after a stopped one: the launch
    has two workgroups (CUBOID_ICP_MAX_WG = 1) and many more pairs.  A stop is a property of the cluster record: the frame of a
    stopped cluster stays CD_OK."""
    case = stop_case(kind)
    snap = fresh(monkeypatch, case, env={"CUBOID_ICP_MAX_WG": "1"})
    exp = case.expected()
    pairs = sum(len(c.pairs) for e in exp for c in e["clusters"])
    assert snap["regime"] == (1 << 16) | 2 and pairs > 2      # rule C17's driver, two workgroups, more pairs than workgroups
    check(case, snap)
    res = (capi.CdFrameResult * case.F).from_buffer_copy(snap["res"])
    assert [res[f].status for f in range(case.F)] == [capi.CD_OK] * case.F
    assert any(c.stopped for c in exp[LINE_FRAME]["clusters"])


@pytest.mark.parametrize("plane_on", [1, 0])
def test_tiny_clusters(monkeypatch, plane_on):
    """cluster_min_size = 1 (check_params accepts it): clusters of one and two points get the record of a pre-marked problem."""
    case = tiny_case(plane_on)
    check(case, fresh(monkeypatch, case))


def test_per_template_fallback(monkeypatch):
    case = fallback_case()
    check(case, fresh(monkeypatch, case))


def test_one_context_through_a_sequence_of_settings(monkeypatch):
    """Six rows of the table in an order that turns every option on, off and on again, the stop batch in between: every call
    equals the result a fresh context gave (test_option_table, test_stops_inside_a_batch), byte for byte."""
    cases = [stop_case("unbounded") if s == "stops" else table_case(s) for s in SEQUENCE]
    for case in cases:
        if case.id not in FRESH:
            fresh(monkeypatch, case, windows=False)
    c = make_ctx(monkeypatch, W * H, 5, small_templates())
    try:
        for case in cases:
            same_snapshot(run(c, case), FRESH[case.id], case.id)   # (run: the read-backs of an option that is off are refused)
    finally:
        c.close()
