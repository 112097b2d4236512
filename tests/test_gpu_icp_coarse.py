"""Coarse-to-fine ICP (rule C18) on the GPU, through the C-ABI, against the reference composed on the CPU
(tests/coarse_reference.py: fused_reference's own pair function, coarse pair -> hand-over -> fine pair), bit for bit: no tolerance.

  a. cd_icp against a lattice template (k_icp_lat) and an arbitrary one (the generic drivers) at the sizes around the eligibility
     edge, the smallest coarse sets and sizes the stride does not divide;
  b. fused batches of three small frames: the mode alone, with rule C17, with a bound, with each guess mode (the single guess of
     cd_params included), with template_slot = -1 over two templates in one grouped stage and in one pass per template, and with
     the outlier filter on a batch whose coarse sets need more room than the last frame's segment has left;
  c. off is off: the records and the launch count of a context that turned the mode off again equal those of one that never
     called the setter;
  d. one context through off -> on -> another stride -> off with a template change in between: every call equals its
     fresh-context result (stale pointers, regrown buffers).

Everything above the first test is plain CPU code: tests/test_coarse_reference_cpu.py imports the scenarios and asserts, from the
reference alone, that each of them shows what it is for."""
import functools
import os

import numpy as np
import pytest

import coarse_reference as CR
import fused_reference as FR
import test_gpu_fused_options as T
from conftest import GOLDEN, rot_xyz
from perception_amd import capi, pcd, synth

pytestmark = pytest.mark.gpu

W0, D0 = T.W0, T.D0
SW, SH = T.SW, T.SH


# ---- b. the fused scenarios --------------------------------------------------------------------------------------------------------
class CoarseCase(T.Case):
    """A fused call with the mode on: coarse = (stride, min_points).  shows: what tests/test_coarse_reference_cpu.py asserts of
    it besides an eligible pair that differs from its single-level record and an ineligible cluster that equals it."""

    def __init__(self, id, frames, prm, tpls, opt, coarse, shows=(), **kw):
        T.Case.__init__(self, id, frames, prm, tpls, opt, **kw)
        self.coarse, self.shows = coarse, shows

    @functools.lru_cache(maxsize=None)
    def expected(self):
        if self.coarse[0] == 0:
            return self.single()
        return CR.expected(self.frames, self.prm, self.tpls, self.opt, self.coarse)

    @functools.lru_cache(maxsize=None)
    def single(self):
        """The same call with the mode off."""
        return FR.expected(self.frames, self.prm, self.tpls, self.opt)

    def off(self):
        return CoarseCase(self.id + "-off", self.frames, self.prm, self.tpls, self.opt, (0, 0), last_slot_resident=self.last_slot_resident)


@functools.lru_cache(maxsize=None)
def small_batch():
    """Three frames of 128 x 96: the grid scene (twelve clusters of 76 .. 37 points), two boxes (735 and 335 points), one box (318)."""
    return np.ascontiguousarray(np.stack([synth.render(synth.scene_grid(3), width=SW, height=SH), synth.frame(1, width=SW, height=SH),
                                          synth.frame(0, width=SW, height=SH)], 0))


def small_params(slot, guess):
    prm = capi.default_params()
    prm.cluster_min_size = 30
    prm.icp_max_iterations = 8
    prm.template_slot = slot
    prm.icp_use_guess = FR.GUESS_MODES[guess]
    return prm


@functools.lru_cache(maxsize=None)
def scenario(name):
    """The settings (stride, min_points) put the eligibility edge inside the grid frame's cluster sizes (40 | 39, 61 | 44), so that
    frame 0 has eligible and ineligible clusters side by side.
      alone     the mode alone: no guess, one lattice template (k_icp_lat; its direct mode in the coarse stage only)
      c17       rule C17 with the per-cluster guess (rule C13 on the coarse set)
      bound     rule C17 with a 1 cm bound, per-frame guesses, two templates in one stage: the guess of a frame is its first
                cluster's, so every other cluster lies decimetres from the template, keeps no correspondence, stops - on the coarse
                set as well: those pairs fall back
      surface   the frame's surface guess, two templates in one stage: clusters whose kept slot is not the one the coarse
                fitness would have chosen
      passes    the per-template fallback of test_gpu_fused_options (one pass per template) with the filter and C17
      params    CD_GUESS_PARAMS, the mode alone: the single guess is frame 0's first-cluster guess.  The reference states the call as
                per-frame guesses that are all that guess - the same ICPs, and neither mode sets a flag
      params-bound   CD_GUESS_PARAMS with rule C17 and a 1 cm bound: cluster 0 of frame 0 is registered, every other pair stops,
                the eligible ones on the coarse set as well - they fall back to the single guess
      filter-big   the `passes` cloud twice, the filter and C17 on, every second point of the clusters of 300 points and more: the
                coarse sets end past the F * N points of a context created without the mode (filter_big_needs), and the filter
                has swapped the object buffer and an ICP source buffer by the time the ICP stage looks for the room"""
    tpls = T.small_templates()
    fr = small_batch()
    if name in ("alone", "alone-t1"):   # (-t1: the other template in slot 0, for the sequence's template change)
        return CoarseCase(name, fr, small_params(0, "none"), {0: tpls[0 if name == "alone" else 1]}, FR.options(), (2, 40))
    if name == "c17":
        return CoarseCase(name, fr, small_params(0, "cluster"), {0: tpls[0]}, FR.options(plane=(W0, D0), guess="cluster"), (5, 60))
    if name == "bound":
        prm = small_params(-1, "per_frame")
        g = T.first_cluster_guesses(fr, prm, tpls[0])
        return CoarseCase(name, fr, prm, tpls, FR.options(plane=(W0, D0), bound=0.01, guess="per_frame", frame_guesses=g), (2, 40), shows=("fall_back",))
    if name == "surface":
        return CoarseCase(name, fr, small_params(-1, "surface"), tpls, FR.options(guess="surface", surface_threshold=T.SURFACE_THR), (3, 40),
                          shows=("fine_choice",))
    if name in ("params", "params-bound"):
        prm = small_params(0, "none")
        G = np.ascontiguousarray(T.first_cluster_guesses(fr, prm, tpls[0])[0], np.float32)
        prm.icp_use_guess = capi.CD_GUESS_PARAMS
        prm.icp_guess[:] = [float(v) for v in G.ravel()]
        every = np.ascontiguousarray(np.stack([G] * len(fr)))
        if name == "params":
            return CoarseCase(name, fr, prm, {0: tpls[0]}, FR.options(guess="per_frame", frame_guesses=every), (2, 40))
        return CoarseCase(name, fr, prm, {0: tpls[0]}, FR.options(plane=(W0, D0), bound=0.01, guess="per_frame", frame_guesses=every), (2, 40),
                          shows=("fall_back",))
    c = T.fallback_case()
    if name == "filter-big":
        return CoarseCase(name, np.ascontiguousarray(np.concatenate([c.frames, c.frames])), c.prm, c.tpls, c.opt, (2, 300), last_slot_resident=True)
    assert name == "passes"
    return CoarseCase(name, c.frames, c.prm, c.tpls, c.opt, (4, 400), last_slot_resident=True)


def filter_big_needs(case):
    """(the points the ICP source buffers must hold for the case's largest stage, the F * N a context has without the mode): the
    stage's clusters lie frame-major, the coarse sets packed behind the last frame's (icp_coarse_plan.hpp)."""
    exp = case.expected()
    s, m = case.coarse
    span_last = sum(c.size for c in exp[-1]["clusters"])
    begin = -(-((case.F - 1) * case.N + span_last) // 16) * 16
    return begin + sum(-(-c.size // s) for e in exp for c in e["clusters"] if c.size >= m), case.F * case.N


SCENARIOS = ("alone", "c17", "bound", "surface", "passes", "params", "params-bound", "filter-big")
# (d): (scenario, mode on)
SEQUENCE = (("alone", False), ("alone", True), ("bound", True), ("alone-t1", True), ("surface", True), ("params-bound", True), ("surface", False),
            ("c17", True), ("params", True))


def expected_stats(case):
    """Per frame, the stats tuple of every cluster's kept pair."""
    return [[CR.stats_tuple(CR.coarse_stats_of(c.pairs[c.slot])) for c in e["clusters"]] for e in case.expected()]


def run(ctx, case):
    """T.run with the mode set as the case says, plus the stats and the launch count."""
    ctx.set_icp_coarse(*case.coarse)
    assert ctx.icp_coarse()[0] == case.coarse[0]
    snap = T.run(ctx, case)
    snap["launches"] = ctx.timing().icp_kernel_launches
    if case.coarse[0]:
        snap["cstats"] = [[CR.stats_tuple(s) for s in ctx.cluster_coarse_stats(f)] for f in range(case.F)]
    else:
        with pytest.raises(capi.CuboidError):
            ctx.cluster_coarse_stats(0)
        snap["cstats"] = None
    return snap


def same(a, b, where):
    T.same_snapshot(a, b, where)
    assert a["cstats"] == b["cstats"], where


def fresh(monkeypatch, case, env=None):
    c = T.make_ctx(monkeypatch, case.N, case.F, case.tpls, env)
    try:
        return run(c, case)
    finally:
        c.close()


# ---- a. cd_icp ---------------------------------------------------------------------------------------------------------------------
def icp_templates():
    """(a lattice: the corner of the launch template within 6 cm of its least coordinates; an arbitrary cloud: the marker scan)"""
    full = pcd.read_xyz(os.path.join(GOLDEN, "template_cuboid_L200_W100_H75_3faces.pcd")).astype(np.float32)
    cut = np.ascontiguousarray(full[((full - full.min(0)) <= np.float32(0.06)).all(1)])
    marker = pcd.read_xyz(os.path.join(GOLDEN, "marker_ascii_tf.pcd")).astype(np.float32)
    return {"lattice": cut, "arbitrary": np.ascontiguousarray(marker)}


def icp_sizes(stride):
    """[(min_points, n)]: around the least legal min_points (3 s: the coarse set of three points, and of four at 3 s + 1), around
    an edge the stride does not divide, and a larger set the stride does not divide."""
    m0, m1 = 3 * stride, 4 * stride + 3
    return [(m0, m0 - 1), (m0, m0), (m0, m0 + 1), (m0, 10 * stride + 3), (m1, m1 - 1), (m1, m1), (m1, m1 + 1), (m1, 3 * stride), (m1, 3 * stride + 1)]


def moved_subset(tpl, n, seed):
    rng = np.random.default_rng(seed)
    p = tpl[rng.choice(len(tpl), size=n, replace=n > len(tpl))].astype(np.float64)
    R = rot_xyz(*np.deg2rad(rng.uniform(-4.0, 4.0, 3)))
    return (p @ R.T + rng.uniform(-0.01, 0.01, 3) + rng.normal(0, 0.001, p.shape)).astype(np.float32)


def check_icp(ctx, slot, tpl, src, prm, coarse, opt, axes=None, where="", guess=None):
    """guess: the single guess of cd_params (CD_GUESS_PARAMS), or None"""
    ctx.set_icp_coarse(*coarse)
    if guess is not None:
        prm = FR.copy_params(prm)
        prm.icp_use_guess = capi.CD_GUESS_PARAMS
        prm.icp_guess[:] = [float(v) for v in np.asarray(guess, np.float32).ravel()]
    st, r, al = ctx.icp(slot, src, prm, want_aligned=True)
    e = CR.pair(tpl, axes, src, prm, opt, None if guess is None else np.asarray(guess, np.float32).reshape(4, 4), coarse)
    assert np.array_equal(np.asarray(list(r.T), np.float32).view(np.uint32), e["T"].view(np.uint32).ravel()), (where, "T")
    assert (r.size, r.iterations, r.converged, r.accepted) == (len(src), e["iterations"], e["converged"], e["accepted"]), where
    assert T._bits(r.fitness) == T._bits(e["fitness"]), (where, r.fitness, e["fitness"])
    assert np.array_equal(al.view(np.uint32), np.asarray(e["aligned"], np.float32).view(np.uint32)), (where, "aligned")
    assert st == (capi.CD_ERR_FEW_CORRESPONDENCES if e["stopped"] else capi.CD_OK), where
    got = ctx.cluster_coarse_stats(0)
    assert len(got) == 1 and CR.stats_tuple(got[0]) == CR.stats_tuple(e["coarse_stats"]), (where, CR.stats_tuple(got[0]), e["coarse_stats"])
    return e


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "arbitrary"])
@pytest.mark.parametrize("stride", [2, 5, 64])
def test_cd_icp_two_levels(monkeypatch, kind, stride):
    tpl = icp_templates()[kind]
    c = T.make_ctx(monkeypatch, 1024, 1, {0: tpl})
    try:
        assert (c.template_lattice_faces(0) > 0) == (kind == "lattice")
        assert c.timing().icp_search in (0, 1)
        prm = capi.default_params()
        prm.icp_max_iterations = 10
        used = set()
        for i, (m, n) in enumerate(icp_sizes(stride)):
            e = check_icp(c, 0, tpl, moved_subset(tpl, n, 1000 * stride + i), prm, (stride, m), FR.options(), where="%s s=%d m=%d n=%d" % (kind, stride, m, n))
            assert e["coarse_stats"].used == (capi.CD_COARSE_USED if n >= m else capi.CD_COARSE_NOT_ELIGIBLE)
            assert e["coarse_stats"].n_coarse == (-(-n // stride) if n >= m else 0)
            used.add(e["coarse_stats"].used)
        assert used == {capi.CD_COARSE_NOT_ELIGIBLE, capi.CD_COARSE_USED}
        assert c.timing().icp_search == (1 if kind == "lattice" else 0)
    finally:
        c.close()


def test_cd_icp_when_the_persistent_launch_hands_over(monkeypatch):
    """CUBOID_ICP_PERSIST = 2: the single launch of a small stage gives up and the multi-launch loop starts over from the initial
    states - which, in the fine stage, means the hand-over is applied again after they are uploaded again."""
    tpl = icp_templates()["arbitrary"]
    c = T.make_ctx(monkeypatch, 1024, 1, {0: tpl}, env={"CUBOID_ICP_PERSIST": "2"})
    try:
        prm = capi.default_params()
        prm.icp_max_iterations = 10
        for i, (m, n) in enumerate([(15, 14), (15, 15), (23, 53), (23, 200)]):
            before = c.timing().icp_persist_gave_up
            e = check_icp(c, 0, tpl, moved_subset(tpl, n, 70 + i), prm, (5, m), FR.options(), where="gave up m=%d n=%d" % (m, n))
            assert c.timing().icp_persist_gave_up - before == (2 if n >= m else 1), (m, n)      # one launch per level
            assert e["coarse_stats"].used == (capi.CD_COARSE_USED if n >= m else capi.CD_COARSE_NOT_ELIGIBLE)
    finally:
        c.close()


def test_cd_icp_falls_back_and_the_fine_level_runs_on(monkeypatch):
    """Rule C17 with a bound that keeps two correspondences of the coarse set and more of the whole cluster: the coarse ICP stops,
    the fine level starts from the call's own guess (none) and iterates."""
    tpl = icp_templates()["lattice"]
    axes = FR.IP.face_axes(tpl)
    src = moved_subset(tpl, 90, 5)
    src[:, 2] += np.float32(0.02)
    _, d2 = FR.IP.nearest(tpl, src)
    coarse_d2 = np.sort(d2[::3])
    bound = float(np.sqrt(0.5 * (np.float64(coarse_d2[1]) + np.float64(coarse_d2[2]))))
    d2_max = FR.correspondence_threshold(bound)
    assert (d2[::3] <= d2_max).sum() == 2 and (d2 <= d2_max).sum() >= 3
    c = T.make_ctx(monkeypatch, 1024, 1, {0: tpl})
    try:
        c.set_icp_plane_weight(W0, D0)
        c.set_icp_max_correspondence_distance(bound)
        prm = capi.default_params()
        prm.icp_max_iterations = 6
        e = check_icp(c, 0, tpl, src, prm, (3, 30), FR.options(plane=(W0, D0), bound=bound), axes=axes)
        s = e["coarse_stats"]
        assert (s.used, s.coarse_status, s.coarse_iterations, s.coarse_converged) == (capi.CD_COARSE_FELL_BACK, capi.CD_ERR_FEW_CORRESPONDENCES, 0, 0)
        assert e["iterations"] >= 1
    finally:
        c.close()


def small_motion(seed):
    rng = np.random.default_rng(seed)
    G = np.eye(4)
    G[:3, :3] = rot_xyz(*np.deg2rad(rng.uniform(-3.0, 3.0, 3)))
    G[:3, 3] = rng.uniform(-0.008, 0.008, 3)
    return G.astype(np.float32)


@pytest.mark.parametrize("kind", ["lattice", "arbitrary"])
def test_cd_icp_from_the_single_guess(monkeypatch, kind):
    """CD_GUESS_PARAMS: the coarse level starts from icp_guess, the fine level from T_c - or, not eligible, from icp_guess, which
    its set-up finds in Tfinal of the states and not in an uploaded guess."""
    tpl = icp_templates()[kind]
    c = T.make_ctx(monkeypatch, 1024, 1, {0: tpl})
    try:
        prm = capi.default_params()
        prm.icp_max_iterations = 10
        for i, (m, n) in enumerate([(30, 29), (30, 30), (30, 31), (30, 301), (15, 15)]):
            G = small_motion(40 + i)
            e = check_icp(c, 0, tpl, moved_subset(tpl, n, 300 + i), prm, (5, m), FR.options(), where="%s m=%d n=%d" % (kind, m, n), guess=G)
            assert e["coarse_stats"].used == (capi.CD_COARSE_USED if n >= m else capi.CD_COARSE_NOT_ELIGIBLE)
            none = CR.pair(tpl, None, moved_subset(tpl, n, 300 + i), prm, FR.options(), None, (5, m))
            assert none["T"].tobytes() != e["T"].tobytes()         # the guess reaches both levels' results
    finally:
        c.close()


@pytest.mark.parametrize("with_guess", [False, True])
def test_cd_icp_stats_after_a_singular_stop(monkeypatch, with_guess):
    """Rule C17 on a line of 41 points parallel to the template's bottom face, coordinates on a 2^-7 grid (the line of
    test_gpu_fused_options' stop batch): the step's system is exactly singular on the coarse set (21 points of the line) and on
    the whole line.  The coarse ICP stops, the pair falls back to the call's own guess - the single guess of cd_params, or none -
    the fine level stops as well, cd_icp returns CD_ERR_FEW_CORRESPONDENCES, and the pair's stats can be read like its plane stats."""
    tpl = T.small_templates()[0]
    axes = FR.IP.face_axes(tpl)
    k = np.arange(-20, 21, dtype=np.float64)
    z = 0.5 if with_guess else -(2.0 ** -6)
    line = np.stack([k * 2.0 ** -7, np.full(41, 2.0 ** -6), np.full(41, z)], 1).astype(np.float32)
    G = None
    if with_guess:
        G = FR.IDENT.copy()
        G[2, 3] = -(0.5 + 2.0 ** -6)
    c = T.make_ctx(monkeypatch, 1024, 1, {0: tpl})
    try:
        c.set_icp_plane_weight(W0, D0)
        prm = capi.default_params()
        prm.icp_max_iterations = 8
        e = check_icp(c, 0, tpl, line, prm, (2, 6), FR.options(plane=(W0, D0)), axes=axes, guess=G, where="line")
        s = e["coarse_stats"]
        assert (e["stopped_singular"], e["iterations"], s.n_coarse, s.used, s.coarse_status) == (1, 0, 21, capi.CD_COARSE_FELL_BACK, capi.CD_ERR_FEW_CORRESPONDENCES)
        assert [int(v) for v in c.cluster_plane_stats(0)[0][:3]] == [0, 0, 1]
    finally:
        c.close()


def test_filter_and_coarse_sets_beyond_a_plain_contexts_buffers(monkeypatch):
    """The setter is called once; two calls follow (the filter swaps the object buffer and an ICP source buffer in each)."""
    case = scenario("filter-big")
    need, plain = filter_big_needs(case)
    assert need > plain
    c = T.make_ctx(monkeypatch, case.N, case.F, case.tpls)
    try:
        c.set_icp_coarse(*case.coarse)
        for _ in range(2):
            snap = T.run(c, case)
            T.check(case, snap)
            assert [[CR.stats_tuple(s) for s in c.cluster_coarse_stats(f)] for f in range(case.F)] == expected_stats(case)
    finally:
        c.close()


@pytest.mark.parametrize("name", SCENARIOS)
def test_fused_batch(monkeypatch, name):
    """The records, cd_get_cluster_results, both read-backs of the points, the labels, the plane stats (T.check) and the coarse
    stats of the kept pairs against the composed reference."""
    case = scenario(name)
    snap = fresh(monkeypatch, case)
    T.check(case, snap)
    assert snap["cstats"] == expected_stats(case), name
    assert snap["launches"] >= 4      # two stages, the gather and the hand-over


# the lattice templates on the generic searches: the sliced loop, the persistent launch off, one whole-cluster launch
# (k_icp_cluster), the template groups of a several-template stage (k_icp_pipe)
DRIVERS = {"sliced": {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_PERSIST": "0"}, "auto": {"CUBOID_ICP_LATTICE": "0"},
           "whole": {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_MODE": "2"}, "grouped": {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_MODE": "3"}}


@pytest.mark.parametrize("driver", sorted(DRIVERS))
@pytest.mark.parametrize("name", ["alone", "surface"])
def test_fused_batch_on_the_generic_drivers(monkeypatch, name, driver):
    """The drivers agree bit for bit, so the reference is the same; what differs is who runs the two stages and finds the
    hand-over's states on the device (rule C17's scenarios have a driver of their own)."""
    case = scenario(name)
    snap = fresh(monkeypatch, case, env=DRIVERS[driver])
    T.check(case, snap)
    assert snap["cstats"] == expected_stats(case), (name, driver)


def test_setter_checks_its_arguments_and_keeps_the_setting(monkeypatch):
    c = T.make_ctx(monkeypatch, 1024, 1, {0: icp_templates()["lattice"]})
    try:
        assert c.icp_coarse() == (0, 0)
        c.set_icp_coarse(5, 60)
        for s, m in ((1, 100), (-2, 100), (65, 1000), (2, 5), (5, 14), (64, 191), (3, 0)):
            with pytest.raises(capi.CuboidError) as e:
                c.set_icp_coarse(s, m)
            assert e.value.status == capi.CD_ERR_INVALID_ARG and c.icp_coarse() == (5, 60), (s, m)
        c.set_icp_coarse(0, -9)                   # off: min_points is not looked at and stays
        assert c.icp_coarse() == (0, 60)
        with pytest.raises(capi.CuboidError):
            c.cluster_coarse_stats(0)
        c.set_icp_coarse(64, 192)
        assert c.icp_coarse() == (64, 192)
        c.set_icp_coarse(None)
        assert c.icp_coarse()[0] == 0
    finally:
        c.close()


def test_draw_and_verify_see_the_fine_result(monkeypatch):
    """cd_draw_last_results and cd_verify_last_results after a call with the mode on: what the explicit calls give for the poses
    of the reference's fine level."""
    case = scenario("alone")
    exp = case.expected()
    B = capi.CD_MAX_CLUSTERS_PER_FRAME
    poses, n = np.full((case.F, B, 4, 4), np.nan), np.zeros(case.F, np.int32)
    for f, e in enumerate(exp):
        n[f] = min(len(e["clusters"]), B)
        for k in range(n[f]):
            poses[f, k] = np.asarray(e["clusters"][k].pose).reshape(4, 4)
    depth = np.ascontiguousarray(np.stack([FR.depth_of_records(fr, SH, SW)[0] for fr in case.frames]))
    cam = capi.default_depth_camera()
    cam.width, cam.height = SW, SH
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params(SW, SH)
    cam.depth_scale = synth.DEPTH_SCALE
    cam.color = capi.CD_COLOR_NONE
    fx, fy, cx, cy = synth.depth_camera_params(SW, SH)
    oprm = capi.overlay_params(P=[fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1, 0], dims=(0.05, 0.05, 0.03))
    vprm = capi.verify_params(dims=(0.05, 0.05, 0.03), min_agree=1)
    c = T.make_ctx(monkeypatch, case.N, case.F, case.tpls)
    try:
        run(c, case)
        img = np.zeros((case.F, SH, SW, 3), np.uint8)
        boxes = bytes(c.draw_last_results(img, capi.CD_DRAW_ALL, oprm))
        verified = bytes(c.verify_last_results(depth, cam, capi.CD_VERIFY_ALL, vprm))
        want_img = np.zeros_like(img)
        assert bytes(c.draw_boxes(want_img, poses, n, oprm)) == boxes and np.array_equal(img, want_img) and img.any()
        assert bytes(c.verify_boxes(depth, poses, n, cam, vprm)) == verified
        assert sum(capi.CdVerifyBox.from_buffer_copy(verified, i * 48).verified for i in range(case.F * B)) == int(n.sum())
    finally:
        c.close()


@pytest.mark.parametrize("name", ["alone", "surface", "passes"])
def test_off_is_off(monkeypatch, name):
    """A context that had the mode on and turned it off again, against one that never called the setter: the same bytes and the
    same launch count - and both the single-level reference."""
    case = scenario(name).off()
    c = T.make_ctx(monkeypatch, case.N, case.F, case.tpls)
    try:
        never = T.run(c, case)
        never["launches"] = c.timing().icp_kernel_launches
        with pytest.raises(capi.CuboidError):
            c.cluster_coarse_stats(0)
    finally:
        c.close()
    c = T.make_ctx(monkeypatch, case.N, case.F, case.tpls)
    try:
        run(c, scenario(name))
        again = run(c, case)
    finally:
        c.close()
    T.same_snapshot(never, again, name)
    assert never["launches"] == again["launches"], name
    T.check(case, never)


def test_one_context_through_a_sequence(monkeypatch):
    """off -> on -> other settings and strides -> off -> on; slot 1 is empty until the first call that wants it, and slot 0's
    template is replaced and put back in between: every call equals the result of a fresh context with the case's own templates
    (a case that names slot 0 does not look at slot 1)."""
    cases = [scenario(n) if on else scenario(n).off() for n, on in SEQUENCE]
    want = [fresh(monkeypatch, case) for case in cases]
    c = T.make_ctx(monkeypatch, SW * SH, 3, {})
    try:
        for case, w in zip(cases, want):
            for slot, t in case.tpls.items():
                c.set_template(slot, t)
            same(run(c, case), w, case.id)
    finally:
        c.close()
