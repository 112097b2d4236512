"""cd_surface_batch and CD_GUESS_SURFACE on the GPU.

1. cd_surface_batch equals cd_surface_frame frame by frame (and the oracle's surface_frame): record bytes and statuses.
2. A CD_GUESS_SURFACE batch equals a CD_GUESS_PER_FRAME batch whose guesses are cd_surface_frame -> cd_surface_guess of each
   frame's objects cloud (identity where the fit fails), byte for byte apart from the CD_FRAME_SURFACE_GUESS bit, in every
   record and read-back, under each ICP driver.
3. Against the oracle: process_frame with CD_GUESS_PARAMS and the guess of the oracle's own surface fit.
4. The behaviour on the pre-check frames: accepted, fewer ICP iterations than the identity start, within 5 mm.
5. Depth input, the cd_set_frame_guesses store, cd_get_surface_results, cd_icp and the threshold setter."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from perception_amd import capi, pcd, synth, templates
from test_oracle_kat import _corner_cloud
from test_surface_guess_cpu import scene_with_yaw

pytestmark = pytest.mark.gpu

IDENT = np.eye(4, dtype=np.float32)


def _b(x):
    return bytes(memoryview(x).cast("B"))


def _objects(i, k_obj):
    """The objects cloud and ground-plane normal the oracle's chain gives frame i with k_obj boxes."""
    from oracle import oracle_py as O
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    o = O.process_frame(synth.frame(i, k_obj=k_obj), capi.default_params(), tpl, want_clouds=True)
    return o["objects"], np.array(o["result"].plane[:3], np.float32)


def _sne_params(thr):
    p = capi.default_params()
    p.plane_distance_threshold = thr
    return p


def _check_batch(ctx, O, clouds, normals, thr, invert):
    prm = _sne_params(thr)
    status, out = ctx.surface_batch(clouds, normals, prm, invert=invert)
    for f, (c, n) in enumerate(zip(clouds, normals)):
        st1, r1 = ctx.surface_frame(c, n, prm, invert=invert)
        so, ro = O.surface_frame(np.asarray(c, np.float32), n, prm, invert=invert)
        assert status[f] == st1 == so, (f, status[f], st1, so)
        assert _b(out[f]) == _b(r1) == _b(ro), f
    return status


def test_surface_batch_equals_surface_frame(O):
    rng = np.random.default_rng(3)
    clouds, normals = [], []
    for i, k in ((0, 1), (1, 1), (2, 3), (4, 3)):   # synthetic frames with one object and with three
        c, n = _objects(i, k)
        clouds.append(c[:, :3])
        normals.append(n)
    for yaw in (0.0, 0.7, -1.2):                      # corner clouds of the KAT
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        clouds.append(_corner_cloud(R, np.array([0.02, -0.03, 0.5]), rng))
        normals.append(np.array([0, 0, 1], np.float32))
    flat = np.c_[rng.uniform(-0.2, 0.2, 800), rng.uniform(-0.2, 0.2, 800), np.full(800, 0.5)].astype(np.float32)
    clouds.append(flat)                               # a flat cloud: no perpendicular planes
    normals.append(np.array([0, 0, 1], np.float32))
    clouds.append(np.zeros((0, 3), np.float32))       # an empty frame
    normals.append(np.array([0, 0, 1], np.float32))
    clouds.append(clouds[0][:57])                     # ragged counts
    normals.append(normals[0])
    ctx = capi.Context(max_points=max(len(c) for c in clouds), max_frames=len(clouds))
    try:
        for invert in (True, False):
            _check_batch(ctx, O, clouds, normals, 0.015, invert)
        s_hi = _check_batch(ctx, O, clouds, normals, 0.015, True)
        s_lo = _check_batch(ctx, O, clouds, normals, 0.004, True)
        # frames that fail at the launch threshold and fit at 0.004 (the pre-check's finding)
        assert any(a == capi.CD_ERR_NO_MODEL and b == capi.CD_OK for a, b in zip(s_hi, s_lo))
        assert s_lo[len(clouds) - 2] == capi.CD_ERR_NO_MODEL   # (the empty frame)
    finally:
        ctx.close()


def test_surface_batch_arguments():
    ctx = capi.Context(max_points=100, max_frames=2)
    lib, prm = ctx.lib, capi.default_params()
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    pts = np.zeros((2, 100, 4), np.float32)
    tn = np.zeros((2, 3), np.float32)
    out = (capi.CdSurfaceFrameResult * 3)()
    st = np.zeros(3, np.int32)

    def call(n, stride=16, P=100, F=2):
        n = np.asarray(n, np.int32)
        return lib.cd_surface_batch(ctx.h, capi._ptr(pts), stride, P, n.ctypes.data_as(i32), F, tn.ctypes.data_as(f32), 1,
                                    C.byref(prm), out, st.ctypes.data_as(i32))
    try:
        assert call([10, 101]) == capi.CD_ERR_INVALID_ARG     # more than points_per_frame
        assert call([10, 10], stride=18) == capi.CD_ERR_INVALID_ARG
        assert call([10, 10], F=0) == capi.CD_ERR_INVALID_ARG
        assert call([10, 10, 10], F=3) == capi.CD_ERR_CAPACITY
        assert call([10, 101], P=200) == capi.CD_ERR_CAPACITY  # a cloud larger than the context
        assert call([0, 0]) == capi.CD_OK and list(st[:2]) == [capi.CD_ERR_NO_MODEL] * 2
    finally:
        ctx.close()


# ---- 2. the fused equivalence ----------------------------------------------------------------------------------------------
def _readback(ctx, res, F):
    recs, clus, clouds, pts = [], [], [], []
    for f in range(F):
        r = res[f]
        recs.append((r.flags, _b(r)))
        clus.append([_b(c) for c in ctx.cluster_results(f)])
        clouds.append([ctx.frame_cloud(f, w).tobytes() for w in (capi.CD_CLOUD_VOXELS, capi.CD_CLOUD_OBJECTS)])
        pts.append([ctx.cluster_points(f, k, aligned=a).tobytes() for k in range(len(clus[-1])) for a in (False, True)])
    return recs, clus, clouds, pts


def _fused_equivalence(frames, prm, tpl, thr=0.015, min_flagged=1):
    F = len(frames)
    ctx = capi.Context(max_points=frames.shape[1], max_frames=F)
    try:
        ctx.set_template(0, tpl)
        if thr != 0.015:
            ctx.set_surface_distance_threshold(thr)
        stored = np.stack([IDENT] * F)         # a store the surface call must leave alone
        stored[:, 0, 3] = 0.01
        ctx.set_frame_guesses(stored)
        prm.icp_use_guess = capi.CD_GUESS_SURFACE
        res_s, pi_s, lb_s = ctx.process_batch(frames, prm, want_indices=True)
        sur_status, sur = ctx.surface_results()
        rb_s = _readback(ctx, res_s, F)
        # the reference guesses, from the single-frame calls on the read-back objects clouds
        guesses, flagged = [], []
        sne = _sne_params(thr)
        for f in range(F):
            r = res_s[f]
            g, fl = IDENT, False
            if any(r.plane):
                obj = np.frombuffer(rb_s[2][f][1], np.float32).reshape(-1, 4)[:, :3]
                st, sr = ctx.surface_frame(obj, np.array(r.plane[:3], np.float32), sne, invert=True)
                assert st == sur_status[f] and _b(sr) == _b(sur[f]), f
                if st == capi.CD_OK:
                    g, fl = capi.surface_guess(np.array(sr.Rt, np.float32)), True
            else:
                assert sur_status[f] == capi.CD_ERR_NO_MODEL
            guesses.append(g)
            flagged.append(fl)
            assert bool(r.flags & capi.CD_FRAME_SURFACE_GUESS) == fl, f
        assert sum(flagged) >= min_flagged
        ctx.set_frame_guesses(np.stack(guesses))
        prm.icp_use_guess = capi.CD_GUESS_PER_FRAME
        res_p, pi_p, lb_p = ctx.process_batch(frames, prm, want_indices=True)
        rb_p = _readback(ctx, res_p, F)
        for f in range(F):
            fs, bs = rb_s[0][f]
            fp, bp = rb_p[0][f]
            assert fs & ~capi.CD_FRAME_SURFACE_GUESS == fp
            res_s[f].flags = fp
            assert _b(res_s[f]) == _b(res_p[f]), f
        assert rb_s[1:] == rb_p[1:]
        assert np.array_equal(pi_s, pi_p) and np.array_equal(lb_s, lb_p)
        # a non-surface call: cd_get_surface_results refuses
        with pytest.raises(capi.CuboidError):
            ctx.surface_results()
        # the store set before the surface call was not touched by it: a PER_FRAME batch with it equals a fresh context's
        ctx.set_frame_guesses(stored)
        prm.icp_use_guess = capi.CD_GUESS_SURFACE
        ctx.process_batch(frames, prm)
        prm.icp_use_guess = capi.CD_GUESS_PER_FRAME
        res_a, _, _ = ctx.process_batch(frames, prm)
        ctx2 = capi.Context(max_points=frames.shape[1], max_frames=F)
        try:
            ctx2.set_template(0, tpl)
            ctx2.set_frame_guesses(stored)
            res_b, _, _ = ctx2.process_batch(frames, prm)
        finally:
            ctx2.close()
        assert capi.results_to_array(res_a).tobytes() == capi.results_to_array(res_b).tobytes()
        return res_s
    finally:
        ctx.close()


def _frames(idx, k_obj=1):
    return np.stack([synth.frame(i, k_obj=k_obj) for i in idx], 0)


@pytest.mark.parametrize("cluster_enable", [1, 0])
def test_fused_equivalence_default_driver(template, cluster_enable):
    prm = capi.default_params()
    prm.cluster_enable = cluster_enable
    frames = np.concatenate([_frames((0, 3, 6)), _frames((1,), k_obj=3)], 0)
    _fused_equivalence(frames, prm, template, thr=0.004)


@pytest.mark.parametrize("env", [{"CUBOID_ICP_LATTICE": "0"}, {"CUBOID_ICP_MODE": "sliced"}, {"CUBOID_ICP_MODE": "cluster"},
                                 {"CUBOID_ICP_MODE": "pipe"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_fused_equivalence_every_driver(template, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _fused_equivalence(_frames((0, 3, 6)), capi.default_params(), template, thr=0.004)


def test_fused_equivalence_launch_threshold(template):
    """At 0.015 most single-box frames fail their first fit: identity guesses, no flag, same bytes."""
    _fused_equivalence(_frames((0, 1, 2, 3)), capi.default_params(), template, thr=0.015, min_flagged=0)


def test_fused_equivalence_scanned_template():
    tpl = pcd.read_xyz(os.path.join(GOLDEN, "eraser_ascii.pcd"))
    _fused_equivalence(_frames((0, 3, 6)), capi.default_params(), tpl, thr=0.004)


def test_process_frame_surface_mode(template):
    """cd_process_frame takes the mode too: equal to a batch of one."""
    fr = synth.frame(2, k_obj=1)
    prm = capi.default_params()
    prm.icp_use_guess = capi.CD_GUESS_SURFACE
    ctx = capi.Context(max_points=fr.shape[0], max_frames=1)
    try:
        ctx.set_template(0, template)
        ctx.set_surface_distance_threshold(0.004)
        r1, _, _ = ctx.process_frame(fr, prm)
        rb, _, _ = ctx.process_batch(fr[None], prm)
        assert _b(r1) == _b(rb[0])
    finally:
        ctx.close()


# ---- 3. against the oracle -------------------------------------------------------------------------------------------------
def test_surface_mode_against_oracle(O, template):
    frames = [synth.render(scene_with_yaw(i, y)) for i, y in ((2, 60.0), (4, -70.0), (1, 30.0))]
    prm = capi.default_params()
    ctx = capi.Context(max_points=frames[0].shape[0], max_frames=len(frames))
    try:
        ctx.set_template(0, template)
        ctx.set_surface_distance_threshold(0.004)
        prm.icp_use_guess = capi.CD_GUESS_SURFACE
        res, _, _ = ctx.process_batch(np.stack(frames), prm)
    finally:
        ctx.close()
    sne = _sne_params(0.004)
    for f, fr in enumerate(frames):
        o0 = O.process_frame(fr, capi.default_params(), template, want_clouds=True)
        r0 = o0["result"]
        st, sr = O.surface_frame(o0["objects"], np.array(r0.plane[:3], np.float32), sne, invert=True)
        q = capi.default_params()
        if st == capi.CD_OK:
            q.icp_use_guess = capi.CD_GUESS_PARAMS
            g = capi.surface_guess(np.array(sr.Rt, np.float32)).reshape(16)
            for k in range(16):
                q.icp_guess[k] = float(g[k])
        ro = O.process_frame(fr, q, template)["result"]
        r = res[f]
        assert bool(r.flags & capi.CD_FRAME_SURFACE_GUESS) == (st == capi.CD_OK)
        r.flags = ro.flags
        assert _b(r) == _b(ro), f


# ---- 4. the behaviour ------------------------------------------------------------------------------------------------------
def test_surface_guess_helps_on_the_precheck_frames(template):
    cases = ((2, 60.0), (4, -70.0), (5, 45.0))
    scenes = [scene_with_yaw(i, y) for i, y in cases]
    frames = np.stack([synth.render(s) for s in scenes])
    ctx = capi.Context(max_points=frames.shape[1], max_frames=len(frames))
    try:
        ctx.set_template(0, template)
        ctx.set_surface_distance_threshold(0.004)
        prm = capi.default_params()
        base, _, _ = ctx.process_batch(frames, prm)
        base_it = [base[f].clusters[0].iterations for f in range(len(cases))]
        prm.icp_use_guess = capi.CD_GUESS_SURFACE
        res, _, _ = ctx.process_batch(frames, prm)
    finally:
        ctx.close()
    for f, sc in enumerate(scenes):
        r = res[f]
        assert r.flags & capi.CD_FRAME_SURFACE_GUESS and r.n_clusters == 1
        cl = r.clusters[0]
        assert cl.accepted
        assert cl.iterations < base_it[f], (f, cl.iterations, base_it[f])
        truth = synth.truth_poses(sc)[0]
        err = np.linalg.norm(np.array(cl.pose).reshape(4, 4)[:3, 3] - truth[:3, 3])
        assert err < 0.005, (f, err)


# ---- 5. further checks -----------------------------------------------------------------------------------------------------
def test_depth_batch_surface_mode_equals_cloud_batch(template):
    idx = (0, 3, 6)
    depth = np.stack([synth.depth_frame(i, k_obj=1)[0] for i in idx])
    cam = capi.default_depth_camera()
    cam.color = capi.CD_COLOR_NONE
    clouds = np.stack(list(_depth_clouds(depth, cam)))
    prm = capi.default_params()
    prm.rgb_offset = -1
    prm.icp_use_guess = capi.CD_GUESS_SURFACE
    ctx = capi.Context(max_points=depth.shape[1] * depth.shape[2], max_frames=len(idx))
    try:
        ctx.set_template(0, template)
        ctx.set_surface_distance_threshold(0.004)
        rd, _, _ = ctx.process_depth_batch(depth, None, cam, prm)
        sd = ctx.surface_results()
        rc, _, _ = ctx.process_batch(clouds, prm)
        sc = ctx.surface_results()
    finally:
        ctx.close()
    assert capi.results_to_array(rd).tobytes() == capi.results_to_array(rc).tobytes()
    assert np.array_equal(sd[0], sc[0]) and [_b(a) for a in sd[1]] == [_b(a) for a in sc[1]]
    assert any(rd[f].flags & capi.CD_FRAME_SURFACE_GUESS for f in range(len(idx)))


def _depth_clouds(depth, cam):
    ctx = capi.Context(max_points=depth.shape[1] * depth.shape[2], max_frames=1)
    try:
        for d in depth:
            yield ctx.depth_to_cloud(cam, d, None, stride_bytes=16, rgb_offset=-1).view(np.float32).copy()
    finally:
        ctx.close()


def test_cd_icp_refuses_surface_mode(template):
    ctx = capi.Context(max_points=1000, max_frames=1)
    try:
        ctx.set_template(0, template)
        prm = capi.default_params()
        prm.icp_use_guess = capi.CD_GUESS_SURFACE
        with pytest.raises(capi.CuboidError) as e:
            ctx.icp(0, template[:100] + np.float32(0.001), prm)
        assert e.value.status == capi.CD_ERR_INVALID_ARG
    finally:
        ctx.close()


def test_surface_threshold_setter():
    ctx = capi.Context(max_points=100, max_frames=1)
    try:
        assert ctx.surface_distance_threshold() == 0.015
        ctx.set_surface_distance_threshold(0.004)
        for bad in (0.0, -0.01, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(capi.CuboidError) as e:
                ctx.set_surface_distance_threshold(bad)
            assert e.value.status == capi.CD_ERR_INVALID_ARG
        assert ctx.surface_distance_threshold() == 0.004
        with pytest.raises(capi.CuboidError):   # no fused call yet
            ctx.surface_results()
    finally:
        ctx.close()
