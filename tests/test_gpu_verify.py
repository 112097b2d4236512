"""Pose verification on the GPU (k_verify.hip, cd_verify_boxes_batch[_device], cd_verify_last_results[_device]): every field of
every record equals canonical rule C14 restated in numpy over WHOLE images (perception_amd/verify.py), the host, device and
one-frame-per-call forms agree, the depth images are only read, the last fused call's poses are verified as its records state
them and stay as they were, every argument check refuses before anything runs, and on depth-fed synth frames 0..15 the device
gives the records tests/test_verify_cpu.py gets from the CPU oracle (tests/golden/verify_records_frames_0_15.json): the same two
accepted clusters fail."""
import ctypes as C

import numpy as np
import pytest
import torch

from perception_amd import capi, synth, templates, verify
from test_gpu_overlay import NAN_POSE, _scene_poses
from test_verify_cpu import CUBE, at, depth_around, golden_records, random_poses, small_camera, synth_depth_camera, unit_camera

pytestmark = pytest.mark.gpu
W, H = synth.WIDTH, synth.HEIGHT
NF = 16
B8 = capi.CD_MAX_CLUSTERS_PER_FRAME


@pytest.fixture(scope="module")
def ctx(template):
    c = capi.Context(max_points=W * H, max_frames=NF)
    c.set_template(0, template)
    yield c
    c.close()


@pytest.fixture(scope="module")
def depth16():
    return np.stack([synth.depth_frame(i)[0] for i in range(16)])


def _dev(depth):
    t = torch.from_numpy(depth.view(np.int16)).cuda().view(torch.uint16)
    torch.cuda.synchronize()
    return t


def _check(ctx, depth, poses, n_boxes, cam, what="", box_dims=None, **kw):
    """The host form against the restatement, every field of every record; the image is unchanged."""
    F = depth.shape[0]
    poses = np.asarray(poses, np.float64).reshape(F, -1, 16)
    want = verify.verify(depth, poses, n_boxes, cam, dims=kw.get("dims", verify.DEFAULT_DIMS), tau=kw.get("tolerance", verify.DEFAULT_TOLERANCE),
                         min_agree=kw.get("min_agree", verify.DEFAULT_MIN_AGREE), min_score=kw.get("min_score", verify.DEFAULT_MIN_SCORE),
                         box_dims=box_dims)
    before = depth.copy()
    got = capi.verify_records(ctx.verify_boxes(depth, poses, n_boxes, cam, capi.verify_params(**kw), box_dims=box_dims), F, poses.shape[1])
    assert np.array_equal(depth, before), what
    bad = [(f, b, got[f, b], want[f, b]) for f in range(F) for b in range(poses.shape[1]) if got[f, b].tobytes() != want[f, b].tobytes()]
    assert not bad, (what, bad[:4])
    return want


# ---- device == restatement ------------------------------------------------------------------------------------------------------
def test_one_pixel_image(ctx):
    cam = unit_camera()
    depth = np.array([3, 3, 3], np.uint16).reshape(3, 1, 1)
    poses = np.stack([at(0.0, 0.0, 1.0), at(9.0, 0.0, 1.0), NAN_POSE])[:, None]
    r = _check(ctx, depth, poses, None, cam, "1x1", dims=CUBE, min_agree=1)
    assert r["verified"].ravel().tolist() == [1, 1, 0] and r["n_hit"].ravel().tolist() == [1, 0, 0] and r["passed"].ravel().tolist() == [1, 0, 0]
    for d, field in ((0, "n_invalid"), (1, "n_occluded"), (5, "n_through"), (4, "n_agree")):
        r = _check(ctx, np.full((1, 1, 1), d, np.uint16), poses[:1], None, cam, "1x1 d=%d" % d, dims=CUBE, tolerance=0.25)
        assert r[field][0, 0] == 1 and r["n_hit"][0, 0] == 1, (d, r)


def test_small_images_with_random_poses(ctx):
    from conftest import rot_xyz
    cam = small_camera()
    rng = np.random.default_rng(3)
    dims, tau = (0.4, 0.2, 0.1), 0.01
    poses = np.empty((5, 4, 4, 4))
    for f in range(5):
        for b in range(4):
            Tb = np.eye(4)
            Tb[:3, :3] = rot_xyz(*rng.uniform(-np.pi, np.pi, 3))
            Tb[:3, 3] = rng.uniform((-0.5, -0.4, 0.5), (0.5, 0.4, 1.5))
            poses[f, b] = Tb
    poses[1, 1, :3, :3] = np.eye(3)           # axis-aligned on the optical axis: the dd_a == 0 branch at u = cx = 48
    poses[1, 1, :3, 3] = (0.0, 0.01, 0.9)
    depth = np.stack([depth_around(cam, poses[f], dims, tau, rng) for f in range(5)])
    n = [4, 3, 0, 1, 4]                       # (valid poses sit in the slots beyond n_boxes: those records must stay zero)
    r = _check(ctx, depth, poses, n, cam, "97x61", dims=dims, tolerance=tau)
    assert (r["verified"] == 1).sum(axis=1).tolist() == n and (r["n_hit"] > 0).sum() >= 6
    for field in ("n_agree", "n_through", "n_occluded", "n_invalid"):
        assert r[field].sum() > 100, field
    assert not any(r[1, 3].tobytes()) and not any(r[2].tobytes()) and not any(r[3, 1:].tobytes())
    # the 400 poses of the CPU test (behind the camera, far off-screen, non-finite, huge, scaled): 25 frames of 16 slots
    rp = np.stack(random_poses()).reshape(25, 16, 4, 4)
    for lo in (0, 13):
        sl = rp[lo:lo + 12]
        dd = np.stack([depth_around(cam, sl[f], dims, tau, rng) for f in range(12)])
        r = _check(ctx, dd, sl, None, cam, "random %d" % lo, dims=dims, tolerance=tau)
        assert (r["verified"] == 0).sum() >= 30 and (r["n_hit"] > 0).sum() >= 30


def test_scene_frames(ctx, depth16):
    poses, n = _scene_poses()                 # overlap, a box across the right and the top border, one wholly outside, a NaN pose
    cam = synth_depth_camera()
    r = _check(ctx, depth16[:6], poses, n, cam, "scenes", dims=synth.CUBOID_DIMS)
    assert r["verified"].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 1], [1, 1, 1], [1, 1, 0], [1, 0, 1]]
    assert r["n_hit"][4, 0] == 0 and r["n_hit"][3, 2] > 0 and r["n_hit"][4, 1] > 0
    assert r["passed"][1, 0] == 1 and r["n_through"][1, 0] == 0     # a truth pose on its own frame


def test_rectangle_edge_cases(ctx):
    cam = small_camera()
    rng = np.random.default_rng(8)
    # a box close enough to cover the whole image: the rectangle is the image
    big, tau = (4.0, 3.0, 0.2), 0.01
    T = at(0.0, 0.0, 0.5)
    depth = depth_around(cam, [T], big, tau, rng)[None]
    r = _check(ctx, depth, T[None, None], None, cam, "whole image", dims=big, tolerance=tau)
    assert r["n_hit"][0, 0] == 97 * 61
    # slivers 0.07 pixels wide on the first column, the last column and column 49; and two beyond the borders, whose clipped
    # rectangles are one pixel wide (column 0, column 96) and hold no hit
    thin = (0.001, 0.3, 0.001)
    poses = np.stack([at(-48.0 / 70.0, 0.0, 1.0), at(48.0 / 70.0, 0.0, 1.0), at(1.0 / 70.0, 0.0, 1.0), at(-49.5 / 70.0, 0.0, 1.0),
                      at(49.5 / 70.0, 0.0, 1.0)])[None]
    depth = depth_around(cam, poses[0], thin, tau, rng)[None]
    r = _check(ctx, depth, poses, None, cam, "slivers", dims=thin, tolerance=tau, min_agree=1)
    assert (r["verified"][0] == 1).all() and (r["n_hit"][0, :3] > 15).all() and (r["n_hit"][0, :3] <= 22).all() and not r["n_hit"][0, 3:].any(), r["n_hit"]


def test_many_boxes_per_frame_and_box_dims(ctx):
    cam = small_camera()
    rng = np.random.default_rng(40)
    dims, tau = (0.3, 0.2, 0.1), 0.01
    poses = np.empty((2, 40, 4, 4))
    for f in range(2):
        for b in range(40):
            poses[f, b] = at(*rng.uniform((-0.5, -0.3, 0.6), (0.5, 0.3, 1.4)))
    depth = np.stack([depth_around(cam, poses[f, :6], dims, tau, rng) for f in range(2)])
    r = _check(ctx, depth, poses, [33, 2], cam, "40 slots", dims=dims, tolerance=tau)
    assert (r["verified"][0] == 1).sum() == 33 and (r["verified"][1] == 1).sum() == 2
    # dims per slot against params->dims
    bd = rng.uniform(0.05, 0.4, (2, 40, 3))
    bd[1, 5] = np.nan                          # (beyond n_boxes: not looked at)
    a = _check(ctx, depth, poses, [33, 2], cam, "box_dims", box_dims=bd, dims=dims, tolerance=tau)
    assert not np.array_equal(a["n_hit"], r["n_hit"])


def test_host_device_and_batch_forms_agree(ctx, depth16):
    poses, n = _scene_poses()
    cam = synth_depth_camera()
    prm = capi.verify_params(dims=synth.CUBOID_DIMS)
    depth = np.ascontiguousarray(depth16[:6])
    hb = ctx.verify_boxes(depth, poses, n, cam, prm)
    t = _dev(depth)
    db = ctx.verify_boxes(t, poses, n, cam, prm)
    assert bytes(db) == bytes(hb)
    assert bytes(ctx.verify_boxes(t, poses, n, cam, prm)) == bytes(hb), "a second call gave other records"
    assert np.array_equal(t.cpu().numpy().view(np.uint16), depth), "the depth tensor changed"
    for f in range(6):
        ob = ctx.verify_boxes(depth[f:f + 1], poses[f:f + 1], n[f:f + 1], cam, prm)
        assert bytes(ob)[:3 * 48] == bytes(hb)[f * 3 * 48:(f + 1) * 3 * 48], f
    assert bytes(ctx.verify_boxes(depth, poses, n, cam, None)) == bytes(ctx.verify_boxes(depth, poses, n, cam, capi.default_verify_params()))


# ---- the last fused call's poses -------------------------------------------------------------------------------------------------
def _record_poses(res, F, which):
    poses = np.full((F, B8, 4, 4), np.nan)
    n = np.zeros(F, np.int32)
    for f in range(F):
        n[f] = min(res[f].n_clusters, B8)
        for k in range(n[f]):
            if which == capi.CD_VERIFY_ALL or res[f].clusters[k].accepted:
                poses[f, k] = np.array(res[f].clusters[k].pose).reshape(4, 4)
    return poses, n


def test_verify_last_results_after_a_depth_batch(ctx, prm, template, depth16):
    F = 4
    depth = np.ascontiguousarray(depth16[:F])
    rgb = np.stack([synth.depth_frame(i)[1] for i in range(F)])
    cam = synth_depth_camera()
    cam.color = capi.CD_COLOR_RGB8
    strict = capi.default_params()
    strict.icp_accept_fitness = 7.3e-6     # between the fitnesses of these frames' clusters: ACCEPTED and ALL differ
    res, _, _ = ctx.process_depth_batch(depth, rgb, cam, strict)
    before = bytes(capi.results_to_array(res).tobytes())
    clusters_before = [bytes(c) for f in range(F) for c in ctx.cluster_results(f)]
    cloud_before = ctx.frame_cloud(0, capi.CD_CLOUD_OBJECTS).tobytes()
    vprm = capi.verify_params(dims=synth.CUBOID_DIMS)
    t = _dev(depth)
    verified = {}
    for which in (capi.CD_VERIFY_ACCEPTED, capi.CD_VERIFY_ALL):
        poses, n = _record_poses(res, F, which)
        want = verify.verify(depth, poses, n, cam, dims=synth.CUBOID_DIMS)
        got = capi.verify_records(ctx.verify_last_results(depth, cam, which, vprm), F, B8)
        assert got.tobytes() == want.tobytes(), which
        assert bytes(ctx.verify_last_results(t, cam, which, vprm)) == got.tobytes(), which
        verified[which] = int(want["verified"].sum())
    assert 0 < verified[capi.CD_VERIFY_ACCEPTED] < verified[capi.CD_VERIFY_ALL] == sum(res[f].n_clusters for f in range(F))
    # verifying left the fused call's records and read-backs as they were
    assert bytes(capi.results_to_array(res).tobytes()) == before
    assert [bytes(c) for f in range(F) for c in ctx.cluster_results(f)] == clusters_before
    assert ctx.frame_cloud(0, capi.CD_CLOUD_OBJECTS).tobytes() == cloud_before
    assert np.array_equal(t.cpu().numpy().view(np.uint16), depth)
    # drawing still works after it, and verifying after drawing
    img = np.array(rgb, copy=True)
    ctx.draw_last_results(img, capi.CD_DRAW_ALL)
    assert (img != rgb).any()
    assert capi.verify_records(ctx.verify_last_results(depth, cam, capi.CD_VERIFY_ALL, vprm), F, B8).tobytes() == want.tobytes()
    # another compute call in between: nothing to verify any more
    ctx.icp(0, template[:600], prm)
    for d in (depth, t):
        with pytest.raises(capi.CuboidError) as e:
            ctx.verify_last_results(d, cam, capi.CD_VERIFY_ALL, vprm)
        assert e.value.status == capi.CD_ERR_INVALID_ARG
    # ... and cd_verify_boxes_batch is such a compute call
    ctx.process_depth_batch(depth, rgb, cam, strict)
    ctx.verify_boxes(depth[:1], np.eye(4)[None, None], None, cam, vprm)
    with pytest.raises(capi.CuboidError) as e:
        ctx.verify_last_results(depth, cam, capi.CD_VERIFY_ALL, vprm)
    assert e.value.status == capi.CD_ERR_INVALID_ARG


def test_verify_last_results_without_a_fused_call():
    c = capi.Context(max_points=64 * 48, max_frames=2)
    cam = unit_camera(64, 48)
    with pytest.raises(capi.CuboidError) as e:
        c.verify_last_results(np.zeros((1, 48, 64), np.uint16), cam)
    assert e.value.status == capi.CD_ERR_INVALID_ARG
    c.close()


def test_use_slot_dims_picks_the_dims_of_each_records_slot(template, depth16):
    other = (0.2, 0.075, 0.1)
    c = capi.Context(max_points=W * H, max_frames=2)
    c.set_template(0, template)
    c.set_template(1, templates.template_xyz32(*other, 0.005))
    prm = capi.default_params()
    prm.template_slot = -1
    cam = synth_depth_camera()
    depth = np.ascontiguousarray(depth16[1:3])
    res, _, _ = c.process_depth_batch(depth, None, cam, prm)
    poses, n = _record_poses(res, 2, capi.CD_VERIFY_ALL)
    slots = [[res[f].clusters[k].template_slot for k in range(n[f])] for f in range(2)]
    print("template slots of the records:", slots)
    for table in ({0: synth.CUBOID_DIMS, 1: other}, {0: other, 1: synth.CUBOID_DIMS}):
        bd = np.zeros((2, B8, 3))
        for f in range(2):
            for k in range(n[f]):
                bd[f, k] = table[slots[f][k]]
        want = verify.verify(depth, poses, n, cam, box_dims=bd)
        vprm = capi.verify_params(dims=(9.0, 9.0, 9.0), slot_dims=table, use_slot_dims=1)
        got = capi.verify_records(c.verify_last_results(depth, cam, capi.CD_VERIFY_ALL, vprm), 2, B8)
        assert got.tobytes() == want.tobytes(), table
    c.close()


# ---- behaviour --------------------------------------------------------------------------------------------------------------------
def test_the_device_gives_the_cpu_records_on_frames_0_to_15(ctx, depth16):
    cam = synth_depth_camera()
    t = _dev(depth16)
    res = ctx.process_depth_batch_device(t, None, cam, capi.default_params())
    got = capi.verify_records(ctx.verify_last_results(t, cam, capi.CD_VERIFY_ALL, capi.verify_params(dims=synth.CUBOID_DIMS)), 16, B8)
    gold = golden_records()
    failed, seen = [], 0
    for f in range(16):
        n = min(res[f].n_clusters, B8)
        assert not any(got[f, n:].tobytes())
        for k in range(n):
            r, g = got[f, k], gold[f, k]
            print("frame %2d cluster %d: accepted %d %s" % (f, k, res[f].clusters[k].accepted, r))
            assert int(res[f].clusters[k].accepted) == g["accepted"], (f, k)
            assert all(int(r[key]) == g[key] for key in ("verified", "passed") + verify.COUNTS), (f, k, r, g)
            assert r["score"] == verify.score(g["n_agree"], g["n_through"])
            seen += 1
            if res[f].clusters[k].accepted and not r["passed"]:
                failed.append((f, k))
                assert r["score"] < 0.5
    assert seen == len(gold) == 33 and failed == [(5, 2), (14, 2)], failed


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(ctx, depth16):
    lib, h = ctx.lib, ctx.h
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    depth = np.ascontiguousarray(depth16[:2])
    poses = np.ascontiguousarray(np.stack(synth.truth_poses(synth.scene_for(0, k_obj=3)))[None].repeat(2, 0))
    n = np.array([3, 2], np.int32)
    out = (capi.CdVerifyBox * 6)()
    C.memset(out, 0x5A, C.sizeof(out))
    untouched = bytes(out)
    good_cam, good = synth_depth_camera(), capi.verify_params(dims=synth.CUBOID_DIMS)
    t = _dev(depth)
    bad = capi.CD_ERR_INVALID_ARG

    def cam_with(**kw):
        c = synth_depth_camera()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def call(d=depth, cam=good_cam, F=2, p=poses, nb=n, B=3, bd=None, prm=good, o=out, fn=lib.cd_verify_boxes_batch):
        ptr = None if d is None else (C.c_void_p(d.data_ptr()) if fn is lib.cd_verify_boxes_batch_device else d.ctypes.data_as(C.c_void_p))
        return fn(h, None if cam is None else C.byref(cam), ptr, F, None if p is None else p.ctypes.data_as(dp),
                  None if nb is None else nb.ctypes.data_as(ip), B, None if bd is None else bd.ctypes.data_as(dp),
                  None if prm is None else C.byref(prm), o)

    for fn, d in ((lib.cd_verify_boxes_batch, depth), (lib.cd_verify_boxes_batch_device, t)):
        k = dict(fn=fn, d=d)
        assert call(**dict(k, d=None)) == bad and call(cam=None, **k) == bad and call(p=None, **k) == bad and call(nb=None, **k) == bad and call(o=None, **k) == bad
        for field in ("fx", "fy", "depth_scale"):
            for v in (0.0, -1.0, np.nan, np.inf):
                assert call(cam=cam_with(**{field: v}), **k) == bad, (field, v)
        assert call(cam=cam_with(color=5), **k) == bad
        assert call(cam=cam_with(width=0), **k) == bad and call(cam=cam_with(height=0), **k) == bad and call(cam=cam_with(width=-4), **k) == bad
        assert call(cam=cam_with(width=W + 1), **k) == bad                 # width * height over max_points
        assert call(F=0, **k) == bad and call(F=-1, **k) == bad and call(F=NF + 1, **k) == bad
        assert call(B=0, **k) == bad and call(B=1025, **k) == bad
        for v in (np.nan, np.inf, -np.inf, -0.01):
            assert call(prm=capi.verify_params(dims=(0.2, v, 0.03)), **k) == bad, v
            assert call(prm=capi.verify_params(tolerance=v), **k) == bad, v
            bd = np.full((2, 3, 3), 0.1)
            bd[1, 1, 2] = v
            assert call(bd=bd, **k) == bad, v
        for v in (np.nan, np.inf, -np.inf):
            assert call(prm=capi.verify_params(min_score=v), **k) == bad, v
        assert call(prm=capi.verify_params(min_agree=-1), **k) == bad
        assert call(nb=np.array([3, -1], np.int32), **k) == bad and call(nb=np.array([4, 0], np.int32), **k) == bad
    assert bytes(out) == untouched, "a refused call wrote records"
    assert np.array_equal(depth, depth16[:2]) and np.array_equal(t.cpu().numpy().view(np.uint16), depth16[:2])
    assert lib.cd_verify_boxes_batch(None, None, None, 2, None, None, 3, None, None, None) == bad
    # a non-finite pose is not an error; zero dims, zero tolerance and the boundary counts are accepted
    poses2 = poses.copy()
    poses2[0, 1, 2, 3] = np.inf
    assert call(p=poses2, nb=np.array([3, 0], np.int32), prm=capi.verify_params(dims=(0.2, 0.0, 0.03), tolerance=0.0, min_score=-1.0, min_agree=0)) == capi.CD_OK
    assert [out[i].verified for i in range(6)] == [1, 0, 1, 0, 0, 0]
    # cd_verify_last_results: the same checks on what it takes
    res, _, _ = ctx.process_depth_batch(depth[:1], None, good_cam, capi.default_params())
    out8 = (capi.CdVerifyBox * 8)()
    C.memset(out8, 0x5A, C.sizeof(out8))
    untouched = bytes(out8)
    last = lambda d=depth[:1], cam=good_cam, which=capi.CD_VERIFY_ALL, prm=good, o=out8: lib.cd_verify_last_results(
        h, None if cam is None else C.byref(cam), None if d is None else d.ctypes.data_as(C.c_void_p), which, C.byref(prm), o)
    assert last(d=None) == bad and last(cam=None) == bad and last(o=None) == bad
    assert last(cam=cam_with(width=0)) == bad and last(cam=cam_with(width=W + 1)) == bad and last(cam=cam_with(fx=0.0)) == bad
    assert last(which=2) == bad and last(which=-1) == bad
    assert last(prm=capi.verify_params(tolerance=-1.0)) == bad and last(prm=capi.verify_params(use_slot_dims=1, slot_dims={7: (1.0, np.inf, 1.0)})) == bad
    assert bytes(out8) == untouched
    assert last() == capi.CD_OK and sum(out8[i].verified for i in range(8)) == res[0].n_clusters   # (the checks invalidated nothing)
