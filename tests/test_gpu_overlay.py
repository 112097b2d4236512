"""The overlay on the GPU (k_overlay.hip, cd_draw_boxes_batch[_device], cd_draw_last_results[_device]): the drawn images equal
canonical rule C11 restated in numpy (perception_amd/overlay.py) byte for byte, the host, device and one-frame-per-call forms
agree, nothing but the painted pixels changes, the last fused call's poses are drawn as its records state them and stay as
they were, every argument check refuses before anything runs, and the boxes drawn for accepted single-box frames lie where
synth put the cuboids."""
import ctypes as C

import numpy as np
import pytest
import torch

from perception_amd import capi, overlay, synth
from test_depth_cpu import synth_camera

pytestmark = pytest.mark.gpu
W, H = synth.WIDTH, synth.HEIGHT
NF = 16
FX, FY, CX, CY = synth.depth_camera_params()
SYNTH_P = (FX, 0.0, CX, 0.0, 0.0, FY, CY, 0.0, 0.0, 0.0, 1.0, 0.0)
NAN_POSE = np.full((4, 4), np.nan)

# Behaviour test: `python tools/overlay_tolerance.py --frames 16` (CPU oracle alone) prints 3.969 px as the largest corner error
# over single-box synth frames 0..15, all of them accepted; plus one pixel for the truncation of step 3 (rule C11).
# No frame of the range is left out.
BEHAVIOUR_FRAMES = tuple(range(16))
BEHAVIOUR_TOL_PX = 3.969 + 1.0


@pytest.fixture(scope="module")
def ctx(template):
    c = capi.Context(max_points=W * H, max_frames=NF)
    c.set_template(0, template)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rgb6():
    return np.stack([synth.depth_frame(i)[1] for i in range(6)])


def _shift(T, dx=0.0, dy=0.0, dz=0.0):
    T = np.array(T, np.float64)
    T[:3, 3] += (dx, dy, dz)
    return T


def _scene_poses():
    """(6, 3, 4, 4) poses and n_boxes: frames with 0, 1 and 3 boxes, overlapping boxes, a box partly and a box wholly outside the
    image, a skipped box among drawn ones, and valid poses in slots beyond n_boxes that must not be drawn."""
    t = [synth.truth_poses(synth.scene_for(i, k_obj=3)) for i in range(6)]
    poses = np.empty((6, 3, 4, 4))
    for f in range(6):
        poses[f] = np.stack(t[f])
    n = np.array([0, 1, 3, 3, 2, 3], np.int32)
    poses[3, 1] = _shift(poses[3, 0], dx=0.02, dy=0.01)          # overlaps box 0
    poses[3, 2] = _shift(poses[3, 0], dx=0.45)                   # crosses the right border
    poses[4, 0] = _shift(poses[4, 0], dx=-3.0)                   # wholly outside (left), |pixel| < 8192
    poses[4, 1] = _shift(poses[4, 1], dy=-0.38)                  # crosses the top border
    poses[5, 1] = NAN_POSE                                       # skipped, between two drawn boxes
    return poses, n


def _records(boxes, F, B):
    a = np.frombuffer(bytes(boxes), np.int32).reshape(-1, 20)[:F * B]
    assert not a[:, 17:].any()
    return a[:, :17].reshape(F, B, 17)


def _check(ctx, imgs, poses, n_boxes, what="", **kw):
    """Draw on a copy with the host form and compare with the restatement: images, box records, untouched bytes."""
    want, wboxes, painted = overlay.draw(imgs, poses, n_boxes, **kw)
    got = np.array(imgs, copy=True)
    params = capi.overlay_params(**kw)
    boxes = ctx.draw_boxes(got, poses, n_boxes, params)
    F, B = wboxes.shape[:2]
    assert np.array_equal(_records(boxes, F, B), wboxes), what
    assert np.array_equal(got[~painted], np.asarray(imgs)[~painted]), what + ": a byte outside the painted set changed"
    assert (got[painted] == np.asarray(kw.get("rgb", overlay.DEFAULT_RGB), np.uint8)).all(), what
    assert np.array_equal(got, want), what
    return got, wboxes, painted


@pytest.mark.parametrize("thickness", [1, 2, 5])
def test_drawn_images_equal_the_restatement(ctx, rgb6, thickness):
    poses, n = _scene_poses()
    got, boxes, painted = _check(ctx, rgb6, poses, n, what="t=%d" % thickness, P=SYNTH_P, dims=synth.CUBOID_DIMS, thickness=thickness)
    assert boxes[..., 16].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 1], [1, 1, 1], [1, 1, 0], [1, 0, 1]]
    assert not painted[0].any() and np.array_equal(got[0], rgb6[0])
    assert painted[1].any() and painted[2].sum() > painted[1].sum()
    assert painted[3, :, W - 1].any() and painted[4, 0, :].any()         # the boxes that cross a border reach it
    if thickness > 1:
        thin = overlay.draw(rgb6, poses, n, P=SYNTH_P, dims=synth.CUBOID_DIMS, thickness=1)[2]
        assert painted.sum() > thin.sum() and painted[thin].all()


def test_colour_and_extrinsics(ctx, rgb6):
    poses, n = _scene_poses()
    _check(ctx, rgb6, poses, n, what="colour", P=SYNTH_P, dims=synth.CUBOID_DIMS, rgb=(17, 3, 250))
    E = np.eye(4)
    c, s = np.cos(0.05), np.sin(0.05)
    E[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    E[:3, 3] = (0.015, -0.004, 0.002)
    a = _check(ctx, rgb6, poses, n, what="E", P=SYNTH_P, E=E, dims=synth.CUBOID_DIMS)
    b = _check(ctx, rgb6, poses, n, what="identity", P=SYNTH_P, dims=synth.CUBOID_DIMS)
    assert not np.array_equal(a[1], b[1])
    _check(ctx, rgb6, poses, n, what="defaults")      # the D435 P of the defaults
    got = np.array(rgb6, copy=True)
    ctx.draw_boxes(got, poses, n, None)               # params == NULL
    assert np.array_equal(got, overlay.draw(rgb6, poses, n)[0])


def test_small_images(ctx):
    rng = np.random.default_rng(3)
    eye_P = (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0)
    one = rng.integers(0, 256, (3, 1, 1, 3)).astype(np.uint8)
    T = np.eye(4)
    T[:3, 3] = (0.0, 0.0, 1.0)
    poses = np.stack([T, _shift(T, dx=9.0), NAN_POSE])[:, None]
    got, boxes, painted = _check(ctx, one, poses, None, what="1x1", P=eye_P, dims=(0.5, 0.5, 0.5), thickness=1)
    assert painted.reshape(3).tolist() == [True, False, False] and boxes[:, 0, 16].tolist() == [1, 1, 0]
    _check(ctx, one, poses, None, what="1x1 thick", P=eye_P, dims=(0.5, 0.5, 0.5), thickness=64)
    w, h = 97, 61
    img = rng.integers(0, 256, (5, h, w, 3)).astype(np.uint8)
    P = (70.0, 0.0, 48.3, 0.0, 0.0, 70.0, 30.1, 0.0, 0.0, 0.0, 1.0, 0.0)
    from conftest import rot_xyz
    poses = np.empty((5, 4, 4, 4))
    for f in range(5):
        for b in range(4):
            Tb = np.eye(4)
            Tb[:3, :3] = rot_xyz(*rng.uniform(-np.pi, np.pi, 3))
            Tb[:3, 3] = rng.uniform((-0.5, -0.4, 0.5), (0.5, 0.4, 1.5))
            poses[f, b] = Tb
    for t in (1, 2, 5, 11):
        _, boxes, painted = _check(ctx, img, poses, [4, 3, 0, 1, 4], what="97x61 t=%d" % t, P=P, dims=(0.4, 0.2, 0.1), thickness=t)
    assert painted.any(axis=(1, 2)).tolist() == [True, True, False, True, True]


def test_host_device_and_batch_forms_agree(ctx, rgb6):
    poses, n = _scene_poses()
    params = capi.overlay_params(P=SYNTH_P, dims=synth.CUBOID_DIMS, thickness=3)
    host = np.array(rgb6, copy=True)
    hb = ctx.draw_boxes(host, poses, n, params)
    t = torch.from_numpy(rgb6).cuda()
    torch.cuda.synchronize()
    db = ctx.draw_boxes(t, poses, n, params)
    assert bytes(db) == bytes(hb)
    assert np.array_equal(t.cpu().numpy(), host)
    for f in range(6):
        one = np.array(rgb6[f:f + 1], copy=True)
        ob = ctx.draw_boxes(one, poses[f:f + 1], n[f:f + 1], params)
        assert np.array_equal(one[0], host[f]), f
        assert bytes(ob)[:3 * 80] == bytes(hb)[f * 3 * 80:(f + 1) * 3 * 80], f
    # a second draw on drawn images repaints the same pixels
    again = np.array(host, copy=True)
    ctx.draw_boxes(again, poses, n, params)
    assert np.array_equal(again, host)


def _record_poses(res, F, which):
    B = capi.CD_MAX_CLUSTERS_PER_FRAME
    poses = np.full((F, B, 4, 4), np.nan)
    n = np.zeros(F, np.int32)
    for f in range(F):
        n[f] = min(res[f].n_clusters, B)
        for k in range(n[f]):
            if which == capi.CD_DRAW_ALL or res[f].clusters[k].accepted:
                poses[f, k] = np.array(res[f].clusters[k].pose).reshape(4, 4)
    return poses, n


def test_draw_last_results_after_a_depth_batch(ctx, prm, template):
    F = 4
    pairs = [synth.depth_frame(i) for i in range(F)]
    depth, rgb = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    cam = synth_camera()
    strict = capi.default_params()
    strict.icp_accept_fitness = 7.3e-6     # between the fitnesses of these frames' clusters: ACCEPTED and ALL differ
    res, _, _ = ctx.process_depth_batch(depth, rgb, cam, strict)
    before = bytes(capi.results_to_array(res).tobytes())
    acc = [[res[f].clusters[k].accepted for k in range(res[f].n_clusters)] for f in range(F)]
    assert any(a for fr in acc for a in fr) and any(not a for fr in acc for a in fr), acc
    clusters_before = [bytes(c) for f in range(F) for c in ctx.cluster_results(f)]
    params = capi.overlay_params(P=SYNTH_P, dims=synth.CUBOID_DIMS)
    B = capi.CD_MAX_CLUSTERS_PER_FRAME
    drawn = {}
    for which in (capi.CD_DRAW_ACCEPTED, capi.CD_DRAW_ALL):
        poses, n = _record_poses(res, F, which)
        want, wboxes, painted = overlay.draw(rgb, poses, n, P=SYNTH_P, dims=synth.CUBOID_DIMS)
        got = np.array(rgb, copy=True)
        boxes = ctx.draw_last_results(got, which, params)
        assert np.array_equal(_records(boxes, F, B), wboxes), which
        assert np.array_equal(got, want), which
        assert np.array_equal(got[~painted], rgb[~painted])
        t = torch.from_numpy(rgb).cuda()
        torch.cuda.synchronize()
        dboxes = ctx.draw_last_results(t, which, params)
        assert bytes(dboxes) == bytes(boxes) and np.array_equal(t.cpu().numpy(), want), which
        drawn[which] = int(wboxes[..., 16].sum())
    assert 0 < drawn[capi.CD_DRAW_ACCEPTED] < drawn[capi.CD_DRAW_ALL] == sum(len(a) for a in acc)
    # drawing left the fused call's records and read-backs as they were
    assert bytes(capi.results_to_array(res).tobytes()) == before
    assert [bytes(c) for f in range(F) for c in ctx.cluster_results(f)] == clusters_before
    assert len(ctx.frame_cloud(0, capi.CD_CLOUD_OBJECTS)) == res[0].n_objects
    # the device form on the images of the _device fused call: same records, same picture
    td = torch.from_numpy(depth.view(np.int16)).cuda().view(torch.uint16)
    tc = torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()
    res2 = ctx.process_depth_batch_device(td, tc, cam, strict)
    assert bytes(capi.results_to_array(res2).tobytes()) == before
    ctx.draw_last_results(tc, capi.CD_DRAW_ALL, params)
    assert np.array_equal(tc.cpu().numpy(), want)
    # another compute call in between: nothing to draw any more, and nothing is drawn
    ctx.icp(0, template[:600], prm)
    img = np.array(rgb, copy=True)
    with pytest.raises(capi.CuboidError) as e:
        ctx.draw_last_results(img, capi.CD_DRAW_ALL, params)
    assert e.value.status == capi.CD_ERR_INVALID_ARG and np.array_equal(img, rgb)
    with pytest.raises(capi.CuboidError) as e:
        ctx.draw_last_results(tc, capi.CD_DRAW_ALL, params)
    assert e.value.status == capi.CD_ERR_INVALID_ARG
    # ... and cd_draw_boxes_batch is such a compute call
    ctx.process_depth_batch(depth, rgb, cam, strict)
    ctx.draw_boxes(np.array(rgb[:1], copy=True), np.eye(4)[None, None], None, params)
    with pytest.raises(capi.CuboidError):
        ctx.draw_last_results(img, capi.CD_DRAW_ALL, params)


def test_draw_last_results_without_a_fused_call():
    c = capi.Context(max_points=64 * 48, max_frames=2)
    img = np.zeros((1, 48, 64, 3), np.uint8)
    with pytest.raises(capi.CuboidError) as e:
        c.draw_last_results(img)
    assert e.value.status == capi.CD_ERR_INVALID_ARG and not img.any()
    c.close()


def test_argument_checks(ctx, rgb6):
    lib, h = ctx.lib, ctx.h
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    img = np.array(rgb6[:2], copy=True)
    poses = np.ascontiguousarray(np.stack(synth.truth_poses(synth.scene_for(0, k_obj=3)))[None].repeat(2, 0))
    n = np.array([3, 2], np.int32)
    out = (capi.CdOverlayBox * 6)()
    good = capi.overlay_params(P=SYNTH_P)

    def call(rgb=img, w=W, hh=H, F=2, p=poses, nb=n, B=3, prm=good, o=out, fn=lib.cd_draw_boxes_batch):
        return fn(h, None if rgb is None else rgb.ctypes.data_as(C.c_void_p), w, hh, F, None if p is None else p.ctypes.data_as(dp),
                  None if nb is None else nb.ctypes.data_as(ip), B, None if prm is None else C.byref(prm), o)

    bad = capi.CD_ERR_INVALID_ARG
    assert call(rgb=None) == bad and call(p=None) == bad and call(nb=None) == bad and call(o=None) == bad
    assert call(w=0) == bad and call(hh=0) == bad and call(w=-4) == bad
    assert call(w=W + 1, hh=H) == bad                          # width * height over max_points
    assert call(w=8193, hh=1) == bad and call(w=1, hh=8193) == bad   # (8193 pixels fit the context: the side is what is refused)
    assert call(F=0) == bad and call(F=-1) == bad and call(F=NF + 1) == bad
    assert call(B=0) == bad and call(B=1025) == bad
    for t in (0, -1, 65):
        assert call(prm=capi.overlay_params(P=SYNTH_P, thickness=t)) == bad, t
    for field, idx in (("P", 0), ("P", 11), ("E", 3), ("E", 15), ("dims", 2)):
        for v in (np.nan, np.inf, -np.inf):
            o = capi.overlay_params(P=SYNTH_P)
            getattr(o, field)[idx] = v
            assert call(prm=o) == bad, (field, idx, v)
    assert call(nb=np.array([3, -1], np.int32)) == bad and call(nb=np.array([4, 0], np.int32)) == bad
    assert np.array_equal(img, rgb6[:2]), "a refused call drew something"
    assert lib.cd_draw_boxes_batch(None, None, W, H, 2, None, None, 3, None, None) == bad
    t = torch.from_numpy(rgb6[:2]).cuda()
    torch.cuda.synchronize()
    dev = lambda **kw: lib.cd_draw_boxes_batch_device(
        h, C.c_void_p(t.data_ptr()), kw.get("w", W), H, 2, poses.ctypes.data_as(dp), n.ctypes.data_as(ip), 3,
        C.byref(kw.get("prm", good)), out)
    assert dev(w=8193) == bad and dev(prm=capi.overlay_params(thickness=0)) == bad
    assert np.array_equal(t.cpu().numpy(), rgb6[:2])
    # a non-finite pose is not an error; the maximum thickness and the boundary counts are accepted
    poses2 = poses.copy()
    poses2[0, 1, 2, 3] = np.inf
    assert call(p=poses2, prm=capi.overlay_params(P=SYNTH_P, thickness=64), nb=np.array([3, 0], np.int32)) == capi.CD_OK
    assert [out[i].drawn for i in range(6)] == [1, 0, 1, 0, 0, 0]
    # cd_draw_last_results: the same checks on what it takes
    res, _, _ = ctx.process_batch(synth.frame(0)[None], capi.default_params())
    one = np.array(rgb6[:1], copy=True)
    out8 = (capi.CdOverlayBox * 8)()
    last = lambda rgb=one, w=W, hh=H, which=capi.CD_DRAW_ALL, prm=good, o=out8: lib.cd_draw_last_results(
        h, None if rgb is None else rgb.ctypes.data_as(C.c_void_p), w, hh, which, C.byref(prm), o)
    assert last(rgb=None) == bad and last(o=None) == bad and last(w=0) == bad and last(w=W + 1) == bad and last(w=8193, hh=1) == bad
    assert last(which=2) == bad and last(which=-1) == bad
    assert last(prm=capi.overlay_params(thickness=65)) == bad
    assert np.array_equal(one, rgb6[:1])
    assert last() == capi.CD_OK and sum(out8[i].drawn for i in range(8)) == res[0].n_clusters   # (the checks invalidated nothing)


def test_drawn_boxes_lie_where_synth_put_the_cuboids(ctx, prm):
    """Single-box synth frames 0..15, every one accepted by the chain: each drawn corner within BEHAVIOUR_TOL_PX (per axis) of the
    projection of synth.truth_poses, minimised over the box's 180-degree symmetries (overlay.corner_error_px)."""
    F = len(BEHAVIOUR_FRAMES)
    clouds = np.stack([synth.frame(i, k_obj=1) for i in BEHAVIOUR_FRAMES])
    rgb = np.stack([synth.depth_frame(i, k_obj=1)[1] for i in BEHAVIOUR_FRAMES])
    res, _, _ = ctx.process_batch(clouds, prm)
    params = capi.overlay_params(P=SYNTH_P, dims=synth.CUBOID_DIMS)
    img = np.array(rgb, copy=True)
    boxes = _records(ctx.draw_last_results(img, capi.CD_DRAW_ACCEPTED, params), F, capi.CD_MAX_CLUSTERS_PER_FRAME)
    errs = []
    for j, i in enumerate(BEHAVIOUR_FRAMES):
        assert res[j].n_clusters == 1 and res[j].clusters[0].accepted, i
        assert boxes[j, 0, 16] == 1 and not boxes[j, 1:].any(), i
        truth = synth.truth_poses(synth.scene_for(i, k_obj=1))[0]
        errs.append(overlay.corner_error_px(boxes[j, 0, :16], truth, P=SYNTH_P, dims=synth.CUBOID_DIMS))
        assert (img[j] != rgb[j]).any(), i
    print("corner errors (px):", ["%.3f" % e for e in errs])
    assert max(errs) <= BEHAVIOUR_TOL_PX, errs
