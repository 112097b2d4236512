"""Unregistered depth + colour pairs on the GPU (k_texture_map, cd_depth_to_cloud_mapped, cd_process_depth_batch_mapped[_device]):
the device mapping equals canonical rule C12 restated in numpy (perception_amd/texture_map.py) byte for byte, the chain on the
raw pairs is byte for byte cd_process_batch on the restatement's clouds, the registered special case is cd_process_depth_batch,
the colour gate and the overlay work on the raw colour images at their own size, and every refusal comes before anything runs.

cd_depth_to_cloud_mapped is a host call on ONE frame, so the shapes that need a batch or a device pointer (a pixel count that is
no multiple of the tile, frames smaller than a workgroup's stride, a device pointer off by 2 bytes) go through the fused calls
with the crops wide open and a 1 mm leaf, and are compared - records, indices and the voxel clouds read back, colours included -
with cd_process_batch fed the restatement's records."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rot_xyz
from perception_amd import capi, overlay, synth
from perception_amd import color_gate as cg
from perception_amd import texture_map as tm
from test_depth_cpu import synth_camera
from test_gpu_overlay import _record_poses, _records

pytestmark = pytest.mark.gpu
W, H = synth.WIDTH, synth.HEIGHT
P = W * H
NF = 8
BASELINE_X = 0.015


def _ccam(**kw):
    """The README's colour camera, 15 mm to the side and slightly turned."""
    kw.setdefault("R", rot_xyz(0.004, -0.006, 0.003))
    kw.setdefault("t", (BASELINE_X, -0.0007, 0.0003))
    return capi.color_camera(**kw)


@pytest.fixture(scope="module")
def pairs():
    cc = _ccam()
    fr = [synth.unregistered_frame(i, cc) for i in range(NF)]
    return np.stack([p[0] for p in fr]), np.stack([p[1] for p in fr]), cc


@pytest.fixture(scope="module")
def ctx(template):
    c = capi.Context(max_points=P, max_frames=NF)
    c.set_template(0, template)
    yield c
    c.close()


def _dev(depth, color, off_depth=0, off_color=0):
    """The images in HBM; off_* > 0 shifts the tensor by that many elements off its 16-byte aligned allocation."""
    d = torch.zeros(depth.size + 8, dtype=torch.int16, device="cuda")[off_depth:off_depth + depth.size].view(depth.shape)
    d.copy_(torch.from_numpy(depth.view(np.int16)))
    c = torch.zeros(color.size + 16, dtype=torch.uint8, device="cuda")[off_color:off_color + color.size].view(color.shape)
    c.copy_(torch.from_numpy(color))
    torch.cuda.synchronize()
    return d, c


def _readback(c, n_frames):
    out = []
    for f in range(n_frames):
        out.append(c.frame_cloud(f, capi.CD_CLOUD_VOXELS, 16, 12).tobytes())
        out.append(c.frame_cloud(f, capi.CD_CLOUD_OBJECTS, 16, 12).tobytes())
        out.append(b"".join(bytes(r) for r in c.cluster_results(f)))
    return out


def _open_params():
    prm = capi.default_params()
    prm.crop_z_min, prm.crop_z_max, prm.crop_x_min, prm.crop_x_max = -1e3, 1e3, -1e3, 1e3
    prm.crop2_enable = 0
    prm.leaf_size = 0.001
    return prm


def _random_pair(rng, w, h, cw, ch, F):
    depth = rng.integers(300, 900, (F, h, w)).astype(np.uint16)
    depth[rng.random((F, h, w)) < 0.1] = 0
    color = rng.integers(0, 256, (F, ch, cw, 3)).astype(np.uint8)
    return depth, color


@pytest.mark.parametrize("mode", [capi.CD_NOTEX_DROP, capi.CD_NOTEX_KEEP])
def test_depth_to_cloud_mapped_equals_the_restatement(ctx, pairs, mode):
    depth, rgb, cc0 = pairs
    rng = np.random.default_rng(31 + mode)
    # the synth pair, 640 x 480 -> 640 x 480, non-trivial R and t
    cam = synth_camera()
    cc = _ccam(no_texture=mode)
    for f in (0, 3):
        want, iu, iv, tex = tm.texture_map(depth[f], rgb[f], cam, cc)
        got = ctx.depth_to_cloud(cam, depth[f], rgb[f], color_camera=cc)
        assert np.array_equal(got, want), (mode, f)
        assert 0.3 < tex.mean() < 0.45 and len(np.unique(want[tex, 3])) >= 2
    # other record layouts
    got = ctx.depth_to_cloud(cam, depth[0], rgb[0], stride_bytes=32, rgb_offset=16, color_camera=cc)
    want = tm.texture_map(depth[0], rgb[0], cam, cc)[0]
    assert np.array_equal(got[:, :3], want[:, :3]) and np.array_equal(got[:, 4], want[:, 3]) and not got[:, [3, 5, 6, 7]].any()
    # random images: the identity pair of the README, 424 x 240 depth under a 640 x 480 colour image, 3 x 2 under 5 x 4, a larger
    # rotation with a colour image smaller than the depth image, and a colour camera behind the scene
    shapes = [
        (synth_camera(), capi.color_camera(no_texture=mode)),
        (synth_camera(424, 240), _ccam(no_texture=mode)),
        (synth_camera(3, 2), capi.color_camera(5, 4, K=(3.0, 3.0, 2.0, 1.5), t=(0.01, 0.0, 0.0), no_texture=mode)),
        (synth_camera(640, 480), capi.color_camera(320, 200, K=(300.0, 310.0, 150.0, 90.0), R=rot_xyz(0.1, -0.2, 0.3),
                                                  t=(0.05, -0.02, 0.01), no_texture=mode)),
        (synth_camera(67, 3), capi.color_camera(9, 7, K=(5.0, 5.0, 4.0, 3.0), t=(0.0, 0.0, -2.0), no_texture=mode)),
    ]
    for cam, cc in shapes:
        d, c3 = _random_pair(rng, cam.width, cam.height, cc.width, cc.height, 1)
        want, iu, iv, tex = tm.texture_map(d[0], c3[0], cam, cc)
        got = ctx.depth_to_cloud(cam, d[0], c3[0], color_camera=cc)
        assert np.array_equal(got, want), (mode, cam.width, cam.height, cc.width, cc.height)
    assert not tex.any()                                  # (the last camera sees nothing)
    # all-invalid and saturated depth
    cam, cc = synth_camera(), _ccam(no_texture=mode)
    for fill in (0, 65535):
        d = np.full((H, W), fill, np.uint16)
        assert np.array_equal(ctx.depth_to_cloud(cam, d, rgb[1], color_camera=cc), tm.texture_map(d, rgb[1], cam, cc)[0]), fill


def _chain_equals_cloud_batch(ctx, cam, cc, depth, color, prm, dev_offsets=((0, 0),)):
    """Host and device forms of the mapped call against cd_process_batch on the restatement's records."""
    F = depth.shape[0]
    n = cam.width * cam.height
    clouds = tm.texture_map(depth, color, cam, cc)[0].view(np.float32)
    q = capi.CdParams()
    C.memmove(C.byref(q), C.byref(prm), C.sizeof(q))
    q.rgb_offset = 12
    res_c, pi_c, lb_c = ctx.process_batch(clouds, q, want_indices=True)
    back_c = _readback(ctx, F)
    prm.rgb_offset = 40                                    # ignored by the mapped call
    res_h, pi_h, lb_h = ctx.process_depth_batch(depth, color, cam, prm, want_indices=True, color_camera=cc)
    assert bytes(res_h) == bytes(res_c) and np.array_equal(pi_h, pi_c) and np.array_equal(lb_h, lb_c)
    assert _readback(ctx, F) == back_c
    for od, oc in dev_offsets:
        td, tc = _dev(depth, color, od, oc)
        assert (td.data_ptr() % 16 != 0) == (od != 0)
        pi, lb = np.empty((F, n), np.int32), np.empty((F, n), np.int32)
        res_d = ctx.process_depth_batch_device(td, tc, cam, prm, plane_inliers=pi, labels=lb, color_camera=cc)
        assert bytes(res_d) == bytes(res_c) and np.array_equal(pi, pi_c) and np.array_equal(lb, lb_c), (od, oc)
        assert _readback(ctx, F) == back_c, (od, oc)
    return res_c


def test_mapped_batch_equals_cloud_batch(ctx, pairs):
    depth, rgb, cc = pairs
    cam = synth_camera()
    for mode in (capi.CD_NOTEX_DROP, capi.CD_NOTEX_KEEP):
        cc2 = _ccam(no_texture=mode)
        res = _chain_equals_cloud_batch(ctx, cam, cc2, depth, rgb, capi.default_params(), dev_offsets=((0, 0), (1, 3)))
        assert sum(r.n_clusters for r in res) >= NF and all(r.status == capi.CD_OK for r in res)
    prm = capi.default_params()
    prm.leaf_size = 0.001
    prm.plane_distance_threshold = 0.01
    _chain_equals_cloud_batch(ctx, cam, cc, depth, rgb, prm)


@pytest.mark.parametrize("shape", [(424, 240, 640, 480, 3), (3, 2, 5, 4, 7), (67, 3, 9, 7, 8), (300, 1, 33, 17, 5)])
def test_odd_batches_and_unaligned_device_pointers(ctx, shape):
    """Pixel counts that are no multiple of the 2048-pixel tile, frames smaller than the 256 pixels a lane steps by (a lane then
    crosses several frames in one step), and depth / colour tensors 2 bytes / 1 byte off their aligned allocation, which take
    the element-wise loads."""
    w, h, cw, ch, F = shape
    assert (w * h * F) % 2048 != 0
    rng = np.random.default_rng(w * 1000 + h)
    cam = synth_camera(w, h)
    K = synth.depth_camera_params(w, h)
    cam.fx, cam.fy, cam.cx, cam.cy = K
    cc = capi.color_camera(cw, ch, K=(K[0] * cw / w * 0.8, K[1] * ch / h * 0.8, cw / 2.0, ch / 2.0), R=rot_xyz(0.01, 0.02, -0.03),
                           t=(0.01, 0.002, -0.001))
    depth, color = _random_pair(rng, w, h, cw, ch, F)
    tex = tm.texture_map(depth, color, cam, cc)[3]
    assert all(tex[f].any() for f in range(F)) and not tex.all()
    _chain_equals_cloud_batch(ctx, cam, cc, depth, color, _open_params(), dev_offsets=((0, 0), (1, 1)))
    voxels = [ctx.frame_cloud(f, capi.CD_CLOUD_VOXELS, 16, 12) for f in range(F)]
    assert all(len(vx) > 0 for vx in voxels) and any(vx[:, 3].any() for vx in voxels)


def test_registered_special_case_equals_the_registered_call(ctx):
    cam = synth_camera()
    cc = capi.color_camera(cam.width, cam.height, K=(cam.fx, cam.fy, cam.cx, cam.cy))
    fr = [synth.depth_frame(i) for i in range(NF)]
    depth, rgb = np.stack([p[0] for p in fr]), np.stack([p[1] for p in fr])
    clusters = []
    for prm in (capi.default_params(), _open_params()):
        a = ctx.process_depth_batch(depth, rgb, cam, prm, want_indices=True)
        clusters.append(sum(r.n_clusters for r in a[0]))
        back_a = _readback(ctx, NF)
        b = ctx.process_depth_batch(depth, rgb, cam, prm, want_indices=True, color_camera=cc)
        assert bytes(a[0]) == bytes(b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert _readback(ctx, NF) == back_a
        td, tc = _dev(depth, rgb)
        assert bytes(ctx.process_depth_batch_device(td, tc, cam, prm, color_camera=cc)) == bytes(a[0])
    assert clusters[0] >= NF                               # (the default parameters find the boxes; the open crops need not)


def _color_P(cc, with_E=True):
    """CameraInfo.P of the colour camera, times the extrinsics E (4 x 4) when the caller wants them honoured."""
    Pm = np.array([[cc.fx, 0, cc.cx, 0], [0, cc.fy, cc.cy, 0], [0, 0, 1, 0]], np.float64)
    E = np.eye(4)
    E[:3, :3] = np.array(list(cc.R), np.float64).reshape(3, 3)
    E[:3, 3] = list(cc.t)
    return (Pm @ E if with_E else Pm), E


def test_colour_gate_on_the_raw_colour_images(ctx, pairs):
    depth, rgb, cc = pairs
    rgb = rgb.copy()
    rgb[5] = (150, 140, 130)                                # a frame without a red component
    cam = synth_camera()
    for with_E in (True, False):
        prm = capi.default_params()
        prm.bbox_enable = 1
        prm.bbox_P[:] = [float(x) for x in _color_P(cc, with_E)[0].ravel()]
        want = [cg.color_bbox(rgb[f]) for f in range(NF)]
        assert want[5]["found"] == 0 and sum(w["found"] for w in want) == NF - 1
        ctx.set_bbox_source(capi.CD_BBOX_COLOR)
        a = ctx.process_depth_batch(depth, rgb, cam, prm, want_indices=True, color_camera=cc)
        got = [{"rect": tuple(b.rect), "found": b.found, "area2": b.area2, "n_components": b.n_components, "n_mask": b.n_mask}
               for b in ctx.frame_bboxes()]
        assert got == want
        td, tc = _dev(depth, rgb)
        pi, lb = np.empty((NF, P), np.int32), np.empty((NF, P), np.int32)
        res_d = ctx.process_depth_batch_device(td, tc, cam, prm, plane_inliers=pi, labels=lb, color_camera=cc)
        assert bytes(res_d) == bytes(a[0]) and np.array_equal(pi, a[1]) and np.array_equal(lb, a[2])
        assert [tuple(b.rect) for b in ctx.frame_bboxes()] == [w["rect"] for w in want]
        # the same rectangles fed per frame to cd_process_batch on the restatement's clouds
        clouds = tm.texture_map(depth, rgb, cam, cc)[0].view(np.float32)
        ctx.set_frame_bboxes(np.array([w["rect"] for w in want], np.int32))
        ctx.set_bbox_source(capi.CD_BBOX_PER_FRAME)
        prm.rgb_offset = 12
        b = ctx.process_batch(clouds, prm, want_indices=True)
        assert bytes(a[0]) == bytes(b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        ctx.set_bbox_source(capi.CD_BBOX_PARAMS)
        assert a[0][5].n_objects == 0 and all(a[0][f].n_objects > 0 for f in range(NF) if f != 5)
        prm.bbox_enable = 0
        ungated = ctx.process_batch(clouds, prm)[0]
        assert any(a[0][f].n_objects != ungated[f].n_objects for f in range(NF))
    ctx.set_frame_bboxes(None)


def test_draw_last_results_on_the_colour_images(ctx):
    """A colour image of its own size (560 x 420): the boxes of a mapped device call drawn into it with P = the colour camera's
    and E = the extrinsics, against overlay.py."""
    F = 4
    cc = capi.color_camera(560, 420, K=(540.0, 539.0, 281.5, 209.0), R=rot_xyz(0.004, -0.006, 0.003), t=(BASELINE_X, -0.0007, 0.0003))
    fr = [synth.unregistered_frame(i, cc, k_obj=1) for i in range(F)]
    depth, rgb = np.stack([p[0] for p in fr]), np.stack([p[1] for p in fr])
    cam = synth_camera()
    Pm, E = _color_P(cc, with_E=False)
    kw = dict(P=Pm.ravel(), E=E, dims=synth.CUBOID_DIMS)
    params = capi.overlay_params(**kw)
    td, tc = _dev(depth, rgb)
    res = ctx.process_depth_batch_device(td, tc, cam, capi.default_params(), color_camera=cc)
    assert sum(r.n_clusters for r in res) >= F
    B = capi.CD_MAX_CLUSTERS_PER_FRAME
    poses, n = _record_poses(res, F, capi.CD_DRAW_ALL)
    want, wboxes, painted = overlay.draw(rgb, poses, n, **kw)
    boxes = ctx.draw_last_results(tc, capi.CD_DRAW_ALL, params)
    assert np.array_equal(_records(boxes, F, B), wboxes)
    assert np.array_equal(tc.cpu().numpy(), want) and painted.any(axis=(1, 2)).all()
    # the host form, after the host call
    res_h, _, _ = ctx.process_depth_batch(depth, rgb, cam, capi.default_params(), color_camera=cc)
    assert bytes(res_h) == bytes(res)
    img = np.array(rgb, copy=True)
    hboxes = ctx.draw_last_results(img, capi.CD_DRAW_ALL, params)
    assert bytes(hboxes) == bytes(boxes) and np.array_equal(img, want)
    # the extrinsics matter, and the boxes lie on the red pixels of the colour image: within 8 px = the 3.969 px corner error
    # measured at the depth K (tests/test_gpu_overlay.py) x 540 / 384 for the colour K, + 1 truncation + 1 half thickness
    ident = overlay.draw(rgb, poses, n, P=Pm.ravel(), dims=synth.CUBOID_DIMS)[2]
    assert not np.array_equal(ident, painted)
    red = (rgb[..., 0] == 200) & (rgb[..., 2] == 40)
    for f in range(F):
        ys, xs = np.nonzero(painted[f])
        ry, rx = np.nonzero(red[f])
        assert rx.min() - 8 <= xs.min() and xs.max() <= rx.max() + 8 and ry.min() - 8 <= ys.min() and ys.max() <= ry.max() + 8, f


def test_refusals(ctx, pairs):
    depth, rgb, cc = pairs
    cam = synth_camera()
    prm = capi.default_params()
    lib, h = ctx.lib, ctx.h
    ref = ctx.process_depth_batch(depth[:2], rgb[:2], cam, prm, color_camera=cc)[0]
    ref_bytes = bytes(ref)
    n_clusters = len(ctx.cluster_results(0))
    res = (capi.CdFrameResult * (NF + 1))()
    out = np.zeros((P, 4), np.uint32)
    n = C.c_int()
    td, tc = _dev(depth[:2], rgb[:2])
    host = (depth.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p))
    dev = (C.c_void_p(td.data_ptr()), C.c_void_p(tc.data_ptr()))

    def cam_with(**kw):
        c2 = synth_camera()
        for k, v in kw.items():
            setattr(c2, k, v)
        return c2

    def cc_with(**kw):
        c2 = _ccam()
        for k, v in kw.items():
            if k in ("R", "t"):
                getattr(c2, k)[v[0]] = v[1]
            else:
                setattr(c2, k, v)
        return c2

    D, Cc = "depth", "color"
    cases = [
        # everything check_depth refuses
        dict(null=D), dict(cam=cam_with(width=0)), dict(cam=cam_with(height=0)), dict(cam=cam_with(width=W + 1)),
        dict(nf=0), dict(nf=NF + 1), dict(cam=cam_with(color=2)), dict(null=Cc),
        dict(cam=cam_with(fx=float("nan"))), dict(cam=cam_with(fy=0.0)), dict(cam=cam_with(depth_scale=-0.001)),
        # the mapped call's own
        dict(cam=cam_with(color=capi.CD_COLOR_NONE)), dict(cc=None),
        dict(cc=cc_with(width=0)), dict(cc=cc_with(height=0)), dict(cc=cc_with(width=-640)), dict(cc=cc_with(width=W + 1)),
        dict(cc=cc_with(width=65536, height=65536)),
        dict(cc=cc_with(fx=0.0)), dict(cc=cc_with(fx=float("nan"))), dict(cc=cc_with(fy=-1.0)), dict(cc=cc_with(fy=float("inf"))),
        dict(cc=cc_with(R=(0, float("nan")))), dict(cc=cc_with(R=(8, float("inf")))), dict(cc=cc_with(t=(0, float("nan")))),
        dict(cc=cc_with(t=(2, float("-inf")))), dict(cc=cc_with(no_texture=2)), dict(cc=cc_with(no_texture=-1)),
    ]
    for i, case in enumerate(cases):
        c1, c2, nf = case.get("cam", cam), case.get("cc", cc), case.get("nf", 1)
        for fn, (dp, cp) in ((lib.cd_process_depth_batch_mapped, host), (lib.cd_process_depth_batch_mapped_device, dev)):
            st = fn(h, C.byref(c1), None if c2 is None else C.byref(c2), None if case.get("null") == D else dp,
                    None if case.get("null") == Cc else cp, nf, C.byref(prm), C.cast(res, C.c_void_p), None, None)
            assert st == capi.CD_ERR_INVALID_ARG, (i, case)
            assert lib.cd_last_error(h), i
        if nf == 1:
            st = lib.cd_depth_to_cloud_mapped(h, C.byref(c1), None if c2 is None else C.byref(c2), None if case.get("null") == D else host[0],
                                              None if case.get("null") == Cc else host[1], out.ctypes.data_as(C.c_void_p), 16, 12, P, C.byref(n))
            assert st == capi.CD_ERR_INVALID_ARG, (i, case)
    assert lib.cd_process_depth_batch_mapped(h, None, C.byref(cc), host[0], host[1], 1, C.byref(prm), C.cast(res, C.c_void_p), None, None) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_process_depth_batch_mapped(None, C.byref(cam), C.byref(cc), host[0], host[1], 1, C.byref(prm), C.cast(res, C.c_void_p), None, None) == capi.CD_ERR_INVALID_ARG
    assert not out.any() and not bytes(res).strip(b"\0")
    # nothing was launched or copied: the last batch's results are still there, and a valid call gives what it gave
    assert len(ctx.cluster_results(0)) == n_clusters
    again = ctx.process_depth_batch(depth[:2], rgb[:2], cam, prm, color_camera=cc)[0]
    assert bytes(again) == ref_bytes
    assert bytes(ctx.process_depth_batch_device(td, tc, cam, prm, color_camera=cc)) == ref_bytes
    # the gate's sources: CD_BBOX_COLOR is served, CD_BBOX_PER_FRAME without rectangles is refused as everywhere
    gated = capi.default_params()
    gated.bbox_enable = 1
    gated.bbox_P[:] = [float(x) for x in _color_P(cc)[0].ravel()]
    ctx.set_frame_bboxes(None)
    ctx.set_bbox_source(capi.CD_BBOX_PER_FRAME)
    with pytest.raises(capi.CuboidError) as e:
        ctx.process_depth_batch(depth[:2], rgb[:2], cam, gated, color_camera=cc)
    assert e.value.status == capi.CD_ERR_INVALID_ARG
    ctx.set_bbox_source(capi.CD_BBOX_PARAMS)
    # capacity of cd_depth_to_cloud_mapped's output
    st = lib.cd_depth_to_cloud_mapped(h, C.byref(cam), C.byref(cc), host[0], host[1], out.ctypes.data_as(C.c_void_p), 16, 12, P - 1, C.byref(n))
    assert st == capi.CD_ERR_CAPACITY and n.value == P
