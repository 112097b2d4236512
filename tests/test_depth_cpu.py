"""Depth-image input without a GPU: the cd_depth_camera mirror of the binding, and canonical rule C7 restated in
numpy - the contract the device deprojection (tests/test_gpu_depth.py) is held to bit for bit - checked against the clouds
synth renders directly."""
import ctypes as C

import numpy as np

from perception_amd import capi, synth

QNAN = np.uint32(0x7FC00000)


def deproject(depth, color, cam):
    """Rule C7: (H, W) uint16 depth (+ (H, W, 3) uint8 colour or None) -> (H * W, 4) uint32 records x y z rgb, float32
    arithmetic one IEEE operation at a time (numpy never contracts)."""
    h, w = depth.shape
    v, u = np.divmod(np.arange(h * w, dtype=np.int64), w)
    f32 = np.float32
    d = depth.reshape(-1)
    z = d.astype(f32) * f32(cam.depth_scale)
    x = ((u.astype(f32) - f32(cam.cx)) / f32(cam.fx)) * z
    y = ((v.astype(f32) - f32(cam.cy)) / f32(cam.fy)) * z
    out = np.empty((h * w, 4), np.uint32)
    out[:, 0], out[:, 1], out[:, 2] = x.view(np.uint32), y.view(np.uint32), z.view(np.uint32)
    out[d == 0, :3] = QNAN
    if color is None:
        out[:, 3] = 0
    else:
        c = color.reshape(-1, 3).astype(np.uint32)
        out[:, 3] = (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]
    return out


def synth_camera(width=synth.WIDTH, height=synth.HEIGHT, color=capi.CD_COLOR_RGB8, depth_scale=synth.DEPTH_SCALE):
    cam = capi.default_depth_camera()
    cam.width, cam.height = width, height
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params(width, height)
    cam.depth_scale = depth_scale
    cam.color = color
    return cam


def test_depth_camera_struct_matches_header():
    lib = capi.load_library()
    assert lib.cd_struct_size(4) == C.sizeof(capi.CdDepthCamera) == 32
    a = capi.CdDepthCamera()
    lib.cd_default_depth_camera(C.byref(a))
    b = capi.default_depth_camera()
    for name, _ in capi.CdDepthCamera._fields_:
        assert getattr(a, name) == getattr(b, name), name
    assert (a.width, a.height, a.color) == (640, 480, capi.CD_COLOR_NONE)


def test_synth_depth_frame_deprojects_to_the_rendered_cloud():
    for i in range(2):
        depth, rgb = synth.depth_frame(i)
        ref = synth.frame(i)
        assert depth.shape == (synth.HEIGHT, synth.WIDTH) and depth.dtype == np.uint16
        assert rgb.shape == (synth.HEIGHT, synth.WIDTH, 3) and rgb.dtype == np.uint8
        rec = deproject(depth, rgb, synth_camera())
        xyz = rec[:, :3].view(np.float32)
        bad = np.isnan(ref[:, 2])
        assert np.array_equal(np.isnan(xyz[:, 2]), bad) and np.array_equal(depth.reshape(-1) == 0, bad)
        assert (rec[bad, :3] == QNAN).all()
        assert np.array_equal(rec[:, 3], ref[:, 3].view(np.uint32))          # synth._pack_rgb's packing
        # xyz moves along the pixel's ray by the depth quantisation (0.5 mm at most)
        ray = np.linalg.norm(xyz[~bad].astype(np.float64) / xyz[~bad, 2:3].astype(np.float64), axis=1)
        err = np.linalg.norm(xyz[~bad].astype(np.float64) - ref[~bad, :3].astype(np.float64), axis=1)
        assert (err <= 0.0005 * ray + 1e-6).all(), err.max()
        dz = np.abs(xyz[~bad, 2].astype(np.float64) - ref[~bad, 2].astype(np.float64))
        assert dz.max() <= 0.0005 + 1e-6


def test_deproject_restatement_on_hand_made_pixels():
    cam = synth_camera(width=3, height=2, color=capi.CD_COLOR_RGB8, depth_scale=0.001)
    cam.fx, cam.fy, cam.cx, cam.cy = 2.0, 4.0, 1.0, 0.5
    depth = np.array([[1000, 0, 2000], [65535, 1, 500]], np.uint16)
    color = np.arange(18, dtype=np.uint8).reshape(2, 3, 3)
    rec = deproject(depth, color, cam)
    xyz = rec[:, :3].view(np.float32)
    assert (rec[1, :3] == QNAN).all() and rec[1, 3] == (3 << 16) | (4 << 8) | 5
    f32 = np.float32
    assert xyz[0].tolist() == [f32(-0.5) * f32(1.0), f32(-0.125) * f32(1.0), f32(1.0)]
    assert xyz[2, 0] == f32(0.5) * (f32(2000) * f32(0.001))
    assert xyz[3, 2] == f32(65535) * f32(0.001)
    assert (deproject(depth, None, cam)[:, 3] == 0).all()
