"""Canonical rule C12 restated in numpy: an unregistered depth image + the colour camera's image and the
depth -> colour extrinsics -> the coloured organized cloud, in the depth camera's frame.  This is the contract the device
mapping (k_texture.hip) and the host entry cd_texture_project are held to bit for bit.  float32 arithmetic, one IEEE operation
at a time (numpy never contracts); no occlusion test, no lens distortion.
"""
import numpy as np

QNAN = np.uint32(0x7FC00000)
CD_NOTEX_DROP, CD_NOTEX_KEEP = 0, 1


def project(depth, cam, ccam):
    """Steps 1-5 and the xyz of step 6 for every pixel of depth (H, W) or (F, H, W) uint16: (xyz float32 (..., H * W, 3),
    iu int32, iv int32, textured bool), each (..., H * W); iu = iv = -1 where the point is not textured.  cam / ccam: anything
    with the fields of cd_depth_camera / cd_color_camera."""
    f32 = np.float32
    depth = np.asarray(depth, np.uint16)
    h, w = depth.shape[-2:]
    d = depth.reshape(depth.shape[:-2] + (h * w,))
    v, u = np.divmod(np.arange(h * w, dtype=np.int64), w)
    R = [f32(x) for x in ccam.R]
    t = [f32(x) for x in ccam.t]
    with np.errstate(all="ignore"):
        z = d.astype(f32) * f32(cam.depth_scale)
        x = ((u.astype(f32) - f32(cam.cx)) / f32(cam.fx)) * z
        y = ((v.astype(f32) - f32(cam.cy)) / f32(cam.fy)) * z
        xc = ((R[0] * x + R[1] * y) + R[2] * z) + t[0]
        yc = ((R[3] * x + R[4] * y) + R[5] * z) + t[1]
        zc = ((R[6] * x + R[7] * y) + R[8] * z) + t[2]
        pu = (xc / zc) * f32(ccam.fx) + f32(ccam.cx)
        pv = (yc / zc) * f32(ccam.fy) + f32(ccam.cy)
        fu = np.floor(pu + f32(0.5)).astype(np.float64)     # (the bounds are compared in double, where an int32 size is exact)
        fv = np.floor(pv + f32(0.5)).astype(np.float64)
        tex = (d != 0) & (zc > 0) & np.isfinite(pu) & np.isfinite(pv) & (fu >= 0) & (fu < int(ccam.width)) & (fv >= 0) & (fv < int(ccam.height))
        iu = np.where(tex, fu, -1.0).astype(np.int32)
        iv = np.where(tex, fv, -1.0).astype(np.int32)
    xyz = np.stack([x, y, z], axis=-1)
    assert xyz.dtype == np.float32 and pu.dtype == np.float32
    gone = (d == 0) if int(ccam.no_texture) == CD_NOTEX_KEEP else ~tex
    xyz.view(np.uint32)[gone] = QNAN
    return xyz, iu, iv, tex


def texture_map(depth, color, cam, ccam):
    """Rule C12 on depth (H, W) [or a batch (F, H, W)] uint16 and color (ch, cw, 3) [(F, ch, cw, 3)] uint8: the records
    (H * W, 4) [(F, H * W, 4)] uint32 x y z rgb, and iu, iv, textured as project() returns them."""
    depth = np.asarray(depth, np.uint16)
    color = np.asarray(color, np.uint8)
    batch = depth.ndim == 3
    d3 = depth if batch else depth[None]
    c4 = color if batch else color[None]
    assert c4.shape == (d3.shape[0], int(ccam.height), int(ccam.width), 3), c4.shape
    xyz, iu, iv, tex = project(d3, cam, ccam)
    F, P = xyz.shape[:2]
    rec = np.zeros((F, P, 4), np.uint32)
    rec[:, :, :3] = xyz.view(np.uint32)
    for f in range(F):
        m = tex[f]
        c = c4[f][iv[f][m], iu[f][m]].astype(np.uint32)
        rec[f, m, 3] = (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]
    if not batch:
        return rec[0], iu[0], iv[0], tex[0]
    return rec, iu, iv, tex
