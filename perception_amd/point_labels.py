"""Canonical rule C15 restated in numpy: the label of every input point of a fused call, by provenance.

This module is the specification (include/cuboid_hip.h states the rule, DESIGN.md lists it): the device
(perception_amd/csrc/k_labels.hip, cd_label_points_last / cd_label_depth_last) equals labels_of_frame byte for byte when it is fed
that call's own outputs.  numpy only - no GPU, no library.

A point's voxel is the cell VoxelGrid put it in: floor(p * inv_leaf) - min_b in float32 with inv_leaf = 1.0f / leaf, numbered
idx = i + j dx + k dx dy; a voxel's number is the rank of its idx among the frame's occupied cells, which is the order of the
voxel cloud.  The voxel's class is read off the call's plane_inliers, object cloud and labels - no geometry is tested again.
"""
import numpy as np

LABEL_INVALID, LABEL_CROPPED, LABEL_PLANE, LABEL_OBJECT, LABEL_GATED, LABEL_CLUSTER0 = 0, 1, 2, 3, 4, 8
MAX_RANKS = 256 - LABEL_CLUSTER0      # cluster ranks 0 .. 247 have a label of their own

# the default palette of cd_tint_labels_batch
_CLUSTER_RGB = [(230, 25, 75), (60, 180, 75), (0, 130, 200), (255, 225, 25), (145, 30, 180), (70, 240, 240), (240, 50, 230), (170, 110, 40)]


def default_palette():
    """(256, 4) uint8, r g b alpha per label: alpha 0 for INVALID, CROPPED and the reserved values, a grey for the plane, orange
    for OBJECT, a dark red for GATED, eight cluster colours that repeat with the rank."""
    pal = np.zeros((256, 4), np.uint8)
    pal[LABEL_PLANE] = (128, 128, 128, 96)
    pal[LABEL_OBJECT] = (255, 165, 0, 128)
    pal[LABEL_GATED] = (139, 0, 0, 128)
    for r in range(MAX_RANKS):
        pal[LABEL_CLUSTER0 + r] = _CLUSTER_RGB[r % 8] + (160,)
    return pal


def deproject(depth, cam):
    """Rule C7 for one (H, W) uint16 image: the (H * W, 3) float32 cloud in record order, NaN where the depth value is 0."""
    d = np.asarray(depth)
    H, W = d.shape
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    z = d.astype(np.float32) * np.float32(cam.depth_scale)
    x = ((u - np.float32(cam.cx)) / np.float32(cam.fx)) * z
    y = ((v - np.float32(cam.cy)) / np.float32(cam.fy)) * z
    out = np.stack([x, y, z], -1).astype(np.float32)
    out[d == 0] = np.nan
    return out.reshape(-1, 3)


def kept_by_crop(xyz, prm):
    """(finite, kept): the S0 predicate - finite, then the z limits, then the x limits, double limits, both inclusive."""
    p = np.asarray(xyz, np.float32)
    fin = np.isfinite(p).all(1)
    x, z = p[:, 0].astype(np.float64), p[:, 2].astype(np.float64)
    with np.errstate(invalid="ignore"):
        kept = fin & (z >= prm.crop_z_min) & (z <= prm.crop_z_max) & (x >= prm.crop_x_min) & (x <= prm.crop_x_max)
    return fin, kept


def voxel_numbers(kept_xyz, leaf):
    """Voxel number of every kept point and the number of occupied cells (the arithmetic of VoxelGrid::applyFilter)."""
    inv = np.float32(1.0) / np.float32(leaf)
    fl = np.floor(np.asarray(kept_xyz, np.float32) * inv)                 # float32, one operation each
    min_b = fl.min(0)                                                      # floor(min * inv): floor and * inv are monotone
    ijk = (fl - min_b).astype(np.int64)                                    # (int)(floor(p * inv) - min_b), the subtraction in float32
    div = fl.max(0).astype(np.int64) - min_b.astype(np.int64) + 1
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    uniq, number = np.unique(idx, return_inverse=True)
    return number.reshape(-1), len(uniq)


def object_voxels(voxels, objects):
    """Voxel of every object point: the object cloud walked as an order-preserving subsequence of the voxel cloud, matched on
    the 12 bytes of xyz."""
    vb = np.ascontiguousarray(np.asarray(voxels, np.float32)[:, :3]).view(np.uint32).reshape(-1, 3)
    ob = np.ascontiguousarray(np.asarray(objects, np.float32)[:, :3]).view(np.uint32).reshape(-1, 3)
    out = np.empty(len(ob), np.int64)
    v = 0
    for j in range(len(ob)):
        while v < len(vb) and not (vb[v, 0] == ob[j, 0] and vb[v, 1] == ob[j, 1] and vb[v, 2] == ob[j, 2]):
            v += 1
        assert v < len(vb), "the object cloud is not a subsequence of the voxel cloud"
        out[j] = v
        v += 1
    return out


def voxel_classes(n_voxels, plane_inliers, voxels, objects, labels):
    """uint8[n_voxels]: GATED, then PLANE for the refined inliers, then OBJECT / CLUSTER0 + r for the voxels of the object cloud."""
    cls = np.full(n_voxels, LABEL_GATED, np.uint8)
    cls[np.asarray(plane_inliers, np.int64)] = LABEL_PLANE
    ov = object_voxels(voxels, objects)
    lab = np.asarray(labels, np.int64)[:len(ov)]
    cls[ov] = np.where((lab >= 0) & (lab < MAX_RANKS), LABEL_CLUSTER0 + lab, LABEL_OBJECT).astype(np.uint8)
    return cls


def labels_of_frame(points, prm, n_voxels, plane_inliers, voxels, objects, labels):
    """uint8[n]: rule C15 for the n input records `points` ((n, >= 3) float32) of one frame of a fused call run with `prm`,
    from that call's outputs for the frame: n_voxels, the plane_inliers (indices into the voxel cloud), the voxel cloud, the
    object cloud and its per-point cluster labels."""
    p = np.asarray(points, np.float32)[:, :3]
    out = np.full(len(p), LABEL_INVALID, np.uint8)
    fin, kept = kept_by_crop(p, prm)
    out[fin & ~kept] = LABEL_CROPPED
    if not kept.any():
        assert n_voxels == 0
        return out
    if n_voxels == 0:          # the frame's chain ended in the voxel stage (CD_ERR_LEAF_TOO_SMALL): no voxel, no class
        out[kept] = LABEL_GATED
        return out
    number, occupied = voxel_numbers(p[kept], prm.leaf_size)
    assert occupied == n_voxels, "occupied cells %d != n_voxels %d" % (occupied, n_voxels)
    out[kept] = voxel_classes(n_voxels, plane_inliers, voxels, objects, labels)[number]
    return out


def tint(rgb8, labels, palette=None):
    """cd_tint_labels_batch: c' = (c (255 - a) + p a + 127) / 255 in integers, (p, a) from palette[label].  rgb8 (..., 3) uint8,
    labels its leading shape; returns a new array."""
    pal = default_palette() if palette is None else np.asarray(palette, np.uint8).reshape(256, 4)
    c = np.asarray(rgb8, np.uint8).astype(np.uint32)
    e = pal[np.asarray(labels, np.uint8)].astype(np.uint32)
    a = e[..., 3:4]
    return ((c * (255 - a) + e[..., :3] * a + 127) // 255).astype(np.uint8)
