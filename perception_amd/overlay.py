"""Canonical rule C11 restated in plain Python / numpy: the projected ICP box that
cuboid_detection/scripts/draw_bbox.py:44-83 draws over the colour image.

This is the CPU statement of what perception_amd/csrc/k_overlay.hip computes on the device and cd_overlay_project on the
host; the tests require both to equal it bit for bit (corners, drawn flags) and byte for byte (images).  Nothing here is on
a hot path.  OpenCV is not a dependency: parity with a real cv2.line (its fixed-point thick-line polygon) is unpinned.
"""
import numpy as np

COORD_MAX = 8192          # |pixel coordinate| of a drawn box, and the largest image side
MAX_THICKNESS = 64
# the 12 corner pairs of draw_bbox.py:66-77, in that order
EDGES = ((0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7))

# cd_default_overlay_params: the D435 K of the reference's README.md:78 (float32 values, as cd_default_depth_camera holds them)
DEFAULT_P = (float(np.float32(384.0898742675781)), 0.0, float(np.float32(322.4656677246094)), 0.0,
             0.0, float(np.float32(384.0898742675781)), float(np.float32(240.64073181152344)), 0.0,
             0.0, 0.0, 1.0, 0.0)
DEFAULT_E = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)
DEFAULT_DIMS = (0.2, 0.1, 0.03)
DEFAULT_THICKNESS = 2
DEFAULT_RGB = (0, 255, 0)


def corners(pose, dims=DEFAULT_DIMS):
    """Step 1: cd_bbox_corners(pose, l, w, h) - (8, 3) float32, the order of icp.cpp:99-106."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        H = np.asarray(pose, np.float64).reshape(16).astype(f32)
        out = np.empty((8, 3), f32)
        for k in range(8):
            sx, sy, sz = (1.0 if k & 4 else -1.0), (1.0 if k & 2 else -1.0), (1.0 if k & 1 else -1.0)
            x, y, z = f32(sx * float(dims[0]) / 2), f32(sy * float(dims[1]) / 2), f32(sz * float(dims[2]) / 2)
            for r in range(3):
                out[k, r] = ((H[4 * r] * x + H[4 * r + 1] * y) + H[4 * r + 2] * z) + H[4 * r + 3]
    return out


def matrix(P=DEFAULT_P, E=DEFAULT_E):
    """Step 2: M = P E as 12 Python floats, every entry ((p0 e0 + p1 e1) + p2 e2) + p3 e3."""
    P = [float(v) for v in np.asarray(P, np.float64).reshape(12)]
    E = [float(v) for v in np.asarray(E, np.float64).reshape(16)]
    return [((P[4 * r] * E[c] + P[4 * r + 1] * E[4 + c]) + P[4 * r + 2] * E[8 + c]) + P[4 * r + 3] * E[12 + c]
            for r in range(3) for c in range(4)]


def project_point(M, xyz):
    """Steps 3 and 4 for one point (three floats, taken as doubles): (u, v) pixel or None when it makes its box a skipped one."""
    x, y, z = (float(v) for v in xyz)
    h = [((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] for r in range(3)]
    if not h[2] > 0.0:                       # h_2 <= 0 or NaN
        return None
    u, v = h[0] / h[2], h[1] / h[2]
    lim = float(COORD_MAX + 1)               # |trunc(a)| <= 8192  <=>  |a| < 8193; a NaN or an infinity fails
    if not (-lim < u < lim) or not (-lim < v < lim):
        return None
    return int(u), int(v)                    # truncation toward zero


def project(pose, P=DEFAULT_P, E=DEFAULT_E, dims=DEFAULT_DIMS):
    """Steps 1-4 for one box: (corners: 16 ints u0, v0 .. u7, v7 - zeros when skipped, drawn: 0 / 1) = cd_overlay_project."""
    M = matrix(P, E)
    out = []
    for c in corners(pose, dims):
        px = project_point(M, c)
        if px is None:
            return [0] * 16, 0
        out.extend(px)
    return out, 1


def segment_mask(width, height, a, b, thickness):
    """Step 6: the painted pixels of the segment a-b (integer end points) as a (height, width) bool array."""
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    t2 = np.int64(int(thickness) * int(thickness))
    xs = np.arange(width, dtype=np.int64)[None, :]
    ys = np.arange(height, dtype=np.int64)[:, None]
    dx, dy = np.int64(bx - ax), np.int64(by - ay)
    ex, ey = xs - ax, ys - ay
    fx, fy = xs - bx, ys - by
    L = dx * dx + dy * dy
    s = ex * dx + ey * dy
    cr = ex * dy - ey * dx
    near_a = (L == 0) | (s <= 0)
    near_b = ~near_a & (s >= L)
    return np.where(near_a, 4 * (ex * ex + ey * ey) <= t2,
                    np.where(near_b, 4 * (fx * fx + fy * fy) <= t2, 4 * (cr * cr) <= t2 * L))


def box_mask(width, height, box_corners, thickness=DEFAULT_THICKNESS):
    """Steps 5 and 6 of one drawn box (its 16 projected ints): union of its 12 edges' masks."""
    m = np.zeros((height, width), bool)
    c = [(box_corners[2 * k], box_corners[2 * k + 1]) for k in range(8)]
    for i, j in EDGES:
        m |= segment_mask(width, height, c[i], c[j], thickness)
    return m


def draw(images, poses, n_boxes=None, P=DEFAULT_P, E=DEFAULT_E, dims=DEFAULT_DIMS, thickness=DEFAULT_THICKNESS, rgb=DEFAULT_RGB):
    """Rule C11 on images (F, H, W, 3) uint8 with poses (F, B, 4, 4) (or (F, B, 16)) and n_boxes (F,) (None: all B).
    Returns (drawn images - a copy, boxes (F, B, 17) int32: 16 corners + drawn, painted (F, H, W) bool)."""
    img = np.array(images, dtype=np.uint8, copy=True)
    assert img.ndim == 4 and img.shape[3] == 3
    F, H, W = img.shape[:3]
    assert 1 <= W <= COORD_MAX and 1 <= H <= COORD_MAX and 1 <= int(thickness) <= MAX_THICKNESS
    poses = np.asarray(poses, np.float64).reshape(F, -1, 16)
    B = poses.shape[1]
    n_boxes = np.full(F, B, np.int32) if n_boxes is None else np.asarray(n_boxes, np.int32)
    boxes = np.zeros((F, B, 17), np.int32)
    painted = np.zeros((F, H, W), bool)
    for f in range(F):
        for b in range(int(n_boxes[f])):
            c, drawn = project(poses[f, b], P, E, dims)
            boxes[f, b, :16], boxes[f, b, 16] = c, drawn
            if drawn:
                painted[f] |= box_mask(W, H, c, thickness)
        img[f][painted[f]] = np.asarray(rgb, np.uint8)
    return img, boxes, painted


# the rotations that map a cuboid onto itself with its axes kept: the identity and the three 180-degree turns (an ICP pose is
# only defined up to these)
SYMMETRIES = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))


def corner_error_px(box_corners, truth_pose, P=DEFAULT_P, E=DEFAULT_E, dims=DEFAULT_DIMS):
    """How far a drawn box (its 16 projected ints) lies from where `truth_pose` puts it: the largest per-axis distance, over the
    eight corners, between the drawn pixel and the untruncated projection of the truth's corner, minimised over SYMMETRIES."""
    M = matrix(P, E)
    got = np.asarray(box_corners, np.float64).reshape(8, 2)
    best = np.inf
    for sgn in SYMMETRIES:
        T = np.array(truth_pose, np.float64).reshape(4, 4)
        T[:3, :3] = T[:3, :3] * np.asarray(sgn)[None, :]
        worst = 0.0
        for k, c in enumerate(corners(T, dims)):
            x, y, z = (float(v) for v in c)
            h = [((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] for r in range(3)]
            worst = max(worst, abs(got[k, 0] - h[0] / h[2]), abs(got[k, 1] - h[1] / h[2]))
        best = min(best, worst)
    return best
