"""Canonical rule C14 restated in plain Python / numpy: the cuboid of an ICP pose rendered into the depth image the
pose was found in, and every covered pixel compared with what the sensor measured there.

This is the CPU statement of what perception_amd/csrc/k_verify.hip computes on the device and cd_verify_pixel /
cd_verify_box_host on the host; the tests require all of them to equal it in every field.  verify_box walks WHOLE images (the
device walks a rectangle it can prove sufficient: that proof is tested against this).  The selections are np.where over the
rule's own comparisons, never np.minimum / np.maximum, so that a NaN takes the same turn here as in the C code.  Nothing here is
on a hot path.
"""
import numpy as np

MISS, AGREE, THROUGH, OCCLUDED, INVALID = 0, 1, 2, 3, 4
DEFAULT_DIMS = (0.2, 0.1, 0.03)
DEFAULT_TOLERANCE = 0.01
DEFAULT_MIN_SCORE = 0.9
DEFAULT_MIN_AGREE = 200
RECORD = np.dtype([("verified", "<i4"), ("passed", "<i4"), ("n_hit", "<i4"), ("n_agree", "<i4"), ("n_through", "<i4"),
                   ("n_occluded", "<i4"), ("n_invalid", "<i4"), ("reserved", "<i4"), ("agree_abs_um", "<i8"), ("score", "<f8")])
COUNTS = ("n_hit", "n_agree", "n_through", "n_occluded", "n_invalid", "agree_abs_um")
_UM_LIMIT = 9223372036854775808.0     # a term of 2^63 or more counts as 2^63 - 1


def camera(cam):
    """(fx, fy, cx, cy, depth_scale) of a cd_depth_camera-like object: its float32 values widened to Python floats."""
    return tuple(float(np.float32(getattr(cam, k))) for k in ("fx", "fy", "cx", "cy", "depth_scale"))


def _pose(pose):
    return [float(v) for v in np.asarray(pose, np.float64).reshape(16)]


def verified(pose, dims=DEFAULT_DIMS):
    """Step 1: False when an entry of R, t is non-finite or a corner is not in front of the camera."""
    H = _pose(pose)
    if not all(np.isfinite(H[4 * r + c]) for r in range(3) for c in range(4)):
        return False
    half = [float(d) / 2.0 for d in dims]
    with np.errstate(all="ignore"):
        for k in range(8):
            x = np.float64(half[0] if k & 4 else -half[0])
            y = np.float64(half[1] if k & 2 else -half[1])
            z = np.float64(half[2] if k & 1 else -half[2])
            zc = ((np.float64(H[8]) * x + np.float64(H[9]) * y) + np.float64(H[10]) * z) + np.float64(H[11])
            if not zc > 0.0:
                return False
    return True


def _render(cam, pose, dims, u, v):
    """Steps 2 and 3 for the pixels (u, v) (float64 arrays of one shape): (hit bool array, z_r)."""
    fx, fy, cx, cy, _ = camera(cam)
    H = np.asarray(_pose(pose), np.float64)
    with np.errstate(all="ignore"):
        dx = (u - cx) / fx
        dy = (v - cy) / fy
        tn = np.full(u.shape, -np.inf)
        tf = np.full(u.shape, np.inf)
        miss = np.zeros(u.shape, bool)
        for a in range(3):
            c0, c1, c2 = H[a], H[4 + a], H[8 + a]
            half = np.float64(float(dims[a])) / np.float64(2.0)
            o = -((c0 * H[3] + c1 * H[7]) + c2 * H[11])
            dd = (c0 * dx + c1 * dy) + c2
            par = dd == 0.0
            t1 = (-half - o) / dd
            t2 = (half - o) / dd
            lo = np.where(t1 < t2, t1, t2)
            hi = np.where(t1 < t2, t2, t1)
            miss = miss | (par & bool(np.abs(o) > half))
            tn = np.where(par, tn, np.where(lo > tn, lo, tn))
            tf = np.where(par, tf, np.where(hi < tf, hi, tf))
        hit = ~miss & (tn <= tf) & (tn > 0.0)
    return hit, tn


def _classes(cam, hit, z_r, d, tau):
    """Step 4: (class array, per-pixel term of agree_abs_um as int64)."""
    scale = camera(cam)[4]
    tau = float(tau)
    with np.errstate(all="ignore"):
        z_m = d.astype(np.float64) * scale
        cls = np.where(d == 0, INVALID, np.where(z_m - z_r > tau, THROUGH, np.where(z_r - z_m > tau, OCCLUDED, AGREE)))
        cls = np.where(hit, cls, MISS)
        e = np.abs(z_m - z_r) * 1e6 + 0.5
        agree = cls == AGREE
        um = np.where(agree & (e < _UM_LIMIT), e, 0.0).astype(np.int64)
        um = np.where(agree & ~(e < _UM_LIMIT), np.int64(np.iinfo(np.int64).max), um)
    return cls, um


def depth_cloud(depth, cam):
    """Canonical rule C7 without colour: the (H * W, 4) float32 records x y z rgb (NaN where the depth is 0, rgb word 0) that the
    fused depth calls deproject an (H, W) uint16 image to - what a CPU chain is fed to get the poses this image verifies."""
    f32 = np.float32
    depth = np.asarray(depth)
    h, w = depth.shape
    v, u = np.divmod(np.arange(h * w, dtype=np.int64), w)
    d = depth.reshape(-1)
    out = np.zeros((h * w, 4), f32)
    z = d.astype(f32) * f32(cam.depth_scale)
    out[:, 0] = ((u.astype(f32) - f32(cam.cx)) / f32(cam.fx)) * z
    out[:, 1] = ((v.astype(f32) - f32(cam.cy)) / f32(cam.fy)) * z
    out[:, 2] = z
    out[d == 0, :3] = np.nan
    return out


def classify(cam, pose, dims, tau, u, v, d):
    """Steps 2-4 for one pixel: (class, z_r) - z_r is 0.0 for a miss.  Step 1 is not applied."""
    uu, vv = np.array([float(int(u))]), np.array([float(int(v))])
    hit, z_r = _render(cam, pose, dims, uu, vv)
    cls, _ = _classes(cam, hit, z_r, np.array([int(d)], np.uint16), tau)
    return int(cls[0]), (float(z_r[0]) if hit[0] else 0.0)


def verify_box(depth, cam, pose, dims=DEFAULT_DIMS, tau=DEFAULT_TOLERANCE):
    """The counts of rule C14 for one box over one whole (H, W) uint16 image: a dict of verified, n_hit, n_agree, n_through,
    n_occluded, n_invalid, agree_abs_um."""
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16 and depth.ndim == 2
    out = dict(verified=0, n_hit=0, n_agree=0, n_through=0, n_occluded=0, n_invalid=0, agree_abs_um=0)
    if not verified(pose, dims):
        return out
    h, w = depth.shape
    v, u = np.divmod(np.arange(h * w, dtype=np.int64), w)
    hit, z_r = _render(cam, pose, dims, u.astype(np.float64), v.astype(np.float64))
    cls, um = _classes(cam, hit, z_r, depth.reshape(-1), tau)
    out.update(verified=1, n_hit=int(hit.sum()), n_agree=int((cls == AGREE).sum()), n_through=int((cls == THROUGH).sum()),
               n_occluded=int((cls == OCCLUDED).sum()), n_invalid=int((cls == INVALID).sum()))
    with np.errstate(over="ignore"):
        out["agree_abs_um"] = int(np.sum(um, dtype=np.int64))
    return out


def score(n_agree, n_through):
    """Step 5: n_agree / (n_agree + n_through), 0.0 when there is neither."""
    den = int(n_agree) + int(n_through)
    return float(np.float64(int(n_agree)) / np.float64(den)) if den else 0.0


def passed(rec, min_agree=DEFAULT_MIN_AGREE, min_score=DEFAULT_MIN_SCORE):
    """Step 5 for a dict of counts (or a RECORD row)."""
    return int(bool(rec["verified"]) and int(rec["n_agree"]) >= int(min_agree) and score(rec["n_agree"], rec["n_through"]) >= float(min_score))


def record(counts, min_agree=DEFAULT_MIN_AGREE, min_score=DEFAULT_MIN_SCORE):
    """One RECORD (= cd_verify_box) from the counts of verify_box."""
    r = np.zeros((), RECORD)
    r["verified"] = counts["verified"]
    for k in COUNTS:
        r[k] = counts[k]
    r["score"] = score(counts["n_agree"], counts["n_through"])
    r["passed"] = passed(counts, min_agree, min_score)
    return r


def verify(depth_batch, poses, n_boxes, cam, dims=DEFAULT_DIMS, tau=DEFAULT_TOLERANCE, min_agree=DEFAULT_MIN_AGREE,
           min_score=DEFAULT_MIN_SCORE, box_dims=None):
    """Rule C14 on images (F, H, W) uint16 with poses (F, B, 4, 4) (or (F, B, 16)) and n_boxes (F,) (None: all B): an (F, B) array
    of RECORD, all zero in the slots at and beyond n_boxes[f].  box_dims: None or (F, B, 3), the dims of each slot."""
    depth_batch = np.asarray(depth_batch)
    F = depth_batch.shape[0]
    poses = np.asarray(poses, np.float64).reshape(F, -1, 16)
    B = poses.shape[1]
    n_boxes = np.full(F, B, np.int32) if n_boxes is None else np.asarray(n_boxes, np.int32)
    bd = None if box_dims is None else np.asarray(box_dims, np.float64).reshape(F, B, 3)
    out = np.zeros((F, B), RECORD)
    for f in range(F):
        for b in range(int(n_boxes[f])):
            d = dims if bd is None else tuple(float(x) for x in bd[f, b])
            out[f, b] = record(verify_box(depth_batch[f], cam, poses[f, b], d, tau), min_agree, min_score)
    return out
