"""The scenarios of the pose-information tests (rule C23), as plain CPU code: templates, views of one, two and three faces, the edge
values of the stand-alone call and the fused cases.  tests/test_pose_info_cpu.py asserts, from the specification alone
(perception_amd/pose_info.py), that each shows what it is for, and runs the host arithmetic on all of them;
tests/test_gpu_pose_info.py compares the library with the same specification bit for bit."""
import functools
import os

import numpy as np

import fused_reference as FR
import pair_score_scenarios as PSS
import pose_info_reference as PR
import test_gpu_fused_options as T
from conftest import GOLDEN
from perception_amd import capi, icp_plane as IP, pcd, synth, templates

f32 = np.float32
IDENT = np.eye(4, dtype=f32)
RANGE = capi.CD_POSE_INFO_RANGE_DEFAULT
SUPPORT = 16.0                    # the support the scenarios pass (never the library's default)
SETTING = (RANGE, SUPPORT)
SW, SH = T.SW, T.SH


@functools.lru_cache(maxsize=None)
def tpl3():
    """The launch file's cuboid, 0.2 x 0.1 x 0.03 at 2 mm: three faces, one per axis (lat_nearest_axes), 7250 points.  In index
    order: the face of constant z, then y, then x - a point on a shared edge belongs to the earlier face (rule C5's tie)."""
    return templates.template_xyz32(**templates.DEFAULT_TEMPLATE)


@functools.lru_cache(maxsize=None)
def tpl_small():
    """0.05 x 0.05 x 0.03 at 2 mm: three faces, 1375 points."""
    return templates.template_xyz32(0.05, 0.05, 0.03, 0.002)


@functools.lru_cache(maxsize=None)
def tpl6():
    """The six-face cuboid of the golden files (two faces per axis: lat_nearest's face loop), 21400 points."""
    return np.ascontiguousarray(pcd.read_xyz(os.path.join(GOLDEN, "template_cuboid_L200_W100_H75.pcd")).astype(f32))


@functools.lru_cache(maxsize=None)
def tpl6_small():
    """A six-face box of 0.06 x 0.04 x 0.02 at 2 mm, make_cuboid.py's three faces and their opposites: 2200 points, two faces per
    axis (lat_nearest's face loop)."""
    L, W, H, d = 0.06, 0.04, 0.02, 0.002
    X, Y, Z = (np.round(np.arange(-e / 2.0, e / 2.0, d), 6) for e in (L, W, H))
    grid = lambda a, b: tuple(v.ravel() for v in np.meshgrid(a, b))
    out = []
    for sgn in (-1.0, 1.0):
        fx, fy = grid(X, Y)
        out.append(np.stack([fx, fy, np.full(fx.shape, sgn * H / 2.0)], axis=1))
        gx, gz = grid(X, Z)
        out.append(np.stack([gx, np.full(gx.shape, sgn * W / 2.0), gz], axis=1))
        hy, hz = grid(Y, Z)
        out.append(np.stack([np.full(hy.shape, sgn * L / 2.0), hy, hz], axis=1))
    return np.ascontiguousarray(np.concatenate(out).astype(f32))


@functools.lru_cache(maxsize=None)
def faces_of(name):
    """The template's faces as index arrays, in index order, with each face's constant axis: [(w, indices)]."""
    tpl = {"tpl3": tpl3, "tpl6": tpl6, "small": tpl_small}[name]()
    w = IP.face_axes(tpl)
    cuts = [0] + [int(i) + 1 for i in np.nonzero(np.diff(w))[0]] + [len(tpl)]
    # (two consecutive faces of one axis would not show in diff: none of these templates has them)
    return [(int(w[a]), np.arange(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]


def interior(tpl, idx):
    """The points of a face that lie on no edge of the template's bounding box along the face's own axes: no tie with another face."""
    lo, hi = tpl.min(axis=0), tpl.max(axis=0)
    p = tpl[idx]
    on_box = (p == lo[None, :]) | (p == hi[None, :])
    return idx[on_box.sum(axis=1) <= 1]


def motion(angle_deg=2.0, shift=(0.001, -0.0005, 0.0008)):
    return PSS.motion(angle_deg, shift)


def moved_view(tpl, idx, n, seed, noise=0.001, T=None):
    """(src, T): n of the template points idx with noise, taken to the scene by the inverse of T (float64), so that T brings
    them back onto the template up to rounding."""
    rng = np.random.default_rng(seed)
    T = motion() if T is None else T
    p = tpl[rng.choice(idx, min(n, len(idx)), replace=False)].astype(np.float64) + rng.normal(scale=noise, size=(min(n, len(idx)), 3))
    Ti = np.linalg.inv(T.astype(np.float64))
    return np.ascontiguousarray((p @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32)), T


# ---- known answers: exact lattice points, T = identity -------------------------------------------------------------------------------
def exact_one_face():
    """Every point of the template's first face: nothing ties with an earlier face."""
    return tpl3()[faces_of("tpl3")[0][1]], IDENT, tpl3()


def exact_two_faces():
    """The first two faces (constant z, constant y): their common edge runs along x."""
    f = faces_of("tpl3")
    return tpl3()[np.concatenate([f[0][1], f[1][1]])], IDENT, tpl3()


def exact_three_faces():
    return tpl3().copy(), IDENT, tpl3()


def exact_two_faces_plus(k):
    """The two faces plus k interior points of the third, spread over it."""
    src, _, tpl = exact_two_faces()
    third = interior(tpl, faces_of("tpl3")[2][1])
    pick = third[np.linspace(0, len(third) - 1, k).astype(int)]
    return np.concatenate([src, tpl[pick]]), IDENT, tpl


PLUS = (1, 3, 10, 50)


# ---- the cases every implementation runs: (name, src, T, tpl, max_range, min_support, accepted) --------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for name, (src, T_, tpl) in (("one_face", exact_one_face()), ("two_faces", exact_two_faces()), ("three_faces", exact_three_faces())):
        out.append((name, src, T_, tpl, RANGE, 1.0, 1))
    for k in PLUS:
        src, T_, tpl = exact_two_faces_plus(k)
        out.append(("two_plus_%d" % k, src, T_, tpl, RANGE, 1.0, 1))
    f3, f6 = faces_of("tpl3"), faces_of("tpl6")
    for name, idx, n, seed in (("view_one", f3[0][1], 1400, 1), ("view_two", np.concatenate([f3[0][1], f3[2][1]]), 1400, 2),
                               ("view_three", np.arange(len(tpl3())), 1400, 3), ("view_three_few", np.arange(len(tpl3())), 65, 4)):
        src, T_ = moved_view(tpl3(), idx, n, seed)
        out.append((name, src, T_, tpl3(), RANGE, SUPPORT, 1))
    src, T_ = moved_view(tpl6(), np.concatenate([f6[0][1], f6[1][1], f6[5][1]]), 900, 5)
    out.append(("six_faces", src, T_, tpl6(), RANGE, SUPPORT, 1))
    src, T_ = moved_view(tpl3(), np.arange(len(tpl3())), 300, 6, noise=0.004)            # a range that many points miss
    out.append(("not_accepted", src, T_, tpl3(), 0.004, SUPPORT, 0))
    out += [("tau", ) + tau_case() + (SUPPORT, 1), ("edge_ties", ) + tie_case() + (1.0, 1), ("far", ) + far_case() + (1.0, 1)]
    return out


def tau_case():
    """(src, T, tpl, d): four points straight off the small template's first face at one height - their float32 d2 is one value v,
    and d is chosen so that tau(d) = v exactly: inside - and two points one float further out (outside)."""
    from perception_amd import pair_score as PS
    tpl = tpl_small()
    w, idx = faces_of("small")[0]
    src = tpl[interior(tpl, idx)[[0, 7, 50, 99, 130, 160]]].copy()
    c = src[0, w]
    away = f32(1.0) if c == tpl[:, w].max() else f32(-1.0)
    z1 = f32(c + away * f32(0.0625))
    src[:4, w] = z1
    src[4:, w] = np.nextafter(z1, f32(away) * f32(np.inf))
    v = f32(f32(z1 - c) * f32(z1 - c))
    d = float(np.nextafter(np.sqrt(np.float64(v)), np.inf))
    assert PS.tau_of(d) == v
    return src, IDENT, tpl, d


def tie_case():
    """(src, T, tpl, d): points exactly on the edges that two faces share, and slightly off them: the neighbour is the lower index."""
    tpl = tpl3()
    lo, hi = tpl.min(axis=0), tpl.max(axis=0)
    edge = tpl[((tpl == lo[None, :]) | (tpl == hi[None, :])).sum(axis=1) >= 2]
    src = np.concatenate([edge, edge + f32(2.0 ** -12), tpl[::9]])
    return np.ascontiguousarray(src.astype(f32)), IDENT, tpl, 0.002


def far_case():
    """(src, T, tpl, d): a range of 300 m and points 200 m off the first face - r r = 40000 is outside LatFix's range (2^14) and
    goes through the general conversion - among points on the template."""
    tpl = tpl_small()
    w, idx = faces_of("small")[0]
    src = tpl[::5].copy()
    far = tpl[interior(tpl, idx)[:40:4]].copy()
    far[:, w] += f32(200.0) if far[0, w] == tpl[:, w].max() else f32(-200.0)
    return np.ascontiguousarray(np.concatenate([src, far])), IDENT, tpl, 300.0


# ---- the stand-alone call's sizes -----------------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 3001)      # one wave's pass, the workgroup's four, and a cluster of a few thousand


@functools.lru_cache(maxsize=None)
def size_case(n):
    """(src, T): n noisy points of the whole three-face template under a small motion."""
    return moved_view(tpl3(), np.arange(len(tpl3())), n, 100 + n) if n else (np.zeros((0, 3), f32), motion())


# ---- the fused call -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused_batch():
    """Four frames of 128 x 96: two boxes, the grid scene (twelve small clusters: more than a frame record holds), one box, and a
    table with no object on it (no cluster)."""
    return np.ascontiguousarray(np.concatenate([PSS.fused_batch(), synth.frame(4, k_obj=0, width=SW, height=SH)[None]], 0))


class PoseCase(T.Case):
    """A fused call with rule C23 on at SETTING, and rule C21 at `pair` (None: off)."""

    def __init__(self, id, frames, prm, tpls, opt, pair=None, **kw):
        T.Case.__init__(self, id, frames, prm, tpls, opt, **kw)
        self.pair = pair

    @functools.lru_cache(maxsize=None)
    def expected(self):
        return PR.expected(self.frames, self.prm, self.tpls, self.opt, SETTING, self.pair)


FUSED_KINDS = ("alone", "bound", "cluster_guess_pair")


@functools.lru_cache(maxsize=None)
def fused_case(kind):
    """alone: the mode with nothing else, template_slot = -1 over the two slots.  bound: rule C8 (with rule C17, which the reference
    needs for it).  cluster_guess_pair: rule C13's guess, with rule C21 on as well."""
    prm = capi.default_params()
    prm.cluster_min_size = 30
    prm.icp_max_iterations = 12
    prm.template_slot = -1
    opt, pair = FR.options(), None
    if kind == "bound":
        opt = FR.options(plane=(capi.CD_ICP_PLANE_WEIGHT_DEFAULT, capi.CD_ICP_PLANE_SWITCH_DEFAULT), bound=PSS.BOUND)
    elif kind == "cluster_guess_pair":
        prm.icp_use_guess = capi.CD_GUESS_CLUSTER
        opt, pair = FR.options(guess="cluster"), PSS.SETTING
    else:
        assert kind == "alone"
    return PoseCase("pose-" + kind, fused_batch(), prm, PSS.fused_templates(), opt, pair=pair)


@functools.lru_cache(maxsize=None)
def tiny_case():
    """Clusters of one and two points next to a real one (the cloud of the fused-option tests)."""
    base = T.tiny_case(0)
    return PoseCase("pose-tiny", base.frames, base.prm, base.tpls, base.opt)


# ---- more results than workgroups, the slots alternating in the queue ----------------------------------------------------------------
RESTAGE_WORKGROUPS = ("1", "2")   # CUBOID_ICP_MAX_WG: the cap on the kernel's grid


@functools.lru_cache(maxsize=None)
def restage_case():
    """Two grid scenes (24 small clusters) against a three-face and a six-face small box, template_slot = -1: by size - the order
    of the kernel's queue - the kept slots alternate, so a workgroup that takes many results restages its tables again and again
    and goes from lat_nearest_axes to lat_nearest and back."""
    prm = capi.default_params()
    prm.cluster_min_size = 30
    prm.icp_max_iterations = 12
    prm.template_slot = -1
    frames = np.ascontiguousarray(np.stack([synth.render(synth.scene_grid(i), width=SW, height=SH) for i in (3, 5)]))
    return PoseCase("pose-restage", frames, prm, {0: tpl_small(), 1: tpl6_small()}, FR.options())


def queue_slots(case):
    """The slots of the case's results in the order of the kernel's queue: largest first, equal sizes in cluster order."""
    cl = [c for e in case.expected() for c in e["clusters"]]
    return [c.slot for c in sorted(cl, key=lambda c: -c.size)]
