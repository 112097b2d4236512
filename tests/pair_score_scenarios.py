"""The scenarios of tests/test_gpu_pair_score.py (rule C21 on the GPU), as plain CPU code: sources, settings and fused cases.
tests/test_pair_score_reference_cpu.py imports them and asserts, from the reference alone (tests/pair_score_reference.py), that each
shows what it is for; the GPU tests then compare the library with the same reference bit for bit."""
import functools
import os

import numpy as np

import fused_reference as FR
import pair_score_reference as PR
import reject_scenarios as RS
import test_gpu_fused_options as T
from conftest import GOLDEN
from perception_amd import capi, pcd, synth, templates

f32 = np.float32
SETTING = (capi.CD_PAIR_SCORE_RANGE_DEFAULT, capi.CD_PAIR_SCORE_MIN_COVERAGE_DEFAULT, capi.CD_PAIR_SCORE_MIN_INLIER_DEFAULT)
SW, SH = T.SW, T.SH                # 128 x 96, the sensor size of the fused-option and rejection tests
PS_THREADS, PS_CHUNK, PS_TILE = 256, 1024, 1024     # kernels.hpp: lanes of a workgroup, queries of an item (four per lane), targets of an LDS tile


# ---- (a) the false accept on scanned templates ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scanned(name):
    return np.ascontiguousarray(pcd.read_xyz(os.path.join(GOLDEN, name + "_ascii.pcd")).astype(f32))


@functools.lru_cache(maxsize=None)
def marker_source(kind):
    """A source taken from the marker scan - "half": every second point; "view": its lower 60 % along its longest axis - turned by
    6 degrees about its centroid, moved by 5 mm, with 0.5 mm of noise (seeded)."""
    p = scanned("marker")
    if kind == "half":
        return RS.moved(p[::2], 6, angle_deg=6.0, shift=0.005)
    ax = int(np.argmax(p.max(axis=0) - p.min(axis=0)))
    return RS.moved(p[p[:, ax] <= np.quantile(p[:, ax], 0.6)], 7, angle_deg=6.0, shift=0.005)


@functools.lru_cache(maxsize=None)
def scanned_pair(kind, template_name):
    """(the oracle's ICP result from the identity, the score at SETTING) of marker_source(kind) against a scanned template."""
    return PR.registered_pair(scanned(template_name), marker_source(kind), capi.default_params(), SETTING)


# ---- the stand-alone call: shapes and edge values -----------------------------------------------------------------------------------
SMALL = (1, 3, 63, 64, 65)
SHAPES = tuple((n, m) for n in SMALL for m in SMALL) + (
    # (n, m): one LDS tile of targets - 1, exact, + 1, two tiles + 1: the template forward, the source backward
    (300, PS_TILE - 1), (300, PS_TILE), (300, PS_TILE + 1), (300, 2 * PS_TILE + 1), (PS_TILE - 1, 300), (PS_TILE, 300), (PS_TILE + 1, 300), (2 * PS_TILE + 1, 300),
    # one query per lane - 1, exact, + 1, in each direction (PS_TILE + 1 above: one query over a whole item - the smallest pair that is
    # split over two workgroups by its source, (300, PS_TILE + 1) by its template)
    (PS_THREADS - 1, 40), (PS_THREADS, 40), (PS_THREADS + 1, 40), (40, PS_THREADS - 1), (40, PS_THREADS), (40, PS_THREADS + 1),
    # both directions split, and three items with an uneven last row
    (PS_CHUNK + 1, PS_CHUNK + 1), (2 * PS_CHUNK + 1, PS_CHUNK + 77),
    # a last tile that the +inf padding fills up by 6 and by 2 points (the tile is padded to a multiple of 8), in each direction
    (10, 14), (14, 10))


def motion(angle_deg=3.0, shift=(0.002, -0.001, 0.0015)):
    a = np.deg2rad(angle_deg)
    M = np.eye(4)
    M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    M[:3, 3] = shift
    return M.astype(f32)


@functools.lru_cache(maxsize=None)
def shape_case(n, m):
    """(src, T, tpl, max_range): template points in a 0.2 m box, the source near a sample of them, a 6 mm range that some points
    of either side miss."""
    rng = np.random.default_rng(1000 * n + m)
    tpl = rng.uniform(-0.1, 0.1, (m, 3)).astype(f32)
    src = (tpl[rng.choice(m, n, replace=n > m)] + rng.normal(scale=0.004, size=(n, 3))).astype(f32)
    return src, motion(), tpl, 0.006


def tie_case():
    """Duplicate points on both sides: every minimum is reached several times."""
    rng = np.random.default_rng(77)
    tpl = np.repeat(rng.uniform(-0.1, 0.1, (150, 3)).astype(f32), 3, axis=0)
    src = np.repeat(tpl[::5] + f32(2.0 ** -9), 2, axis=0)
    return np.ascontiguousarray(src), np.eye(4, dtype=f32), np.ascontiguousarray(tpl), 0.006


def tau_case():
    """f = 0, 1/16, 1/4 and r = 0, 1/16 at the range 1/4: the distances equal to tau = 1/16 are inside."""
    return np.array([[0, 0, 0], [1, 0, 0], [0, 0.5, 0]], f32), np.eye(4, dtype=f32), np.array([[0, 0, 0], [1, 0, 0.25]], f32), 0.25


# ---- the fused call -----------------------------------------------------------------------------------------------------------------
COARSE = (2, 24)                  # rule C18's (stride, min_points) of its combination
BOUND = 0.55                      # rule C8's distance of its combination (no guess: the clusters lie 0.5 .. 0.6 m from the template)


@functools.lru_cache(maxsize=None)
def fused_templates():
    """slot 0: the launch file's default cuboid (0.2 x 0.1 x 0.03, the boxes of the synthetic frames); slot 1: the small box of the
    grid scene"""
    return {0: templates.template_xyz32(**templates.DEFAULT_TEMPLATE), 1: templates.template_xyz32(0.05, 0.05, 0.03, 0.002)}


@functools.lru_cache(maxsize=None)
def fused_batch():
    """Three frames of 128 x 96: two boxes, the grid scene (twelve small clusters: more than a frame record holds), one box."""
    return np.ascontiguousarray(np.stack([synth.frame(1, width=SW, height=SH), synth.render(synth.scene_grid(3), width=SW, height=SH),
                                          synth.frame(0, width=SW, height=SH)], 0))


@functools.lru_cache(maxsize=None)
def fused_depth():
    pairs = [FR.depth_of_records(fr, SH, SW) for fr in fused_batch()]
    return np.ascontiguousarray(np.stack([p[0] for p in pairs])), np.ascontiguousarray(np.stack([p[1] for p in pairs]))


def camera():
    cam = capi.default_depth_camera()
    cam.width, cam.height = SW, SH
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params(SW, SH)
    cam.depth_scale = synth.DEPTH_SCALE
    cam.color = capi.CD_COLOR_RGB8
    return cam


class PairCase(T.Case):
    """A fused call with rule C21 on at SETTING, and rule C18 at `coarse` (None: off)."""

    def __init__(self, id, frames, prm, tpls, opt, coarse=None, empty_slot=False, **kw):
        T.Case.__init__(self, id, frames, prm, tpls, opt, **kw)
        self.coarse, self.empty_slot = coarse, empty_slot

    @functools.lru_cache(maxsize=None)
    def expected(self):
        if self.empty_slot:
            return PR.expected_empty_slot(self.frames, self.prm, self.tpls, self.opt, SETTING)
        return PR.expected(self.depth if self.depth is not None else self.frames, self.prm, self.tpls, self.opt, SETTING, self.coarse)


FUSED_KINDS = ("alone", "bound", "cluster_guess", "coarse", "depth")


@functools.lru_cache(maxsize=None)
def fused_case(kind):
    """alone: the mode with nothing else, template_slot = -1 over the two slots.  bound: rule C8 (with rule C17, which the reference
    needs for it).  cluster_guess: rule C13.  coarse: rule C18.  depth: a depth + colour call."""
    prm = capi.default_params()
    prm.cluster_min_size = 30
    prm.icp_max_iterations = 12
    prm.template_slot = -1
    opt, coarse, depth, rgb = FR.options(), None, None, -1
    if kind == "bound":
        opt = FR.options(plane=(capi.CD_ICP_PLANE_WEIGHT_DEFAULT, capi.CD_ICP_PLANE_SWITCH_DEFAULT), bound=BOUND)
    elif kind == "cluster_guess":
        prm.icp_use_guess = capi.CD_GUESS_CLUSTER
        opt = FR.options(guess="cluster")
    elif kind == "coarse":
        coarse = COARSE
    elif kind == "depth":
        opt, depth, rgb = FR.options(cam=camera()), fused_depth(), 12
        prm.rgb_offset = 12
    else:
        assert kind == "alone"
    return PairCase("pair-" + kind, fused_batch(), prm, fused_templates(), opt, coarse=coarse, depth=depth, rgb=rgb)


@functools.lru_cache(maxsize=None)
def tiny_case():
    """(c) clusters of one and two points next to a real one (the cloud of the fused-option tests)."""
    base = T.tiny_case(0)
    return PairCase("pair-tiny", base.frames, base.prm, base.tpls, base.opt)


@functools.lru_cache(maxsize=None)
def empty_slot_case():
    """(c) template_slot = 2 with slots 0 and 1 loaded: nothing to register against."""
    prm = capi.default_params()
    prm.cluster_min_size = 30
    prm.icp_max_iterations = 12
    prm.template_slot = 2
    return PairCase("pair-empty-slot", fused_batch()[:1], prm, fused_templates(), FR.options(), empty_slot=True)
