"""The scenarios of tests/test_gpu_icp_reject.py (rule C19 on the GPU), as plain CPU code: sources, settings and fused cases.
tests/test_icp_reject_cpu.py imports them and asserts, from the reference alone (tests/reject_reference.py), that each shows what
it is for; the GPU tests then compare the library with the same reference bit for bit."""
import functools
import os

import numpy as np

import fused_reference as FR
import reject_reference as RR
import test_gpu_fused_options as T
from conftest import GOLDEN
from perception_amd import capi, icp_plane as IP, pcd, synth, templates

f32 = np.float32
FACTOR = 4.0                      # the issue's factor for the contamination scene
TEMPLATE_FILES = {"lattice": "template_cuboid_L200_W100_H75_3faces.pcd", "scanned": "eraser_ascii.pcd"}
KINDS = tuple(TEMPLATE_FILES)
ICP_QSLICE, RJ_THREADS = 512, 256  # common.hpp, k_icp_reject.hip
# cd_icp sizes: the least legal ones, around a wave, around the select kernel's workgroup, around a slice, three slices, and
# a cluster of nine slices that gives every thread of the select kernel seventeen points (more points than either template has)
SIZES = (3, 4, 5, 63, 64, 65, RJ_THREADS - 1, RJ_THREADS, RJ_THREADS + 1, ICP_QSLICE - 1, ICP_QSLICE, ICP_QSLICE + 1, 2 * ICP_QSLICE + 1, 4099)
SCENE_SEEDS = (2, 3, 4, 5, 6, 7)   # the contamination scene; the GPU runs the first two of each template
GPU_SCENE_SEEDS = SCENE_SEEDS[:2]


@functools.lru_cache(maxsize=None)
def template(kind):
    return np.ascontiguousarray(pcd.read_xyz(os.path.join(GOLDEN, TEMPLATE_FILES[kind])).astype(f32))


def icp_params(max_iterations=None):
    prm = capi.default_params()
    if max_iterations is not None:
        prm.icp_max_iterations = max_iterations
    return prm


def moved(points, seed, angle_deg=2.0, shift=0.004, noise=0.0005):
    """The points after a small rigid motion about their centroid, with noise (float64 in, float32 out)."""
    rng = np.random.default_rng(seed)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(angle_deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    s = rng.normal(size=3)
    s *= shift / np.linalg.norm(s)
    c = p.mean(axis=0)
    return ((p - c) @ R.T + c + s + rng.normal(scale=noise, size=p.shape)).astype(f32)


def sized_source(kind, n, seed):
    """n points: template points after a small motion, the last n // 6 of them replaced by points of a ball beside the object."""
    tpl = template(kind)
    rng = np.random.default_rng(1000 + seed)
    src = moved(tpl[rng.choice(len(tpl), n, replace=n > len(tpl))], seed)
    nb = n // 6
    if nb:
        d = rng.normal(size=(nb, 3))
        d *= (0.012 * rng.uniform(size=nb) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
        hi = src.max(axis=0).astype(np.float64)
        src[n - nb:] = (np.array([hi[0] + 0.016, hi[1] - 0.02, hi[2] - 0.02]) + d).astype(f32)
    return np.ascontiguousarray(src)


# ---- ties and edge values ------------------------------------------------------------------------------------------------------------
def exact_subset(kind, n=300, seed=11):
    """Template points themselves: every d2 is 0, the median and the threshold are 0, everything is kept."""
    tpl = template(kind)
    return np.ascontiguousarray(tpl[np.sort(np.random.default_rng(seed).choice(len(tpl), n, replace=False))])


def _interior_face_points(n, seed, margin=0.012):
    """n points of one face of the lattice template, further than `margin` from the template's other faces; (points, the face's
    constant axis)"""
    tpl = template("lattice")
    axes = IP.face_axes(tpl)
    w = int(axes[0])
    face = tpl[axes == w]
    others = [a for a in range(3) if a != w]
    lo, hi = tpl.min(axis=0), tpl.max(axis=0)
    inside = np.all([(face[:, a] > lo[a] + margin) & (face[:, a] < hi[a] - margin) for a in others], axis=0)
    pts = face[inside]
    return pts[np.sort(np.random.default_rng(seed).choice(len(pts), n, replace=False))], w


def shifted_face(n=200, seed=12, delta=2.0 ** -8):
    """Points of one lattice face moved along its normal by a power of two, away from the box: every d2 has the same bits."""
    pts, w = _interior_face_points(n, seed)
    tpl = template("lattice")
    out = pts.copy()
    sign = 1.0 if pts[0, w] >= 0.5 * (tpl[:, w].min() + tpl[:, w].max()) else -1.0
    out[:, w] += f32(sign * delta)
    return np.ascontiguousarray(out)


def half_at_the_median(n=240, seed=13, delta=2.0 ** -8):
    """A sixth of the points on the template (d2 = 0), two thirds moved along the face normal by delta (one d2 value, the median's,
    across the median rank) and a sixth by 3 delta (beyond the threshold at factor 4: 9 > 4)."""
    pts, w = _interior_face_points(n, seed)
    tpl = template("lattice")
    sign = 1.0 if pts[0, w] >= 0.5 * (tpl[:, w].min() + tpl[:, w].max()) else -1.0
    out = pts.copy()
    k = n // 6
    out[k:n - k, w] += f32(sign * delta)
    out[n - k:, w] += f32(sign * 3 * delta)
    return np.ascontiguousarray(out)


# ---- small factors: stops -----------------------------------------------------------------------------------------------------------
SMALL_FACTOR = 0.25


def stops_at_once(kind):
    """Six points: two template points and four about 5 mm off the template.  m is one of the four's d2, a quarter of it keeps
    the two exact ones only: fewer than three at the first iteration."""
    tpl = template(kind)
    rng = np.random.default_rng(21)
    p = tpl[np.sort(rng.choice(len(tpl), 6, replace=False))].astype(np.float64)
    d = rng.normal(size=(4, 3))
    p[2:] += 0.005 * d / np.linalg.norm(d, axis=1)[:, None]
    return np.ascontiguousarray(p.astype(f32))


LATER_STOP = {"lattice": (28, 11), "scanned": (30, 31)}   # (points, seed) of stops_later, found by a search on the CPU reference


def stops_later_candidate(kind, n, seed):
    return sized_source(kind, n, 500 + seed)


def stops_later(kind):
    """A source that keeps three or more correspondences at factor 0.25 for at least one iteration and then fewer."""
    return stops_later_candidate(kind, *LATER_STOP[kind])


# ---- rule C8 together with rule C19 -------------------------------------------------------------------------------------------------
BOUND = 0.02


def near_and_far(kind, n_near=200, n_far=60, seed=31):
    """P: template points after a small motion (all within BOUND of the template); Q: points 4 to 6 cm outside the object's box (all
    beyond it).  Returns (source, the mask of P)."""
    tpl = template(kind)
    rng = np.random.default_rng(seed)
    P = moved(tpl[rng.choice(len(tpl), n_near, replace=False)], seed, angle_deg=1.0, shift=0.002)
    hi = tpl.max(axis=0).astype(np.float64)
    lo = tpl.min(axis=0).astype(np.float64)
    Q = np.c_[hi[0] + rng.uniform(0.04, 0.06, n_far), rng.uniform(lo[1], hi[1], n_far), rng.uniform(lo[2], hi[2], n_far)].astype(f32)
    src = np.ascontiguousarray(np.vstack([P, Q]))
    order = rng.permutation(len(src))
    mask = np.r_[np.ones(n_near, bool), np.zeros(n_far, bool)]
    return np.ascontiguousarray(src[order]), mask[order]


# ---- combinations ----------------------------------------------------------------------------------------------------------------
COARSE = (4, 512)                 # rule C18's (stride, min_points) of the combination


def coarse_source(kind):
    """700 points: eligible under COARSE, a coarse set of 175."""
    return sized_source(kind, 700, 77)


def far_source(kind, n=400, seed=41):
    """A cluster where the scene has it: the sized source turned by 50 degrees about z and put 0.4 m away - the identity is no
    start for it, the per-cluster guess (rule C13) is."""
    src = sized_source(kind, n, seed).astype(np.float64)
    a = np.deg2rad(50.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return np.ascontiguousarray((src @ R.T + np.array([0.1, -0.05, 0.4])).astype(f32))


# ---- the fused call -----------------------------------------------------------------------------------------------------------------
SW, SH = T.SW, T.SH


@functools.lru_cache(maxsize=None)
def fused_templates():
    """slot 0: a lattice (the small box of the fused-option tests); slot 1: a scanned cloud (the eraser)"""
    return {0: templates.template_xyz32(0.05, 0.05, 0.03, 0.002), 1: template("scanned")}


@functools.lru_cache(maxsize=None)
def fused_batch():
    """Three frames of 128 x 96: the grid scene (twelve small clusters), two boxes, one box."""
    return np.ascontiguousarray(np.stack([synth.render(synth.scene_grid(3), width=SW, height=SH), synth.frame(1, width=SW, height=SH),
                                          synth.frame(0, width=SW, height=SH)], 0))


class RejectCase(T.Case):
    """A fused call with rule C19 on at `factor` (0: off)."""

    def __init__(self, id, frames, prm, tpls, opt, factor, **kw):
        T.Case.__init__(self, id, frames, prm, tpls, opt, **kw)
        self.factor = factor

    @functools.lru_cache(maxsize=None)
    def expected(self):
        if self.factor == 0:
            return FR.expected(self.frames, self.prm, self.tpls, self.opt)
        return RR.expected(self.frames, self.prm, self.tpls, self.opt, self.factor)


@functools.lru_cache(maxsize=None)
def fused_case(slot, factor=FACTOR):
    prm = capi.default_params()
    prm.cluster_min_size = 30
    prm.icp_max_iterations = 12
    prm.template_slot = slot
    tpls = fused_templates()
    return RejectCase("fused-slot%d-f%g" % (slot, factor), fused_batch(), prm, tpls if slot < 0 else {slot: tpls[slot]}, FR.options(), factor)


def expected_stats(case):
    """Per frame, the stats tuple of every cluster's kept pair."""
    return [[RR.stats_tuple(RR.stats_of(c.pairs[c.slot])) for c in e["clusters"]] for e in case.expected()]
