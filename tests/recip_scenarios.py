"""The scenarios of tests/test_gpu_icp_recip.py (rule C22 on the GPU), as plain CPU code: sources, settings and fused cases.
tests/test_icp_recip_cpu.py imports them and asserts, from the reference alone (tests/recip_reference.py), that each shows what it
is for; the GPU tests then compare the library with the same reference bit for bit.  Templates, sized sources and the fused batch
are tests/reject_scenarios.py's: the two rules are offered for the same scenes."""
import functools

import numpy as np

import fused_reference as FR
import recip_reference as QR
import reject_scenarios as S
import test_gpu_fused_options as T
from perception_amd import capi

f32 = np.float32
KINDS = S.KINDS
template = S.template
icp_params = S.icp_params
ICP_QSLICE, RC_THREADS, RC_CHUNK = 512, 256, 512    # common.hpp, k_icp_recip.hip
# cd_icp sizes: the least legal ones, around a wave, around the workgroup (one query row a lane or two), around a slice - which
# is also the chunk of queries one workgroup takes (513: a second workgroup with a single query; 1025: a third) - and nine
# chunks: tiles before the chunk, the chunk's own and tiles behind it, the last one partial
# (10 and 14: a last tile that the +inf padding fills up by 6 and by 2 points - the tile is padded to a multiple of 8)
SIZES = (3, 4, 5, 10, 14, 63, 64, 65, RC_THREADS - 1, RC_THREADS, RC_THREADS + 1, ICP_QSLICE - 1, ICP_QSLICE, ICP_QSLICE + 1, 2 * RC_CHUNK + 1, 4099)
SCENE_SEEDS = (2, 3, 4, 5)         # the contamination scene of tests/reject_reference.py; the GPU runs the first two of each template
GPU_SCENE_SEEDS = SCENE_SEEDS[:2]
SPLIT_SIZE = 3 * RC_CHUNK + 77     # a source larger than one work split: four workgroups of queries


def sized_source(kind, n, seed):
    return S.sized_source(kind, n, seed)


def exact_subset(kind):
    """reject_scenarios.exact_subset without the points that repeat another's coordinates (the lattice template holds the points of
    an edge once per face): distinct template points, so every d2 is 0 and every point is its template point's only nearest source."""
    pts = S.exact_subset(kind)
    _, first = np.unique(pts, axis=0, return_index=True)
    return np.ascontiguousarray(pts[np.sort(first)])


def split_source(kind):
    """More points than one workgroup takes as queries, so that a cluster's flags come from several workgroups."""
    return S.sized_source(kind, SPLIT_SIZE, 91)


# ---- ties and duplicates -----------------------------------------------------------------------------------------------------------
def tie_source(n=150, seed=12, delta=2.0 ** -8):
    """Pairs of points on either side of a lattice face, delta along its normal from the same template point q: both have q as their
    neighbour and d2 with the same bits, so q's nearest source is a tie that the lower index wins.  The pairs are laid out so that
    the lower index is the outer point for even pairs and the inner one for odd pairs.  Returns (source, the template points)."""
    pts, w = S._interior_face_points(n, seed)
    out = np.repeat(pts, 2, axis=0).copy()
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(f32)
    out[0::2, w] += sign * f32(delta)
    out[1::2, w] -= sign * f32(delta)
    return np.ascontiguousarray(out), pts


def duplicate_source(kind, n=300, n_dup=120, seed=14):
    """A sized source followed by copies of n_dup of its points, and the index of each copy's original: a copy is never kept."""
    src = S.sized_source(kind, n, seed)
    pick = np.sort(np.random.default_rng(seed).choice(n, n_dup, replace=False))
    return np.ascontiguousarray(np.vstack([src, src[pick]])), pick


# ---- stops --------------------------------------------------------------------------------------------------------------------------
def corner_ball(kind, n=40, distance=0.03, radius=0.002, seed=21):
    """A tight ball beyond the template's corner towards (1, 1, 1): every point has the corner as its neighbour, one is kept."""
    tpl = template(kind).astype(np.float64)
    corner = tpl[np.argmax(tpl.sum(axis=1))]
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d *= (radius * rng.uniform(size=n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    return np.ascontiguousarray((corner + distance / np.sqrt(3.0) + d).astype(f32))


# (points, seed) of stops_later, found by a search on the CPU reference over 6, 8, 12 and 20 points and seeds 0 .. 299: about one
# candidate in a hundred keeps three at first and fewer after the first step; none went on for longer
LATER_STOP = {"lattice": (12, 212), "scanned": (12, 2)}


def stops_later_candidate(kind, n, seed, radius=0.002, distance=0.02):
    """n points in a ball of 2 mm, 2 cm from a template point in a random direction: at most a handful of template points share
    them out."""
    tpl = template(kind).astype(np.float64)
    rng = np.random.default_rng(700 + seed)
    q = tpl[rng.integers(len(tpl))]
    d = rng.normal(size=(n, 3))
    d *= (radius * rng.uniform(size=n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    off = rng.normal(size=3)
    off *= distance / np.linalg.norm(off)
    return np.ascontiguousarray((q + off + d).astype(f32))


def stops_later(kind):
    """A source that keeps three correspondences at the first iteration, takes that step, and keeps fewer at the second."""
    return stops_later_candidate(kind, *LATER_STOP[kind])


# ---- combinations ----------------------------------------------------------------------------------------------------------------
BOUND = S.BOUND
COARSE = S.COARSE
near_and_far = S.near_and_far     # (the far points are not reciprocal anyway: the bound changes |K0| and the stats, not the pose)


def half_and_far(kind, n_near=200, n_far=60, seed=33):
    """near_and_far along the template's longest axis a, with the near points taken from its lowest quarter only and, as far points,
    the n_far template points nearest its upper end moved along a onto the plane 2.5 cm beyond it: each is beyond the bound, and
    most are the nearest source of their template neighbour - reciprocal, so only the bound removes them.  Returns (source, the
    mask of P)."""
    tpl = template(kind)
    rng = np.random.default_rng(seed)
    hi = tpl.max(axis=0).astype(np.float64)
    lo = tpl.min(axis=0).astype(np.float64)
    a = int(np.argmax(hi - lo))
    low = np.flatnonzero(tpl[:, a] < lo[a] + 0.25 * (hi[a] - lo[a]))
    P = S.moved(tpl[rng.choice(low, n_near, replace=False)], seed, angle_deg=1.0, shift=0.002)
    Q = tpl[np.argsort(-tpl[:, a], kind="stable")[:n_far]].copy()
    Q[:, a] = f32(hi[a] + 0.025)
    src = np.ascontiguousarray(np.vstack([P, Q]))
    order = rng.permutation(len(src))
    mask = np.r_[np.ones(n_near, bool), np.zeros(len(Q), bool)]
    return np.ascontiguousarray(src[order]), mask[order]


coarse_source = S.coarse_source
far_source = S.far_source

# ---- the fused call -----------------------------------------------------------------------------------------------------------------
SW, SH = S.SW, S.SH
fused_templates = S.fused_templates
fused_batch = S.fused_batch


class RecipCase(T.Case):
    """A fused call with rule C22 on (on = False: off)."""

    def __init__(self, id, frames, prm, tpls, opt, on, **kw):
        T.Case.__init__(self, id, frames, prm, tpls, opt, **kw)
        self.on = on

    @functools.lru_cache(maxsize=None)
    def expected(self):
        if not self.on:
            return FR.expected(self.frames, self.prm, self.tpls, self.opt)
        return QR.expected(self.frames, self.prm, self.tpls, self.opt)


@functools.lru_cache(maxsize=None)
def fused_case(slot, on=True):
    prm = capi.default_params()
    prm.cluster_min_size = 30
    prm.icp_max_iterations = 12
    prm.template_slot = slot
    tpls = fused_templates()
    return RecipCase("recip-fused-slot%d-%s" % (slot, "on" if on else "off"), fused_batch(), prm, tpls if slot < 0 else {slot: tpls[slot]}, FR.options(), on)


def expected_stats(case):
    """Per frame, the stats tuple of every cluster's kept pair."""
    return [[QR.stats_tuple(QR.stats_of(c.pairs[c.slot])) for c in e["clusters"]] for e in case.expected()]
