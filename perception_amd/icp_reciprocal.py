"""Canonical rule C22 in numpy: reciprocal correspondences inside the library's ICP (opt-in through cd_set_icp_reciprocal).  This
module is the specification of the rule's own arithmetic - the reverse nearest-neighbour test and the keep predicate; it needs no
GPU and no library.  perception_amd/csrc/icp_recip_math.hpp restates it for host and device, k_icp_recip.hip runs it on the GPU, and
both are compared with this module bit for bit.

One ICP iteration with the mode on.  Rule C5 has given every source point i of the n current positions X its template point j_i
and the canonical float32 d2_i; rule C8's bound, when set, leaves the set K0 (all points otherwise):

  1. |K0| < 3: the ICP stops as rule C8 stops it (T = identity, not converged, Tfinal as it stands);
  2. for every i of K0, r_i = the index of the source point nearest to q = tpl[j_i] among ALL n current positions (inside K0 or
     not), with d2(q, x) = (dx dx + dy dy) + dz dz in float32, dx = q.x - x.x, every operation rounded on its own, ties to the
     lowest source index;
  3. i is kept iff r_i == i: no i' has d2(q, X_i') < d2(q, X_i) and no i' < i has an equal one;
  4. fewer than three kept: the stop of step 1;
  5. the moment sums, the MSE and the solve's n are over the kept correspondences only.

Everything else of the ICP is untouched (X <- T X for every point, Tfinal <- T Tfinal, the convergence tests, getFitnessScore over
all points).

It restates pcl::IterativeClosestPoint::setUseReciprocalCorrespondences(true) (CorrespondenceEstimation::
determineReciprocalCorrespondences) as commonly described; parity with a real PCL is unpinned (k-d tree ties).  PCL runs its
rejectors on what the reciprocal estimation left; here the mode is not combined with rules C17 and C19.
"""
import numpy as np

MIN_CORR = 3                   # fewer kept correspondences stop the ICP (rule C8's stop)
_ROWS = 256                    # queries per block of the distance matrix

f32 = np.float32


def d2_matrix(queries, targets):
    """d2(q, x) of step 2 for every (query, target) pair: float32, one rounding per operation."""
    q = np.ascontiguousarray(queries, f32).reshape(-1, 3)
    t = np.ascontiguousarray(targets, f32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = q[:, 0, None] - t[None, :, 0]
        dy = q[:, 1, None] - t[None, :, 1]
        dz = q[:, 2, None] - t[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == f32
    return d2


def forward(X, tpl):
    """Rule C5 by brute force: (nn int32, d2 float32) of every source point, ties to the lowest template index."""
    X = np.ascontiguousarray(X, f32).reshape(-1, 3)
    nn = np.empty(len(X), np.int32)
    d2 = np.empty(len(X), f32)
    for r0 in range(0, len(X), _ROWS):
        D = d2_matrix(X[r0:r0 + _ROWS], tpl)
        j = D.argmin(axis=1)
        nn[r0:r0 + _ROWS] = j
        d2[r0:r0 + _ROWS] = D[np.arange(len(j)), j]
    return nn, d2


def keep_mask(X, tpl, nn, d2, d2_max=None):
    """Steps 1 - 3 for one iteration: (keep (bool per point), n0).  X: the n current source positions; tpl: the template; nn, d2:
    rule C5's neighbour (an index into tpl) and float32 squared distance of every source point; d2_max: rule C8's float32 threshold
    on d2 (None: unbounded).  With |K0| < 3 nothing is tested: keep is K0 itself (the caller stops)."""
    X = np.ascontiguousarray(X, f32).reshape(-1, 3)
    tpl = np.ascontiguousarray(tpl, f32).reshape(-1, 3)
    nn = np.asarray(nn).reshape(-1).astype(np.int64)
    d = np.asarray(d2, f32).reshape(-1)
    n = len(X)
    assert len(nn) == n and len(d) == n
    with np.errstate(invalid="ignore"):
        k0 = d <= (f32(d2_max) if d2_max is not None else f32(np.inf))
    n0 = int(k0.sum())
    if n0 < MIN_CORR:
        return k0, n0
    keep = np.zeros(n, bool)
    idx = np.flatnonzero(k0)
    col = np.arange(n)
    for r0 in range(0, len(idx), _ROWS):
        i = idx[r0:r0 + _ROWS]
        D = d2_matrix(tpl[nn[i]], X)                    # queries: the template points; targets: every source point
        own = D[np.arange(len(i)), i]
        with np.errstate(invalid="ignore"):
            closer = (D < own[:, None]).any(axis=1)
            tie_before = ((D == own[:, None]) & (col[None, :] < i[:, None])).any(axis=1)
        keep[i] = ~closer & ~tie_before
    return keep, n0
