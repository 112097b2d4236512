"""Canonical rule C19 in numpy: median-distance correspondence rejection inside the library's ICP (opt-in through
cd_set_icp_median_rejection).  This module is the specification of the rule's own arithmetic - the median, the threshold and the
keep predicate; it needs no GPU and no library.  perception_amd/csrc/icp_reject_math.hpp restates it for host and device,
k_icp_reject.hip runs it on the GPU, and both are compared with this module bit for bit.

One ICP iteration with a factor f (a finite double > 0) set.  The correspondences come from rule C5 (every source point's nearest
template point and the canonical float32 d2); rule C8's bound, when set, leaves the set K0 (all points otherwise):

  1. |K0| < 3: the ICP stops as rule C8 stops it (T = identity, not converged, Tfinal as it stands);
  2. m = the float32 d2 of rank floor(|K0| / 2) (0-based, ascending) over K0 - the upper median, no averaging;
  3. thr = (double) m * f, one rounded double product;
  4. a correspondence of K0 is kept iff (double) d2 <= thr;
  5. fewer than three kept: the stop of step 1;
  6. the moment sums, the MSE and the solve's n are over the kept correspondences only.

Everything else of the ICP is untouched (X <- T X for every point, Tfinal <- T Tfinal, the convergence tests, getFitnessScore over
all points).  d2 is never NaN under rule C5; +inf sorts last and thr may be +inf.

It restates pcl::registration::CorrespondenceRejectorMedianDistance as commonly described (nth_element at size / 2 over the squared
distances, keep <= median * factor, after the correspondence estimation's own bound); parity with a real PCL is unpinned.
"""
import numpy as np

MIN_CORR = 3                   # fewer kept correspondences stop the ICP (rule C8's stop)
FACTOR_OFF = 0.0               # cd_set_icp_median_rejection(ctx, 0): the mode is off
FACTOR_PCL_DEFAULT = 1.0       # CorrespondenceRejectorMedianDistance's own default factor

f32 = np.float32
f64 = np.float64


def valid_factor(factor):
    """A factor the setter accepts as "on": a finite double > 0."""
    f = f64(factor)
    return bool(np.isfinite(f) and f > 0)


def threshold(d2_kept0, factor):
    """(m, thr) of the float32 squared distances of K0 (at least one): steps 2 and 3."""
    d = np.asarray(d2_kept0, f32).reshape(-1)
    assert len(d) >= 1 and not np.isnan(d).any()
    m = np.partition(d, len(d) // 2)[len(d) // 2]
    with np.errstate(all="ignore"):
        thr = f64(m) * f64(factor)
    return f32(m), f64(thr)


def keep_mask(d2, factor, d2_max=None):
    """Steps 1 - 4 for one iteration's squared distances: (keep (bool per point), m, thr, n0).  d2_max: rule C8's float32
    threshold on d2 (None: unbounded).  With |K0| < 3 nothing is selected: keep is K0 itself, m and thr are None (the caller stops)."""
    d = np.asarray(d2, f32).reshape(-1)
    k0 = d <= f32(d2_max) if d2_max is not None else np.ones(len(d), bool)
    n0 = int(k0.sum())
    if n0 < MIN_CORR:
        return k0, None, None, n0
    m, thr = threshold(d[k0], factor)
    return k0 & (d.astype(f64) <= thr), m, thr, n0
