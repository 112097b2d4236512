"""Median-distance correspondence rejection (rule C19) on the GPU, through the C-ABI, against the reference composed on the CPU
(tests/reject_reference.py: the oracle's nearest neighbours and one-iteration solve over the kept points, perception_amd/icp_reject.py's
keep mask), bit for bit: T, iterations, converged, fitness, accepted, aligned points and stats - no tolerance.

  1. off is today's path: records and launch counts with the setter never called, with factor 0, and after on -> off;
  2. stand-alone cd_icp at the cluster sizes where the select kernel or the sliced driver takes another path, both templates;
  3. ties and edge values: all d2 zero, all d2 equal, half of them equal to the median;
  4. small factors: a stop at the first iteration and one at a later iteration;
  5. rule C8 together with rule C19: the rank is taken over the bound's survivors;
  6. the fused call, template_slot = -1 over a lattice and a scanned template and a single slot, stats per cluster included;
  7. the contamination scene through cd_icp;
  8. CD_GUESS_CLUSTER, and coarse-to-fine (rule C18) around the rule;
  9. refusals (rule C17 together with it, invalid factors), one context through on(4) -> on(1.5) -> off -> on(4), stats invalid while off.

The scenarios are tests/reject_scenarios.py's; tests/test_icp_reject_cpu.py asserts from the reference alone that each shows what it
is for."""
import numpy as np
import pytest

import coarse_reference as CR
import fused_reference as FR
import reject_reference as RR
import reject_scenarios as S
import test_gpu_fused_options as T
from perception_amd import capi, cluster_frame as cf, synth, templates

pytestmark = pytest.mark.gpu

f32 = np.float32


def check_icp(ctx, tpl, src, prm, factor, e, where, slot=0):
    """One cd_icp with the mode at `factor` against the reference record e (a dict of reject_reference.pair)."""
    ctx.set_icp_median_rejection(factor)
    assert ctx.icp_median_rejection() == factor
    st, r, al = ctx.icp(slot, src, prm, want_aligned=True)
    assert np.array_equal(np.asarray(list(r.T), f32).view(np.uint32), e["T"].view(np.uint32).ravel()), (where, "T")
    assert (r.size, r.iterations, r.converged, r.accepted, r.template_slot) == (len(src), e["iterations"], e["converged"], e["accepted"], slot), where
    assert T._bits(r.fitness) == T._bits(e["fitness"]), (where, r.fitness, e["fitness"])
    assert np.array_equal(al.view(np.uint32), np.asarray(e["aligned"], f32).view(np.uint32)), (where, "aligned")
    assert st == (capi.CD_ERR_FEW_CORRESPONDENCES if e["stopped"] else capi.CD_OK), where
    got = ctx.cluster_reject_stats(0)
    assert len(got) == 1 and RR.stats_tuple(got[0]) == RR.stats_tuple(e["reject_stats"]), (where, RR.stats_tuple(got[0]), e["reject_stats"])
    assert list(got[0].reserved) == [0, 0, 0], where
    return r


@pytest.fixture(scope="module", params=S.KINDS)
def kind_ctx(request):
    """One context per template kind, the template in slot 0, shared by the cd_icp tests of the kind."""
    tpl = S.template(request.param)
    c = capi.Context(max_points=4608, max_frames=1)
    c.set_template(0, tpl)
    yield request.param, tpl, c
    c.close()


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def test_off_is_todays_path(monkeypatch):
    frames = np.ascontiguousarray(np.stack([synth.frame(i, width=S.SW, height=S.SH) for i in range(4)]))
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    prm = capi.default_params()
    prm.cluster_min_size = 30

    def call(c):
        res, _, _ = c.process_batch(frames, prm)
        with pytest.raises(capi.CuboidError):
            c.cluster_reject_stats(0)
        return (bytes(capi.results_to_array(res)), [[bytes(k) for k in c.cluster_results(f)] for f in range(4)], c.timing().icp_kernel_launches,
                c.timing().icp_search, c.timing().icp_regime)
    never = T.make_ctx(monkeypatch, frames.shape[1], 4, {0: tpl})
    other = T.make_ctx(monkeypatch, frames.shape[1], 4, {0: tpl})
    try:
        base = call(never)
        assert sum(len(f) for f in base[1]) >= 4 and base[2] >= 1
        other.set_icp_median_rejection(0.0)
        assert other.icp_median_rejection() == 0.0 and call(other) == base
        other.set_icp_median_rejection(S.FACTOR)
        res, _, _ = other.process_batch(frames, prm)
        on = [[bytes(k) for k in other.cluster_results(f)] for f in range(4)]
        assert on != base[1] and other.timing().icp_search == 0 and sum(len(other.cluster_reject_stats(f)) for f in range(4)) == sum(len(f) for f in base[1])
        other.set_icp_median_rejection(None)
        assert call(other) == base
        assert call(never) == base
    finally:
        never.close()
        other.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def test_cd_icp_cluster_sizes(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    for n in S.SIZES:
        src = S.sized_source(kind, n, n)
        check_icp(c, tpl, src, prm, S.FACTOR, RR.pair(tpl, src, prm, S.FACTOR), "%s n=%d" % (kind, n))
    assert c.timing().icp_search == 0      # the generic search, also for the lattice template


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_ties_and_edge_values(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    sources = [("exact", S.exact_subset(kind))]
    if kind == "lattice":
        sources += [("shifted", S.shifted_face()), ("half", S.half_at_the_median())]
    for name, src in sources:
        for factor in (S.FACTOR, 1.0):
            check_icp(c, tpl, src, prm, factor, RR.pair(tpl, src, prm, factor), "%s %s f=%g" % (kind, name, factor))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_small_factors_stop(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    for name, src in (("at once", S.stops_at_once(kind)), ("later", S.stops_later(kind))):
        e = RR.pair(tpl, src, prm, S.SMALL_FACTOR)
        r = check_icp(c, tpl, src, prm, S.SMALL_FACTOR, e, "%s stop %s" % (kind, name))
        assert e["stopped"] and not r.converged and not r.accepted
    # the context goes on: an ordinary pair after the stops
    src = S.sized_source(kind, 65, 65)
    check_icp(c, tpl, src, prm, S.FACTOR, RR.pair(tpl, src, prm, S.FACTOR), "%s after the stops" % kind)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_bound_and_rejection_together(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    src, _ = S.near_and_far(kind)
    try:
        c.set_icp_max_correspondence_distance(S.BOUND)
        both = RR.pair(tpl, src, prm, S.FACTOR, d2_max=FR.correspondence_threshold(S.BOUND))
        r_both = check_icp(c, tpl, src, prm, S.FACTOR, both, "%s C8 + C19" % kind)
        c.set_icp_max_correspondence_distance(None)
        r_alone = check_icp(c, tpl, src, prm, S.FACTOR, RR.pair(tpl, src, prm, S.FACTOR), "%s C19 alone" % kind)
        assert list(r_both.T) != list(r_alone.T)
    finally:
        c.set_icp_max_correspondence_distance(None)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot", [-1, 1])
def test_fused_call(monkeypatch, slot):
    case = S.fused_case(slot)
    c = T.make_ctx(monkeypatch, case.N, case.F, case.tpls)
    try:
        c.set_icp_median_rejection(case.factor)
        snap = T.run(c, case)
        T.check(case, snap)
        stats = [[RR.stats_tuple(s) for s in c.cluster_reject_stats(f)] for f in range(case.F)]
        assert stats == S.expected_stats(case)
        K = len(stats[0])
        assert [RR.stats_tuple(s) for s in c.cluster_reject_stats(0, first=K - 2, count=5)] == stats[0][K - 2:] and c.cluster_reject_stats(0, first=K) == []
        with pytest.raises(capi.CuboidError):
            c.cluster_reject_stats(case.F)
        assert c.timing().icp_search == 0
    finally:
        c.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_contamination_scene(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    for seed in S.GPU_SCENE_SEEDS:
        src, truth = RR.contamination_scene(tpl, seed)
        on = check_icp(c, tpl, src, prm, S.FACTOR, RR.pair(tpl, src, prm, S.FACTOR), "%s scene %d" % (kind, seed))
        c.set_icp_median_rejection(0)
        st, off, _ = c.icp(0, src, prm)
        assert st == capi.CD_OK
        err = lambda r: RR.translation_error(np.array(list(r.T)).reshape(4, 4), truth)
        assert err(on) < err(off), (kind, seed, err(on), err(off))


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_cluster_guess_and_coarse_to_fine(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params(40)
    far = S.far_source(kind)
    g = np.asarray(cf.guess(cf.shape_frame(far), cf.shape_frame(tpl))[0], f32)
    guessed = FR.copy_params(prm)
    guessed.icp_use_guess = capi.CD_GUESS_CLUSTER
    check_icp(c, tpl, far, guessed, S.FACTOR, RR.pair(tpl, far, prm, S.FACTOR, guess=g), "%s cluster guess" % kind)
    src = S.coarse_source(kind)
    try:
        c.set_icp_coarse(*S.COARSE)
        fine, st = RR.coarse_pair(tpl, src, prm, S.FACTOR, S.COARSE)
        check_icp(c, tpl, src, prm, S.FACTOR, fine, "%s coarse-to-fine" % kind)
        got = c.cluster_coarse_stats(0)
        assert len(got) == 1 and CR.stats_tuple(got[0]) == CR.stats_tuple(st)
        fine, st = RR.coarse_pair(tpl, far, prm, S.FACTOR, (4, 64), guess_mode="cluster")
        c.set_icp_coarse(4, 64)
        check_icp(c, tpl, far, guessed, S.FACTOR, fine, "%s coarse-to-fine with the cluster guess" % kind)
        assert CR.stats_tuple(c.cluster_coarse_stats(0)[0]) == CR.stats_tuple(st)
    finally:
        c.set_icp_coarse(0)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    tpl = S.template("lattice")
    frames = S.fused_batch()[:1]
    c = T.make_ctx(monkeypatch, frames.shape[1], 1, {0: tpl})
    try:
        prm = S.icp_params()
        src = S.sized_source("lattice", 65, 65)
        c.set_icp_median_rejection(2.0)
        for bad in (float("nan"), -1.0, float("inf"), float("-inf")):
            with pytest.raises(capi.CuboidError) as ei:
                c.set_icp_median_rejection(bad)
            assert ei.value.status == capi.CD_ERR_INVALID_ARG
            assert c.icp_median_rejection() == 2.0          # a refused change keeps the old setting
        c.set_icp_plane_weight(capi.CD_ICP_PLANE_WEIGHT_DEFAULT)
        for call in (lambda: c.icp(0, src, prm), lambda: c.process_batch(frames, prm)):
            with pytest.raises(capi.CuboidError) as ei:
                call()
            assert ei.value.status == capi.CD_ERR_INVALID_ARG and "cd_set_icp_median_rejection" in str(ei.value) and "cd_set_icp_plane_weight" in str(ei.value)
        c.set_icp_plane_weight(None)
        check_icp(c, tpl, src, prm, 2.0, RR.pair(tpl, src, prm, 2.0), "after the refusals")
    finally:
        c.close()


def test_one_context_through_a_sequence_of_settings(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    src = S.sized_source(kind, 513, 513)
    for factor in (4.0, 1.5, 0.0, 4.0):
        if factor:
            check_icp(c, tpl, src, prm, factor, RR.pair(tpl, src, prm, factor), "%s sequence f=%g" % (kind, factor))
        else:
            c.set_icp_median_rejection(0.0)
            st, r, al = c.icp(0, src, prm, want_aligned=True)
            e = FR._pair(tpl, None, src, prm, FR.options(), None)
            assert st == capi.CD_OK and np.array_equal(np.asarray(list(r.T), f32).view(np.uint32), e["T"].view(np.uint32).ravel())
            assert (r.iterations, r.converged, T._bits(r.fitness)) == (e["iterations"], e["converged"], T._bits(e["fitness"]))
            assert np.array_equal(al.view(np.uint32), e["aligned"].view(np.uint32))
            with pytest.raises(capi.CuboidError):
                c.cluster_reject_stats(0)                    # the stats are invalid while the mode is off
