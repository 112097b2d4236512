"""Reciprocal correspondences (rule C22) on the GPU, through the C-ABI, against the reference composed on the CPU
(tests/recip_reference.py: the oracle's nearest neighbours and one-iteration solve over the kept points, perception_amd/icp_reciprocal.py's
keep mask), bit for bit: T, iterations, converged, fitness, accepted, aligned points, status and stats - no tolerance.

  1. off is today's path: records and launch counts with the setter never called, with 0, and after on -> off;
  2. stand-alone cd_icp at the cluster sizes where the kernels or the sliced driver take another path, both templates, and a
     source whose queries are split over four workgroups;
  3. ties and duplicated source points: the lower index is kept;
  4. a stop at the first iteration and one at the second;
  5. rule C8 together with rule C22;
  6. the fused call for slots 0, 1 and -1, stats per cluster included;
  7. the contamination scene through cd_icp;
  8. CD_GUESS_CLUSTER (rule C13), and coarse-to-fine (rule C18) around the rule;
  9. both refused combinations, one context through on -> off -> on, stats invalid while off.

The scenarios are tests/recip_scenarios.py's; tests/test_icp_recip_cpu.py asserts from the reference alone that each shows what it
is for."""
import numpy as np
import pytest

import coarse_reference as CR
import fused_reference as FR
import recip_reference as QR
import recip_scenarios as S
import reject_reference as RR
import test_gpu_fused_options as T
from perception_amd import capi, cluster_frame as cf, synth, templates

pytestmark = pytest.mark.gpu

f32 = np.float32


def check_icp(ctx, tpl, src, prm, e, where, slot=0):
    """One cd_icp with the mode on against the reference record e (a dict of recip_reference.pair)."""
    ctx.set_icp_reciprocal(True)
    assert ctx.icp_reciprocal() == 1
    st, r, al = ctx.icp(slot, src, prm, want_aligned=True)
    assert np.array_equal(np.asarray(list(r.T), f32).view(np.uint32), e["T"].view(np.uint32).ravel()), (where, "T")
    assert (r.size, r.iterations, r.converged, r.accepted, r.template_slot) == (len(src), e["iterations"], e["converged"], e["accepted"], slot), where
    assert T._bits(r.fitness) == T._bits(e["fitness"]), (where, r.fitness, e["fitness"])
    assert np.array_equal(al.view(np.uint32), np.asarray(e["aligned"], f32).view(np.uint32)), (where, "aligned")
    assert st == (capi.CD_ERR_FEW_CORRESPONDENCES if e["stopped"] else capi.CD_OK), where
    got = ctx.cluster_recip_stats(0)
    assert len(got) == 1 and QR.stats_tuple(got[0]) == QR.stats_tuple(e["recip_stats"]), (where, QR.stats_tuple(got[0]), e["recip_stats"])
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
            c.cluster_recip_stats(0)
        return (bytes(capi.results_to_array(res)), [[bytes(k) for k in c.cluster_results(f)] for f in range(4)], c.timing().icp_kernel_launches,
                c.timing().icp_search, c.timing().icp_regime)
    never = T.make_ctx(monkeypatch, frames.shape[1], 4, {0: tpl})
    other = T.make_ctx(monkeypatch, frames.shape[1], 4, {0: tpl})
    try:
        base = call(never)
        assert sum(len(f) for f in base[1]) >= 4 and base[2] >= 1
        other.set_icp_reciprocal(False)
        assert other.icp_reciprocal() == 0 and call(other) == base
        other.set_icp_reciprocal(True)
        res, _, _ = other.process_batch(frames, prm)
        on = [[bytes(k) for k in other.cluster_results(f)] for f in range(4)]
        assert on != base[1] and other.timing().icp_search == 0 and sum(len(other.cluster_recip_stats(f)) for f in range(4)) == sum(len(f) for f in base[1])
        other.set_icp_reciprocal(None)
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
        check_icp(c, tpl, src, prm, QR.pair(tpl, src, prm), "%s n=%d" % (kind, n))
    assert c.timing().icp_search == 0      # the generic search, also for the lattice template


def test_source_split_over_workgroups(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    src = S.split_source(kind)
    r = check_icp(c, tpl, src, prm, QR.pair(tpl, src, prm), "%s split" % kind)
    assert r.size > 3 * S.RC_CHUNK


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_ties_and_duplicates(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    sources = [("exact", S.exact_subset(kind)), ("duplicates", S.duplicate_source(kind)[0])]
    if kind == "lattice":
        sources.append(("ties", S.tie_source()[0]))
    for name, src in sources:
        check_icp(c, tpl, src, prm, QR.pair(tpl, src, prm), "%s %s" % (kind, name))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_stops(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    for name, src in (("at once", S.corner_ball(kind)), ("later", S.stops_later(kind))):
        e = QR.pair(tpl, src, prm)
        r = check_icp(c, tpl, src, prm, e, "%s stop %s" % (kind, name))
        assert e["stopped"] and not r.converged and not r.accepted
    # the context goes on: an ordinary pair after the stops
    src = S.sized_source(kind, 65, 65)
    check_icp(c, tpl, src, prm, QR.pair(tpl, src, prm), "%s after the stops" % kind)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_bound_and_reciprocal_together(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    d2_max = FR.correspondence_threshold(S.BOUND)
    try:
        for name, (src, _) in (("near and far", S.near_and_far(kind)),) + ((("half and far", S.half_and_far(kind)),) if kind == "lattice" else ()):
            c.set_icp_max_correspondence_distance(S.BOUND)
            check_icp(c, tpl, src, prm, QR.pair(tpl, src, prm, d2_max=d2_max), "%s C8 + C22 %s" % (kind, name))
            assert c.cluster_recip_stats(0)[0].last_n0 < len(src)
            c.set_icp_max_correspondence_distance(None)
            check_icp(c, tpl, src, prm, QR.pair(tpl, src, prm), "%s C22 alone %s" % (kind, name))
            assert c.cluster_recip_stats(0)[0].last_n0 == len(src)
    finally:
        c.set_icp_max_correspondence_distance(None)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot", [0, 1, -1])
def test_fused_call(monkeypatch, slot):
    case = S.fused_case(slot)
    c = T.make_ctx(monkeypatch, case.N, case.F, case.tpls)
    try:
        c.set_icp_reciprocal(True)
        snap = T.run(c, case)
        T.check(case, snap)
        stats = [[QR.stats_tuple(s) for s in c.cluster_recip_stats(f)] for f in range(case.F)]
        assert stats == S.expected_stats(case)
        K = len(stats[0])
        assert [QR.stats_tuple(s) for s in c.cluster_recip_stats(0, first=K - 2, count=5)] == stats[0][K - 2:] and c.cluster_recip_stats(0, first=K) == []
        with pytest.raises(capi.CuboidError):
            c.cluster_recip_stats(case.F)
        assert c.timing().icp_search == 0
    finally:
        c.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_contamination_scene(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    for seed in S.GPU_SCENE_SEEDS:
        src, truth = RR.contamination_scene(tpl, seed)
        on = check_icp(c, tpl, src, prm, QR.pair(tpl, src, prm), "%s scene %d" % (kind, seed))
        c.set_icp_reciprocal(False)
        st, off, _ = c.icp(0, src, prm)
        assert st == capi.CD_OK
        err = lambda r: RR.translation_error(np.array(list(r.T)).reshape(4, 4), truth)
        assert err(on) < 0.5 * err(off), (kind, seed, err(on), err(off))


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_cluster_guess_and_coarse_to_fine(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params(40)
    far = S.far_source(kind)
    g = np.asarray(cf.guess(cf.shape_frame(far), cf.shape_frame(tpl))[0], f32)
    guessed = FR.copy_params(prm)
    guessed.icp_use_guess = capi.CD_GUESS_CLUSTER
    check_icp(c, tpl, far, guessed, QR.pair(tpl, far, prm, guess=g), "%s cluster guess" % kind)
    src = S.coarse_source(kind)
    try:
        c.set_icp_coarse(*S.COARSE)
        fine, st = QR.coarse_pair(tpl, src, prm, S.COARSE)
        check_icp(c, tpl, src, prm, fine, "%s coarse-to-fine" % kind)
        got = c.cluster_coarse_stats(0)
        assert len(got) == 1 and CR.stats_tuple(got[0]) == CR.stats_tuple(st)
        fine, st = QR.coarse_pair(tpl, far, prm, (4, 64), guess_mode="cluster")
        c.set_icp_coarse(4, 64)
        check_icp(c, tpl, far, guessed, fine, "%s coarse-to-fine with the cluster guess" % kind)
        assert CR.stats_tuple(c.cluster_coarse_stats(0)[0]) == CR.stats_tuple(st)
    finally:
        c.set_icp_coarse(0)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_refused_combinations(monkeypatch):
    tpl = S.template("lattice")
    frames = S.fused_batch()[:1]
    c = T.make_ctx(monkeypatch, frames.shape[1], 1, {0: tpl})
    try:
        prm = S.icp_params()
        src = S.sized_source("lattice", 65, 65)
        c.set_icp_reciprocal(True)
        for other, on, off in (("cd_set_icp_plane_weight", lambda: c.set_icp_plane_weight(capi.CD_ICP_PLANE_WEIGHT_DEFAULT), lambda: c.set_icp_plane_weight(None)),
                               ("cd_set_icp_median_rejection", lambda: c.set_icp_median_rejection(4.0), lambda: c.set_icp_median_rejection(0))):
            on()
            for call in (lambda: c.icp(0, src, prm), lambda: c.process_batch(frames, prm)):
                with pytest.raises(capi.CuboidError) as ei:
                    call()
                assert ei.value.status == capi.CD_ERR_INVALID_ARG and "cd_set_icp_reciprocal" in str(ei.value) and other in str(ei.value)
            assert c.icp_reciprocal() == 1          # a refused call keeps the settings
            off()
            check_icp(c, tpl, src, prm, QR.pair(tpl, src, prm), "after the refusal with " + other)
    finally:
        c.close()


def test_one_context_through_on_off_on(kind_ctx):
    kind, tpl, c = kind_ctx
    prm = S.icp_params()
    src = S.sized_source(kind, 513, 513)
    for on in (True, False, True):
        if on:
            check_icp(c, tpl, src, prm, QR.pair(tpl, src, prm), "%s sequence on" % kind)
        else:
            c.set_icp_reciprocal(False)
            st, r, al = c.icp(0, src, prm, want_aligned=True)
            e = FR._pair(tpl, None, src, prm, FR.options(), None)
            assert st == capi.CD_OK and np.array_equal(np.asarray(list(r.T), f32).view(np.uint32), e["T"].view(np.uint32).ravel())
            assert (r.iterations, r.converged, T._bits(r.fitness)) == (e["iterations"], e["converged"], T._bits(e["fitness"]))
            assert np.array_equal(al.view(np.uint32), e["aligned"].view(np.uint32))
            with pytest.raises(capi.CuboidError):
                c.cluster_recip_stats(0)                    # the stats are invalid while the mode is off
