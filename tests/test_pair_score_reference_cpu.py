"""The scenarios of tests/test_gpu_pair_score.py show what they are for - asserted from the CPU reference alone
(tests/pair_score_reference.py: the oracle's results plus perception_amd/pair_score.py).  No GPU, no library."""
import numpy as np

import pair_score_scenarios as S
from perception_amd import capi, pair_score as PS

D, MIN_COV, MIN_INL = S.SETTING


def test_the_false_accept_and_the_right_template():
    """(a) From committed fixtures only.  The reference's values at the defaults (5 mm, coverage >= 0.5, inlier fraction >= 0.8):

        source (of marker_ascii.pcd)   template   accepted  fitness   coverage  inlier fraction  reverse_fitness  valid
        every second point, 299        clamp      1         6.4e-06   0.166     0.953           1.7e-03          0
        every second point, 299        marker     1         6.1e-07   1.000     1.000           1.4e-06          1
        lower 60 %, 358                clamp      1         5.4e-06   0.085     0.989           2.1e-03          0
        lower 60 %, 358                marker     1         5.9e-07   0.647     1.000           3.0e-04          1

    The acceptance threshold on the fitness is 4e-4: the marker on the clamp passes it by a factor of sixty."""
    for kind in ("half", "view"):
        r, wrong = S.scanned_pair(kind, "clamp")
        assert r.accepted == 1 and r.converged == 1 and r.fitness < 0.05 * capi.default_params().icp_accept_fitness
        assert wrong["status"] == 0 and wrong["coverage"] < 0.5 * MIN_COV and wrong["inlier_fraction"] > 0.9 and wrong["valid"] == 0
        r, right = S.scanned_pair(kind, "marker")
        assert r.accepted == 1 and right["status"] == 0 and right["coverage"] > 1.25 * MIN_COV and right["inlier_fraction"] == 1.0 and right["valid"] == 1
        assert wrong["reverse_fitness"] > 5 * right["reverse_fitness"]
    assert S.scanned_pair("half", "marker")[1]["coverage"] > 0.99
    assert 0.6 < S.scanned_pair("view", "marker")[1]["coverage"] < 0.7      # a 60 % view covers about 60 %


def test_shapes_name_every_path_of_the_kernel():
    """The stand-alone shapes: around a wave, a tile, two tiles, a row of lanes, and the smallest pairs that are split over
    workgroups in each direction; every random case has points inside and outside the range on both sides."""
    shapes = set(S.SHAPES)
    assert all((n, m) in shapes for n in S.SMALL for m in S.SMALL)
    for e in (S.PS_TILE - 1, S.PS_TILE, S.PS_TILE + 1, 2 * S.PS_TILE + 1, S.PS_THREADS - 1, S.PS_THREADS, S.PS_THREADS + 1):
        assert any(n == e for n, _ in shapes) and any(m == e for _, m in shapes), e
    assert S.PS_CHUNK + 1 in [n for n, _ in shapes] and S.PS_CHUNK + 1 in [m for _, m in shapes]        # one query more than an item holds
    assert len(shapes) == len(S.SHAPES)
    partly = 0
    for n, m in ((300, S.PS_TILE + 1), (S.PS_CHUNK + 1, S.PS_CHUNK + 1), (65, 63)):
        src, T, tpl, d = S.shape_case(n, m)
        o = PS.pair_score(src, T, tpl, d, 0, 0, 1)
        partly += 0 < o["n_source_in"] < n and 0 < o["n_template_in"] < m
    assert partly == 3
    src, T, tpl, d = S.tau_case()
    o = PS.pair_score(src, T, tpl, d, 0, 0, 1, want_distances=True)
    assert (o["f"] == PS.tau_of(d)).sum() == 1 and (o["r"] == PS.tau_of(d)).sum() == 1 and (o["n_source_in"], o["n_template_in"]) == (2, 2)
    src, T, tpl, d = S.tie_case()
    assert len(np.unique(tpl, axis=0)) * 3 == len(tpl) and len(np.unique(src, axis=0)) * 2 == len(src)


def test_fused_cases_score_every_cluster():
    """(b) Synthetic frames, template_slot = -1 over two loaded slots: every cluster of every frame has a score against the slot it
    kept - none is left out - both slots are kept by some cluster, accepted results exist on both sides of `valid`, and a frame
    has more clusters than its record holds."""
    for kind in S.FUSED_KINDS:
        case = S.fused_case(kind)
        exp = case.expected()
        assert case.prm.template_slot == -1 and sorted(case.tpls) == [0, 1]
        clusters = [(c, s) for e in exp for c, s in zip(e["clusters"], e["scores"])]
        skipped = sum(len(e["clusters"]) - len(e["scores"]) for e in exp) + sum(e["counts"][4] - len(e["clusters"]) for e in exp)
        assert skipped == 0 and len(clusters) >= 10
        assert max(e["counts"][4] for e in exp) > capi.CD_MAX_CLUSTERS_PER_FRAME
        assert {c.slot for c, _ in clusters} == {0, 1}
        for c, s in clusters:
            assert s["status"] == 0 and (s["n_source"], s["n_template"]) == (c.size, len(case.tpls[c.slot]))
            assert s["valid"] == int(c.accepted and s["coverage"] >= MIN_COV and s["inlier_fraction"] >= MIN_INL)
        accepted = [s for c, s in clusters if c.accepted]
        assert any(s["valid"] for s in accepted) and any(not s["valid"] for s in accepted), kind
    # what the combinations add: pairs that rule C8 stopped keep their start T and are scored; rule C18 ran a coarse level
    stopped = [(c, s) for e in S.fused_case("bound").expected() for c, s in zip(e["clusters"], e["scores"]) if c.stopped]
    assert stopped and all(s["status"] == 0 and s["n_template_in"] == 0 and not s["valid"] for _, s in stopped)
    assert any(c.coarse_stats.used for e in S.fused_case("coarse").expected() for c in e["clusters"])
    assert any(c.guess_flip >= 0 for e in S.fused_case("cluster_guess").expected() for c in e["clusters"])
    # the modes do change T: the scores of the same clusters differ between the cases
    alone = [s for e in S.fused_case("alone").expected() for s in e["scores"]]
    for kind in ("bound", "cluster_guess", "coarse"):
        other = [s for e in S.fused_case(kind).expected() for s in e["scores"]]
        assert len(other) == len(alone) and other != alone, kind


def test_few_points_and_an_empty_slot():
    """(c)"""
    e = S.tiny_case().expected()[0]
    sizes = [c.size for c in e["clusters"]]
    assert min(sizes) == 1 and 2 in sizes and max(sizes) >= 3 and len(e["scores"]) == len(sizes)
    for c, s in zip(e["clusters"], e["scores"]):
        zero = dict(PS._record(c.size, len(S.tiny_case().tpls[0]), PS.CD_ERR_FEW_CORRESPONDENCES))
        assert (s == zero) if c.size < 3 else (s["status"] == 0 and s["n_source"] == c.size)
    case = S.empty_slot_case()
    assert case.prm.template_slot not in case.tpls
    e = case.expected()[0]
    assert len(e["clusters"]) >= 2 and len(e["scores"]) == len(e["clusters"])
    for c, s in zip(e["clusters"], e["scores"]):
        assert c.size >= 3 and c.accepted == 0 and c.slot == case.prm.template_slot
        assert s == dict(PS._record(c.size, 0, PS.CD_ERR_NO_TEMPLATE))
