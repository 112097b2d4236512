"""The composed reference of coarse-to-fine ICP (tests/coarse_reference.py) on the CPU: with the mode off it is fused_reference
itself, and every scenario of tests/test_gpu_icp_coarse.py shows what it is there to show - asserted here from the reference alone,
so that a scenario that shows nothing fails before it reaches a GPU.

Every scenario has an eligible pair whose two-level record differs in the bits of T from its single-level record, and - in one
frame with such a pair - an ineligible cluster that equals its single-level record.  What else a scenario shows is in its
`shows`: a pair that falls back under a bound that leaves its coarse set fewer than three correspondences, or a cluster whose
kept slot is chosen on the fine fitness.  Each of those is asserted for the scenarios that name it, and some scenario names it.

The issue that asked for the mode words this as "each scenario must contain" all four.  Read literally that cannot be met: the
reference can state a bound only together with rule C17 (fused_reference's docstring), so a scenario "with the mode alone" has no
bound to fall back under, and a scenario with one template has no choice among slots.  So the first two properties are asserted
of every scenario, the other two of the scenarios built for them, and test_some_scenario_shows_each_property holds that none of
the four is left without a scenario."""
import numpy as np
import pytest

import coarse_reference as CR
import fused_reference as FR
import test_gpu_icp_coarse as G
from perception_amd import capi, icp_coarse as IC


def _bits(T):
    return np.asarray(T, np.float32).view(np.uint32).tobytes()


def _same_record(a, b):
    return (_bits(a["T"]) == _bits(b["T"]) and (a["iterations"], a["converged"], a["accepted"]) == (b["iterations"], b["converged"], b["accepted"]) and
            np.float64(a["fitness"]).view(np.uint64) == np.float64(b["fitness"]).view(np.uint64) and
            np.array_equal(np.asarray(a["aligned"]).view(np.uint32), np.asarray(b["aligned"]).view(np.uint32)))


def test_some_scenario_shows_each_property():
    shown = set()
    for name in G.SCENARIOS:
        shown.update(G.scenario(name).shows)
    assert shown == {"fall_back", "fine_choice"}
    guesses = {G.scenario(name).opt["guess"] for name in G.SCENARIOS}
    assert guesses == set(FR.GUESS_MODES)                                   # every guess mode the reference can express
    assert any(G.scenario(n).opt["plane"] is None for n in G.SCENARIOS) and any(G.scenario(n).opt["bound"] is not None for n in G.SCENARIOS)
    assert {G.scenario(n).prm.template_slot for n in G.SCENARIOS} == {0, -1}
    assert {G.scenario(n).coarse[0] for n in G.SCENARIOS} >= {2, 3, 4, 5}   # strides that do and do not divide the sizes
    # the single guess of cd_params: alone and with a bound to fall back under
    single = [n for n in G.SCENARIOS if G.scenario(n).prm.icp_use_guess == capi.CD_GUESS_PARAMS]
    assert sorted(single) == ["params", "params-bound"] and "fall_back" in G.scenario("params-bound").shows
    for n in single:
        case = G.scenario(n)
        g = np.array(list(case.prm.icp_guess), np.float32).reshape(4, 4)
        assert case.opt["guess"] == "per_frame" and all(np.array_equal(f, g) for f in case.opt["frame_guesses"]) and not np.array_equal(g, FR.IDENT)


@pytest.mark.parametrize("name", G.SCENARIOS + ("alone-t1",))
def test_scenario_shows_what_it_is_for(name):
    case = G.scenario(name)
    s, m = case.coarse
    assert IC.setting_ok(s, m) and s >= 2
    two, one = case.expected(), case.single()
    assert 1 <= case.F <= 4 and len(two) == len(one) == case.F
    differs, mixed_frame, fell_back, fine_choice, eligible_pairs, kept_stats = 0, 0, 0, 0, 0, 0
    for e2, e1 in zip(two, one):
        assert e2["counts"] == e1["counts"] and np.array_equal(e2["labels"], e1["labels"])      # the front end does not know the mode
        frame_differs, frame_equal_ineligible = 0, 0
        for c2, c1 in zip(e2["clusters"], e1["clusters"]):
            assert c2.size == c1.size and sorted(c2.pairs) == sorted(c1.pairs)
            for slot in c2.pairs:
                p2, p1, st = c2.pairs[slot], c1.pairs[slot], CR.coarse_stats_of(c2.pairs[slot])
                assert (st.used != IC.NOT_ELIGIBLE) == (c2.size >= m) and st.n_coarse == (-(-c2.size // s) if c2.size >= m else 0)
                if st.used == IC.NOT_ELIGIBLE:
                    assert _same_record(p2, p1)
                    frame_equal_ineligible += 1
                    continue
                eligible_pairs += 1
                if st.used == IC.USED and _bits(p2["T"]) != _bits(p1["T"]):
                    differs += 1
                    frame_differs += 1
                if st.used == IC.FELL_BACK:
                    # the coarse ICP stopped; from the call's own guess the fine level is the single-level ICP
                    assert st.coarse_status == capi.CD_ERR_FEW_CORRESPONDENCES and st.coarse_converged == 0 and _same_record(p2, p1)
                    if case.opt["bound"] is not None and st.coarse_iterations == 0:
                        fell_back += 1
            kept = CR.coarse_stats_of(c2.pairs[c2.slot])
            kept_stats += kept.used != IC.NOT_ELIGIBLE
            if len(c2.pairs) > 1 and kept.used == IC.USED:
                slots = sorted(c2.pairs)
                by_fine = min(slots, key=lambda t: (c2.pairs[t]["fitness"], t))
                by_coarse = min(slots, key=lambda t: (CR.coarse_stats_of(c2.pairs[t]).coarse_fitness, t))
                assert c2.slot == by_fine
                if by_fine != by_coarse:
                    fine_choice += 1
        mixed_frame += bool(frame_differs and frame_equal_ineligible)
    assert differs >= 1 and mixed_frame >= 1 and kept_stats >= 1, (name, differs, mixed_frame)
    if "fall_back" in case.shows:
        assert fell_back >= 1 and fell_back < eligible_pairs, name
    if "fine_choice" in case.shows:
        assert fine_choice >= 1, name
    if name == "filter-big":   # the filter is on and the coarse sets end past what a context without the mode holds
        need, plain = G.filter_big_needs(case)
        assert case.opt["filter"] is not None and plain < need <= plain + 16 + (2 * plain + 2) // 3
    if name in ("passes", "filter-big"):       # two copies of the sources do not fit the frame: one ICP pass per template
        assert case.prm.template_slot == -1 and all(2 * sum(c.size for c in e["clusters"]) > case.N for e in two)


def test_mode_off_is_fused_reference():
    case = G.scenario("surface")
    off = CR.expected(case.frames, case.prm, case.tpls, case.opt, (0, 0))
    for e0, e1 in zip(off, case.single()):
        for c0, c1 in zip(e0["clusters"], e1["clusters"]):
            assert c0.slot == c1.slot and all(_same_record(c0.pairs[t], c1.pairs[t]) for t in c0.pairs)
            assert CR.coarse_stats_of(c0) == IC.NO_STATS
    assert FR._pair is CR.SINGLE_PAIR


def test_cd_icp_cases_cover_the_edges():
    """The sizes of test_cd_icp_two_levels: each stride sees n = m - 1, m, m + 1 at both values of min_points, the three- and
    four-point coarse sets, a size the stride does not divide, and an ineligible 3 s / 3 s + 1."""
    tpls = G.icp_templates()
    assert len(tpls["arbitrary"]) == 597 and capi.lattice_detect(tpls["lattice"]) and not capi.lattice_detect(tpls["arbitrary"])
    for s in (2, 5, 64):
        sizes = G.icp_sizes(s)
        for m in {m for m, _ in sizes}:
            assert IC.setting_ok(s, m) and {m - 1, m, m + 1} <= {n for mm, n in sizes if mm == m}
        assert (3 * s, 3 * s) in sizes and (3 * s, 3 * s + 1) in sizes and any(n % s and n >= m for m, n in sizes)
        assert {len(IC.subsample(n, s, m)) for m, n in sizes} >= {0, 3, 4}
        assert max(n for _, n in sizes) <= 1024
