"""The composed reference of the fused call (tests/fused_reference.py) on the CPU: with every option off it is the oracle's
process_frame, and every scenario of tests/test_gpu_fused_options.py shows what it is there to show - asserted here from the
reference alone, so that a scenario that shows nothing fails before it reaches a GPU."""
import itertools

import numpy as np
import pytest

import fused_reference as FR
import test_gpu_fused_options as S
from perception_amd import capi, icp_plane as IP


def _all(case):
    return [c for e in case.expected() for c in e["clusters"]]


# ---- every option off: the oracle's own chain ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["table", "stops", "tiny", "fallback"])
def test_with_every_option_off_the_reference_is_the_oracle(O, scene):
    base = {"table": S.table_case("r02"), "stops": S.stop_case("unbounded"), "tiny": S.tiny_case(0), "fallback": S.fallback_case()}[scene]
    prm = FR.copy_params(base.prm)
    prm.template_slot = 0
    prm.icp_use_guess = capi.CD_GUESS_NONE
    prm.bbox_enable = 0
    exp = FR.expected(base.frames, prm, base.tpls, FR.options())
    n = 0
    for f, e in enumerate(exp):
        o = O.process_frame(base.frames[f], prm, base.tpls[0], all_clusters=64)
        r = o["result"]
        assert (e["status"], e["counts"], e["ransac_iterations"], e["flags"]) == \
            (r.status, (r.n_cropped, r.n_voxels, r.n_plane, r.n_objects, r.n_clusters), r.ransac_iterations, r.flags)
        assert np.array_equal(e["plane"].view(np.uint32), np.array(list(r.plane), np.float32).view(np.uint32))
        assert np.array_equal(e["plane_inliers"], o["plane_inliers"]) and np.array_equal(e["labels"], o["labels"])
        assert len(e["clusters"]) == len(o["clusters"]) == r.n_clusters
        for c, w in zip(e["clusters"], o["clusters"]):
            assert (c.size, c.iterations, c.converged, c.accepted, c.slot) == (w.size, w.iterations, w.converged, w.accepted, 0)
            assert list(c.T.ravel()) == list(w.T) and c.fitness == w.fitness and c.plane_stats is None
            assert np.array_equal(np.asarray(c.pose), np.array(list(w.pose))) or (np.isnan(c.pose).all() and np.isnan(list(w.pose)).all())
            n += 1
        assert e["outlier"] is None
    assert n > 0


# ---- a. the option table --------------------------------------------------------------------------------------------------------------
def test_table_covers_every_pair_of_option_values():
    assert len(S.TABLE) <= 12 and len(S.ROWS) == len(S.TABLE)
    values = dict(filter=(False, True), plane=(None, (S.W0, S.D0), (S.W0, S.INF)), bound=(False, True),
                  guess=("none", "per_frame", "cluster", "surface"), slot=(0, -1), depth=(False, True), gate=(False, True))
    rows = [dict(filter=r.filter is not None, plane=r.plane, bound=r.bound is not None, guess=r.guess, slot=r.slot, depth=r.depth, gate=r.gate)
            for r in S.TABLE]
    assert all(r[k] in values[k] for r in rows for k in values)
    assert not any(r["bound"] and r["plane"] is None for r in rows)       # not expressible: the oracle has no bound
    for a, b in itertools.combinations(values, 2):
        for va in values[a]:
            for vb in values[b]:
                if {a: va, b: vb} == dict(plane=None, bound=True):
                    continue
                assert any(r[a] == va and r[b] == vb for r in rows), (a, va, b, vb)
    # (e): every option goes on, off and on again along the sequence (the stop batch: C17, per-frame guesses, nothing else)
    seq = [dict(filter=False, plane=True, bound=False, guess=True, slot=False, depth=False, gate=False) if s == "stops" else
           dict(filter=S.ROWS[s].filter is not None, plane=S.ROWS[s].plane is not None, bound=S.ROWS[s].bound is not None,
                guess=S.ROWS[s].guess != "none", slot=S.ROWS[s].slot < 0, depth=S.ROWS[s].depth, gate=S.ROWS[s].gate) for s in S.SEQUENCE]
    assert sum(s != "stops" for s in S.SEQUENCE) == 6
    for k in seq[0]:
        runs = [v for v, _ in itertools.groupby(r[k] for r in seq)]
        assert any(runs[i:i + 3] == [True, False, True] for i in range(len(runs))), (k, runs)


def test_table_batch_is_what_it_says(O):
    prm = S.table_params()
    got = [O.process_frame(fr, prm, S.small_templates()[0])["result"] for fr in S.table_batch()]
    assert got[0].n_clusters == 12 > capi.CD_MAX_CLUSTERS_PER_FRAME
    assert got[1].n_clusters >= 1 and got[2].n_clusters >= 1
    assert got[3].status == capi.CD_OK and got[3].n_objects == 0
    assert got[4].status == capi.CD_ERR_NO_MODEL and got[4].n_cropped == 2
    assert all(len(t) < 1500 and IP.face_axes(t) is not None for t in S.small_templates().values())
    assert prm.icp_max_iterations <= 8


@pytest.fixture(scope="module")
def ungated_objects(O):
    """n_objects of every table frame without the gate, for either input."""
    prm = S.table_params()
    prm.icp_max_iterations = 1
    out = {}
    for depth in (False, True):
        d = S.table_depth()
        frames = [FR.records_of_depth(d[0][f], d[1][f], S.camera()) for f in range(5)] if depth else S.table_batch()
        out[depth] = [O.process_frame(fr, prm, S.small_templates()[0])["result"].n_objects for fr in frames]
    return out


@pytest.mark.parametrize("row_id", [r.id for r in S.TABLE])
def test_table_row_shows_what_it_is_there_for(row_id, ungated_objects):
    row, case = S.ROWS[row_id], S.table_case(row_id)
    exp = case.expected()
    clusters = _all(case)
    print(row_id, [e["counts"][3:] for e in exp], "stopped pairs:", sum(p["stopped"] for c in clusters for p in c.pairs.values()),
          "kept slots:", sorted({c.slot for c in clusters}))
    assert exp[0]["counts"][4] > capi.CD_MAX_CLUSTERS_PER_FRAME and exp[0]["flags"] & capi.CD_FRAME_MORE_CLUSTERS
    assert exp[4]["status"] == capi.CD_ERR_NO_MODEL and exp[3]["counts"][3] == 0
    assert all(c.size >= 60 for c in clusters)
    if row.filter is not None:
        removed = [e["outlier"]["n_removed"] for e in exp]
        assert max(removed) > 0 and min(removed) == 0
    if row.plane is not None:
        assert any(c.plane_stats[0] > 0 for c in clusters)
    if row.bound is not None:       # the bound rejects some but not all correspondences of a cluster's first iteration
        assert any(0 < p["first_kept"] < c.size for c in clusters for p in c.pairs.values())
    if row.slot < 0:
        assert all(sorted(c.pairs) == [0, 1] for c in clusters)
    if row.gate:
        n_o = [e["outlier"]["n_before"] if e["outlier"] else e["counts"][3] for e in exp]
        assert any(a < b for a, b in zip(n_o, ungated_objects[row.depth])) and len(clusters) > 0
    if row.guess == "surface":
        assert any(e["flags"] & capi.CD_FRAME_SURFACE_GUESS for e in exp)
    if row.guess == "cluster":
        assert any(e["flags"] & capi.CD_FRAME_CLUSTER_GUESS for e in exp) and all(c.guess_flip >= 0 for c in clusters)


def test_both_slots_win_somewhere_in_the_table():
    """template_slot = -1: both slots win a cluster, and with C17 on a cluster keeps slot 1 with counters that its slot-0 pair
    does not have (the kept pair's counters are what cd_get_cluster_plane_stats returns)."""
    wins, counters = set(), 0
    for row in S.TABLE:
        if row.slot < 0:
            clusters = _all(S.table_case(row.id))
            wins.update(c.slot for c in clusters)
            if row.plane is not None:
                counters += sum(c.slot == 1 and c.pairs[1]["plane_stats"] != c.pairs[0]["plane_stats"] for c in clusters)
    assert wins == {0, 1} and counters > 0


# ---- b. stops ---------------------------------------------------------------------------------------------------------------------------
def test_the_line_is_one_cluster_with_its_bits_unchanged_and_stops_singular():
    case = S.stop_case("unbounded")
    e = case.expected()[S.LINE_FRAME]
    assert len(e["clusters"]) == 1
    c = e["clusters"][0]
    line = case.frames[S.LINE_FRAME][np.isfinite(case.frames[S.LINE_FRAME][:, 2]) & (case.frames[S.LINE_FRAME][:, 2] == 0.5), :3]
    assert c.size == 41 and np.array_equal(np.sort(c.points.view(np.uint32), axis=0), np.sort(line.view(np.uint32), axis=0))
    assert (c.stopped_singular, c.iterations, c.converged, c.accepted, c.plane_stats) == (1, 0, 0, 0, (0, 0, 1))
    g = case.opt["frame_guesses"][S.LINE_FRAME]
    assert np.array_equal(c.T, g) and c.fitness < FR.MAX_DOUBLE
    tpl = case.tpls[0]
    for sw in (S.D0, S.INF):
        m = IP.icp(tpl, None, c.points, case.prm, S.W0, sw, guess=g)
        assert (m.stopped_singular, m.iterations) == (1, 0)


@pytest.mark.parametrize("kind", ["unbounded", "bounded", "slots"])
def test_stop_batch_has_pairs_behind_its_stops(kind):
    case = S.stop_case(kind)
    exp = case.expected()
    # the driver's queue: every live pair, largest cluster first (a stable sort of the problems, slot-major)
    slots = sorted(case.tpls) if case.prm.template_slot < 0 else [0]
    queue = [(c.size, c.pairs[s]["stopped"], c.pairs[s]["iterations"]) for s in slots for e in exp for c in e["clusters"]]
    queue.sort(key=lambda q: -q[0])
    print(kind, len(queue), "pairs,", sum(q[1] for q in queue), "stopped")
    assert len(queue) > 2                                            # more pairs than the launch's two workgroups
    first_stop = min(i for i, q in enumerate(queue) if q[1])
    behind = [q for q in queue[first_stop + 1:] if not q[1]]
    assert len(behind) >= 3 and all(q[2] > 0 for q in behind)       # with two workgroups, one of them runs after a stop
    line = exp[S.LINE_FRAME]["clusters"][0]
    if kind == "bounded":
        assert all(p["stopped_few"] and p["iterations"] == 0 for c in exp[S.IDENTITY_FRAME]["clusters"] for p in c.pairs.values())
        assert len(exp[S.IDENTITY_FRAME]["clusters"]) >= 1
        # the line under the bound, by the module: its ends (x beyond +-0.12) are further than 0.1 from the template, the 31
        # points kept are still one line: the step is singular as before
        assert (line.first_kept, line.stopped_singular, line.stopped_few) == (31, 1, 0)
    else:
        assert all(p["stopped_singular"] for p in line.pairs.values()) or kind == "slots"
        assert line.pairs[0]["stopped_singular"] == 1
    assert all(e["status"] == capi.CD_OK for e in exp)


# ---- c. tiny clusters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane_on", [1, 0])
def test_tiny_scene_has_single_points_pairs_and_a_real_cluster(plane_on):
    case = S.tiny_case(plane_on)
    assert case.prm.cluster_min_size == 1
    e = case.expected()[0]
    sizes = [c.size for c in e["clusters"]]
    print(sizes)
    assert sizes == [120, 2, 2, 2, 2, 1, 1, 1, 1, 1] and e["flags"] & capi.CD_FRAME_MORE_CLUSTERS
    real = e["clusters"][0]
    assert real.iterations > 0 and real.fitness < FR.MAX_DOUBLE
    for c in e["clusters"][1:]:
        assert (c.iterations, c.converged, c.accepted, c.fitness) == (0, 0, 0, FR.MAX_DOUBLE) and np.array_equal(c.T, FR.IDENT)
        assert c.plane_stats == ((0, 0, 0) if plane_on else None) and np.array_equal(c.aligned, c.points)


# ---- d. the per-template fallback ---------------------------------------------------------------------------------------------------------
def test_fallback_scene_cannot_hold_two_copies_of_its_sources():
    case = S.fallback_case()
    e = case.expected()[0]
    sizes = [c.size for c in e["clusters"]]
    print(sizes, e["outlier"], [(c.slot, {s: p["fitness"] for s, p in c.pairs.items()}) for c in e["clusters"]])
    assert e["outlier"]["n_removed"] > 0 and len(sizes) >= 3
    assert 2 * sum(sizes) > case.N                                   # after the filter
    assert any(c.plane_stats[0] > 0 for c in e["clusters"])
    kept = {c.slot for c in e["clusters"]}
    assert 0 in kept     # a cluster that kept the first slot: its aligned points are not resident after the second pass
    assert any(not np.array_equal(S.aligned_of(case, c), c.aligned) for c in e["clusters"] if c.slot == 0)
